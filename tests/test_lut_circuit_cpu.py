"""The host-only half of LUT circuits: tfhe_lut_circuit_schedule (ASAP levels and its
argument checks), the LutCircuit builder's radix adder, and the planner's stand-alone
test program (zig-tfhe_amd/cpp/test_lut_circuit_cpu.cpp, linked with tfhe_cpu.o alone).
No kernel runs here."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import tfhe_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")
u32p = C.POINTER(C.c_uint32)


def schedule(n_inputs, term_off, term_wire):
    """(status, levels, depth) straight through the C ABI."""
    lib = tfhe_amd.load_library()
    off = np.ascontiguousarray(term_off, np.uint32)
    wire = np.ascontiguousarray(term_wire, np.uint32)
    n = off.size - 1
    levels = np.full(max(n, 1), 99, np.uint32)
    depth = C.c_uint32(99)
    rc = lib.tfhe_lut_circuit_schedule(n_inputs, n, off.ctypes.data_as(u32p), wire.ctypes.data_as(u32p),
                                       levels.ctypes.data_as(u32p), C.byref(depth))
    return rc, levels[:n].tolist(), depth.value


def test_chain():
    c = tfhe_amd.LutCircuit()
    w = c.input()
    for _ in range(5):
        w = c.node(0, [(w, 1)])
    levels, depth = c.schedule()
    assert levels.tolist() == [1, 2, 3, 4, 5] and depth == 5


def test_diamond():
    c = tfhe_amd.LutCircuit()
    a = c.input()
    top = c.node(0, [(a, 1)])
    left, right = c.node(0, [(top, 2)]), c.node(1, [(top, -1), (a, 1)])
    c.node(0, [(left, 1), (right, 1), (a, 3)])
    levels, depth = c.schedule()
    assert levels.tolist() == [1, 2, 2, 3] and depth == 3


def test_node_without_terms_is_level_one():
    c = tfhe_amd.LutCircuit()
    a = c.input()
    k = c.node(0, [], const=1 << 28)  # a trivial ciphertext, bootstrapped
    c.node(0, [(k, 1), (a, 1)])
    levels, depth = c.schedule()
    assert levels.tolist() == [1, 2] and depth == 2


def test_empty_circuit():
    lib = tfhe_amd.load_library()
    depth = C.c_uint32(99)
    assert lib.tfhe_lut_circuit_schedule(3, 0, None, None, None, C.byref(depth)) == 0 and depth.value == 0
    c = tfhe_amd.LutCircuit()
    c.input()
    levels, depth = c.schedule()
    assert levels.size == 0 and depth == 0


def test_forward_and_self_references_are_invalid():
    assert schedule(2, [0, 1, 2], [0, 1]) == (0, [1, 1], 1)
    assert schedule(2, [0, 1, 2], [3, 1])[0] == tfhe_amd.ERR_INVALID  # node 0 reads wire 3 = node 1: forward
    assert schedule(2, [0, 1, 2], [2, 1])[0] == tfhe_amd.ERR_INVALID  # node 0 reads wire 2 = itself
    assert schedule(2, [0, 1, 2], [0, 3])[0] == tfhe_amd.ERR_INVALID  # node 1 reads itself
    assert schedule(2, [0, 1, 2], [0, 2]) == (0, [1, 2], 2)           # node 1 reads node 0: fine


def test_bad_term_off_is_invalid():
    assert schedule(2, [0, 2, 1, 3], [0, 1, 0])[0] == tfhe_amd.ERR_INVALID  # not monotone
    assert schedule(2, [1, 1, 2], [0, 1])[0] == tfhe_amd.ERR_INVALID        # term_off[0] != 0


def test_radix_add_structure():
    """4 digits: per digit a message node and a carry node over the same terms; the carry chain makes
    digit i level i + 1, so 8 nodes at depth 4, and the outputs are 4 message wires + the last carry."""
    c = tfhe_amd.LutCircuit()
    a = [c.input() for _ in range(4)]
    b = [c.input() for _ in range(4)]
    out = c.radix_add(a, b, msg_lut=0, carry_lut=1)
    assert len(c.nodes) == 8 and len(out) == 5
    levels, depth = c.schedule()
    assert depth == 4 and levels.tolist() == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [n[0] for n in c.nodes] == [0, 1] * 4
    assert c.nodes[0][1] == [(a[0], 1), (b[0], 1)]
    carry1 = 8 + 3  # digit 1's carry node
    assert c.nodes[4][1] == c.nodes[5][1] == [(a[2], 1), (b[2], 1), (carry1, 1)]
    assert out == [8, 10, 12, 14, 15]


def test_builder_packs_the_abi_arrays():
    c = tfhe_amd.LutCircuit()
    a, b = c.input(), c.input()
    c.node(2, [(a, 1), (b, -2)], const=0xFFFFFFFF)
    c.node(0)
    d = c.packed()
    assert d.term_off.tolist() == [0, 2, 2] and d.src.tolist() == [0, 1] and d.coef.tolist() == [1, -2]
    assert d.konst.tolist() == [0xFFFFFFFF, 0] and d.lut.tolist() == [2, 0]
    assert d.coef.dtype == np.int32 and d.src.dtype == np.uint32
    with pytest.raises(ValueError):
        c.node(0, [(4, 1)])  # wire 4 does not exist yet
    with pytest.raises(ValueError):
        c.input()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_planner_unit_tests_pass():
    exe = os.path.join(PKG, "lib", "test_lut_circuit_cpu")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
