"""The host-only half of the multi-output LUT bootstrap (include/tfhe_gpu.h "Multi-output LUT
bootstrap"): round_theta, the interleaved test vector, the planner's multi-output wire
numbering, and the definition end to end on the oracle: blind_rotate with the interleaved
table on the rounded input, sample_extract_index at 0 and 1, identity_key_switch.  No kernel
runs here."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import tfhe_amd
from conftest import get_keys, rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")
u32p = C.POINTER(C.c_uint32)
UINT4 = tfhe_amd.make_params("uint4")


def words(seed, *shape):
    return rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("theta", [1, 2, 3])
def test_round_gives_multiples_the_mod_switch_keeps(theta):
    x = words(31 + theta, 5, UINT4.n + 1)
    x[0, :4] = [0xFFFFFFFF, 0, (1 << (20 + theta)) - 1, 1 << (20 + theta)]
    r = tfhe_amd.lut_round_tlwe(UINT4, theta, x)
    s = 21 + theta
    want = ((x.astype(np.uint64) + (1 << (s - 1))) & 0xFFFFFFFF & ~np.uint64((1 << s) - 1)).astype(np.uint32)
    assert np.array_equal(r, want)
    assert not (r % (1 << s)).any()
    switched = ((r.astype(np.uint64) + (1 << 20)) & 0xFFFFFFFF) >> 21  # the blind rotation's own mod switch
    assert np.array_equal(switched, r >> 21) and not (switched % (1 << theta)).any()
    assert r[0, 0] == 0 and r[0, 1] == 0  # the wrap at 0xFFFFFFFF
    assert r[0, 2] == 0 and r[0, 3] == 1 << s  # just below half rounds down, half rounds up


def test_round_theta_zero_is_the_identity_and_four_is_refused():
    x = words(35, 3, UINT4.n + 1)
    x[0, 0] = 0xFFFFFFFF
    assert np.array_equal(tfhe_amd.lut_round_tlwe(UINT4, 0, x), x)
    with pytest.raises(tfhe_amd.TfheError) as e:
        tfhe_amd.lut_round_tlwe(UINT4, 4, x)
    assert e.value.status == tfhe_amd.ERR_INVALID


@pytest.mark.parametrize("theta", [1, 2, 3])
def test_interleave_matches_the_formula(theta):
    nu, N = 1 << theta, UINT4.N
    tv = words(40 + theta, nu, 2, N)  # random a halves too
    got = tfhe_amd.lut_interleave(UINT4, tv.reshape(nu, 2 * N)).reshape(2, N)
    q = np.arange(N)
    want = tv[q % nu, :, q - q % nu].T
    assert np.array_equal(got, want)
    # what it is for: X^-r TV at coefficient j is tv_j at r, for r a multiple of nu
    for r in (0, nu, 6 * nu):
        assert np.array_equal(got[:, r:r + nu], tv[np.arange(nu), :, r].T)


def test_interleave_refuses_other_counts():
    with pytest.raises(ValueError):
        tfhe_amd.lut_interleave(UINT4, words(44, 3, 2 * UINT4.N))
    lib = tfhe_amd.load_library()
    tv, out = words(45, 16, 2 * UINT4.N), np.zeros(2 * UINT4.N, np.uint32)
    assert lib.tfhe_lut_interleave(C.byref(UINT4), tv.ctypes.data_as(u32p), 4, out.ctypes.data_as(u32p)) == tfhe_amd.ERR_INVALID


def five_nodes():
    """2 inputs, thetas (0, 1, 0, 2, 1): n0 = f(w0 + w1) -> wire 2; n1 = f(n0) -> 3, 4; n2 = f(w0) -> 5;
    n3 = f(n1[1] + n2) -> 6..9; n4 = f(n0 - w1) -> 10, 11."""
    c = tfhe_amd.LutCircuit()
    a, b = c.input(), c.input()
    n0 = c.node(0, [(a, 1), (b, 1)])
    n1 = c.node(1, [(n0, 1)], outputs=2)
    n2 = c.node(2, [(a, 1)])
    n3 = c.node(1, [(n1[1], 1), (n2, 1)], outputs=4)
    n4 = c.node(0, [(n0, 1), (b, -1)], outputs=2)
    return c, (n0, n1, n2, n3, n4)


def test_builder_numbers_the_wires_over_all_outputs():
    c, (n0, n1, n2, n3, n4) = five_nodes()
    assert (n0, n1, n2, n3, n4) == (2, [3, 4], 5, [6, 7, 8, 9], [10, 11])
    assert c.theta == [0, 1, 0, 2, 1] and c.multi and c.n_wires == 12
    levels, depth = c.schedule()
    assert levels.tolist() == [1, 2, 1, 3, 2] and depth == 3
    with pytest.raises(ValueError):
        c.node(0, [(12, 1)])  # the next node's own first wire
    with pytest.raises(ValueError):
        c.node(0, [(0, 1)], outputs=3)


def schedule_multi(n_inputs, term_off, term_wire, theta):
    lib = tfhe_amd.load_library()
    off, wire = np.ascontiguousarray(term_off, np.uint32), np.ascontiguousarray(term_wire, np.uint32)
    th = None if theta is None else np.ascontiguousarray(theta, np.uint32)
    n = off.size - 1
    levels, depth = np.full(max(n, 1), 99, np.uint32), C.c_uint32(99)
    rc = lib.tfhe_lut_circuit_schedule_multi(n_inputs, n, off.ctypes.data_as(u32p), wire.ctypes.data_as(u32p),
                                             None if th is None else th.ctypes.data_as(u32p),
                                             levels.ctypes.data_as(u32p), C.byref(depth))
    return rc, levels[:n].tolist(), depth.value


def test_schedule_multi_checks_the_wires():
    off, wire, theta = [0, 2, 3, 4, 6, 8], [0, 1, 2, 0, 4, 5, 2, 1], [0, 1, 0, 2, 1]
    assert schedule_multi(2, off, wire, theta) == (0, [1, 2, 1, 3, 2], 3)
    for k, w in ((2, 3), (2, 4), (4, 6), (4, 9), (4, 10)):  # own first / second wire, own wires, a later node's
        bad = list(wire)
        bad[k] = w
        assert schedule_multi(2, off, bad, theta)[0] == tfhe_amd.ERR_INVALID, (k, w)
    assert schedule_multi(2, off, wire, [0, 1, 4, 2, 1])[0] == tfhe_amd.ERR_INVALID  # theta > 3
    # theta = NULL is the existing schedule: there wire 4 is node 2, which node 3 may read, and wire 5 is itself
    assert schedule_multi(2, off, wire, None)[0] == tfhe_amd.ERR_INVALID
    single = [0, 1, 2, 0, 4, 3, 2, 1]
    lib = tfhe_amd.load_library()
    o, w = np.array(off, np.uint32), np.array(single, np.uint32)
    levels, depth = np.zeros(5, np.uint32), C.c_uint32(0)
    assert lib.tfhe_lut_circuit_schedule(2, 5, o.ctypes.data_as(u32p), w.ctypes.data_as(u32p),
                                         levels.ctypes.data_as(u32p), C.byref(depth)) == 0
    assert schedule_multi(2, off, single, None) == (0, levels.tolist(), depth.value)
    assert schedule_multi(2, off, single, [0] * 5) == (0, levels.tolist(), depth.value)


def test_radix_add_fused_structure():
    """4 digits: one two-output node per digit, the carry chain through the node's second wire."""
    c = tfhe_amd.LutCircuit()
    a = [c.input() for _ in range(4)]
    b = [c.input() for _ in range(4)]
    out = c.radix_add_fused(a, b, lut=0)
    assert len(c.nodes) == 4 and c.theta == [1] * 4 and out == [8, 10, 12, 14, 15]
    assert c.nodes[2][1] == [(a[2], 1), (b[2], 1), (11, 1)]
    levels, depth = c.schedule()
    assert levels.tolist() == [1, 2, 3, 4] and depth == 4


def test_definition_decrypts_on_the_oracle(oracle):
    """UINT4, seeded keys, m = 8, theta = 1, tables x mod 4 and x div 4 interleaved: for every message the
    oracle's blind rotation of the rounded input with the interleaved table, extracted at coefficients 0
    and 1 and key switched, decrypts to (x mod 4, x div 4).  Margin N / (2m) = 64 positions against the
    rounding's sigma of 11.7."""
    k = get_keys(oracle, "uint4")
    sk = tfhe_amd.SecretKey(UINT4, k.k0, k.k1)
    m = 8
    tv = tfhe_amd.lut_interleave(UINT4, [tfhe_amd.lut_generate(UINT4, m, lambda x: x % 4),
                                         tfhe_amd.lut_generate(UINT4, m, lambda x: x // 4)])
    cts = sk.encrypt_lwe_message(np.arange(m, dtype=np.uint32), m, seed0=8100)
    x = tfhe_amd.lut_round_tlwe(UINT4, 1, cts)
    got = []
    for i in range(m):
        acc = oracle.blind_rotate(k.p, x[i], tv, k.ck.bk, k.ck.offset)
        outs = [oracle.identity_key_switch(k.p, oracle.sample_extract_index(acc, j), k.ck.ksk) for j in (0, 1)]
        got.append(tuple(int(v) for v in sk.decrypt_lwe_message(np.array(outs), m)))
    assert got == [(i % 4, i // 4) for i in range(m)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_host_unit_tests_pass():
    exe = os.path.join(PKG, "lib", "test_lut_multi_cpu")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
