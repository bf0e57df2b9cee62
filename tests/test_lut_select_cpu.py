"""The host-only half of the select nodes (include/tfhe_gpu.h "Select nodes"): the level schedule of circuits with
select nodes through tfhe_lut_circuit_schedule_select, every refusal that needs no device, the Python builders
(LutCircuit.select / node2 / lookup), and the identity the definition rests on: the pack of trivial ciphertexts
leaves a = 0 and b[i * w] = c_i exactly, so its spread is the generator's table word for word.  No kernel runs here."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import tfhe_amd
from conftest import rng

u32p = C.POINTER(C.c_uint32)
INV = tfhe_amd.ERR_INVALID
CONST = tfhe_amd.LUT_ENTRY_CONST
UINT4 = tfhe_amd.make_params("uint4")
N = UINT4.N


def u32(a):
    return np.ascontiguousarray(a, np.uint32)


def schedule(n_inputs, term_off, term_wire, theta, m, sel_off, sel_wire):
    """tfhe_lut_circuit_schedule_select on plain lists -> (status, levels, depth)."""
    lib = tfhe_amd.load_library()
    B = len(term_off) - 1
    arrs = [u32(term_off), u32(term_wire), None if theta is None else u32(theta),
            None if sel_off is None else u32(sel_off), u32(sel_wire)]
    ptr = [None if a is None else a.ctypes.data_as(u32p) for a in arrs]
    levels, depth = np.zeros(max(B, 1), np.uint32), C.c_uint32(0)
    rc = lib.tfhe_lut_circuit_schedule_select(n_inputs, B, ptr[0], ptr[1], ptr[2], m, ptr[3], ptr[4],
                                              levels.ctypes.data_as(u32p), C.byref(depth))
    return rc, levels[:B].tolist(), depth.value


# ---- schedule --------------------------------------------------------------------------------------
def test_select_sits_one_above_the_deepest_of_terms_and_entries():
    """2 inputs; nodes 0, 1 at level 1, node 2 over node 1 at level 2; select A: x from an input, entries reach
    level 2 -> 3; select B: x from node 2 (level 2), entries inputs and constants only -> 3; select C: nothing but
    constants and no terms -> 1."""
    term_off = [0, 1, 2, 3, 4, 5, 5]
    term_wire = [0, 1, 3, 0, 4]
    sel_off = [0, 0, 0, 0, 4, 8, 12]
    sel_wire = [2, 3, 4, CONST, 0, 1, CONST, CONST, CONST, CONST, CONST, CONST]
    rc, levels, depth = schedule(2, term_off, term_wire, None, 4, sel_off, sel_wire)
    assert rc == 0 and levels == [1, 1, 2, 3, 3, 1] and depth == 3


def test_entry_that_is_an_input_wire_adds_no_level():
    rc, levels, depth = schedule(3, [0, 1], [0], None, 2, [0, 2], [1, 2])
    assert rc == 0 and levels == [1] and depth == 1


def test_two_deep_nesting():
    """Four ordinary nodes, two select nodes over them, one select node over those two (m = 2): levels 1, 2, 3."""
    term_off = [0, 1, 2, 3, 4, 5, 6, 7]
    term_wire = [0, 0, 0, 0, 1, 1, 2]
    sel_off = [0, 0, 0, 0, 0, 2, 4, 6]
    sel_wire = [3, 4, 5, 6, 7, 8]
    rc, levels, depth = schedule(3, term_off, term_wire, None, 2, sel_off, sel_wire)
    assert rc == 0 and levels == [1, 1, 1, 1, 2, 2, 3] and depth == 3


def test_wire_numbering_with_a_multi_output_node_in_front():
    """1 input; node 0 has theta = 1 and drives wires 1 and 2, node 1 (ordinary, over wire 2) wire 3, the select
    node reads x from wire 3 and the entries 1, 2: level 3.  Wire 4, its own, is refused as an entry."""
    rc, levels, depth = schedule(1, [0, 1, 2, 3], [0, 2, 3], [1, 0, 0], 2, [0, 0, 0, 2], [1, 2])
    assert rc == 0 and levels == [1, 2, 3] and depth == 3
    assert schedule(1, [0, 1, 2, 3], [0, 2, 3], [1, 0, 0], 2, [0, 0, 0, 2], [1, 4])[0] == INV


def test_null_sel_off_is_the_multi_schedule():
    lib = tfhe_amd.load_library()
    g = rng(11000)
    B, n_in = 12, 3
    theta = g.integers(0, 3, B).astype(np.uint32)
    first = np.concatenate([[0], np.cumsum(1 << theta)]).astype(int) + n_in
    off, wires = [0], []
    for b in range(B):
        wires += g.integers(0, first[b], int(g.integers(0, 4))).tolist()
        off.append(len(wires))
    rc, levels, depth = schedule(n_in, off, wires, theta, 0, None, [])
    want, wd = np.zeros(B, np.uint32), C.c_uint32(0)
    assert lib.tfhe_lut_circuit_schedule_multi(n_in, B, u32(off).ctypes.data_as(u32p), u32(wires).ctypes.data_as(u32p),
                                               theta.ctypes.data_as(u32p), want.ctypes.data_as(u32p), C.byref(wd)) == 0
    assert rc == 0 and levels == want.tolist() and depth == wd.value
    # and all-empty select descriptors change nothing either
    assert schedule(n_in, off, wires, theta, 4, [0] * (B + 1), []) == (0, want.tolist(), wd.value)


# ---- refusals --------------------------------------------------------------------------------------
OK = dict(n_inputs=2, term_off=[0, 1, 2], term_wire=[0, 1], theta=[0, 0], m=2, sel_off=[0, 0, 2], sel_wire=[0, 2])


def bad(**kw):
    return schedule(**{**OK, **kw})[0]


def test_the_valid_circuit_of_the_refusal_cases_passes():
    assert schedule(**OK) == (0, [1, 2], 2)


@pytest.mark.parametrize("case", [
    dict(sel_off=[0, 0, 1], sel_wire=[0]),            # an entry count other than 0 or m
    dict(sel_off=[0, 0, 4], sel_wire=[0, 1, 0, 1]),   # 2m entries
    dict(sel_off=[0, 2, 2], sel_wire=[0, 2]),         # a forward entry wire: node 0 reads node 0's own wire
    dict(sel_wire=[0, 3]),                            # node 1's own wire
    dict(sel_wire=[0, 7]),                            # no such wire
    dict(theta=[0, 1]),                               # theta on a select node
    dict(sel_off=[1, 1, 3], sel_wire=[0, 0, 1]),      # sel_off does not start at 0
    dict(sel_off=[0, 2, 0], sel_wire=[0, 1]),         # sel_off not monotone
    dict(m=0), dict(m=1), dict(m=3),                  # m
    dict(term_wire=[0, 3]),                           # a term wire that is not earlier (the _multi check)
    dict(term_off=[1, 1, 2]),                         # term_off not from 0
    dict(theta=[4, 0]),                               # theta > TFHE_LUT_MULTI_MAX_LOG
], ids=str)
def test_schedule_refusals(case):
    assert bad(**case) == INV


def test_null_arguments_and_zero_nodes():
    lib = tfhe_amd.load_library()
    off, so, lv = u32([0, 1]), u32([0, 2]), np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data_as(u32p)  # noqa: E731
    w = u32([0, 1])
    assert lib.tfhe_lut_circuit_schedule_select(2, 1, p(off), p(w), None, 2, p(so), p(w), p(lv), None) == 0
    assert lib.tfhe_lut_circuit_schedule_select(2, 1, None, p(w), None, 2, p(so), p(w), p(lv), None) == INV
    assert lib.tfhe_lut_circuit_schedule_select(2, 1, p(off), None, None, 2, p(so), p(w), p(lv), None) == INV
    assert lib.tfhe_lut_circuit_schedule_select(2, 1, p(off), p(w), None, 2, p(so), None, p(lv), None) == INV
    assert lib.tfhe_lut_circuit_schedule_select(2, 1, p(off), p(w), None, 2, p(so), p(w), None, None) == INV
    assert lib.tfhe_lut_circuit_schedule_select(2, 0, None, None, None, 2, p(so), None, None, None) == 0


def test_device_entries_refuse_a_null_context_and_are_exported():
    lib = tfhe_amd.load_library()
    x = np.zeros(4, np.uint32)
    xp = x.ctypes.data_as(u32p)
    ip = x.view(np.int32).ctypes.data_as(tfhe_amd.i32p)
    assert lib.tfhe_gpu_lut_circuit_eval_select(None, None, None, 2, 1, xp, 1, xp, xp, ip, xp, xp, None, xp, xp, xp, 1,
                                                xp, xp, None) == INV
    assert lib.tfhe_gpu_lut_circuit_eval_select_dev(None, None, None, 2, 1, None, 1, xp, xp, ip, xp, xp, None, xp, xp,
                                                    xp, 1, xp, None, None) == INV
    assert lib.tfhe_gpu_lut_select_batch(None, None, 2, xp, 1, xp, xp, ip, xp, xp, xp, xp, 1) == INV
    assert lib.tfhe_gpu_lut_select_dev(None, None, 2, None, 1, xp, xp, ip, xp, xp, xp, None, 1) == INV
    for name in ("tfhe_gpu_lut_circuit_eval_select", "tfhe_gpu_lut_circuit_eval_select_dev",
                 "tfhe_gpu_lut_select_batch", "tfhe_gpu_lut_select_dev", "tfhe_lut_circuit_schedule_select"):
        assert name in tfhe_amd.EXPORTED_SYMBOLS
    assert lib.tfhe_gpu_abi_version() == 7  # additions only


# ---- the Python builders ---------------------------------------------------------------------------
def test_builders_number_wires_and_refuse_what_the_library_would():
    c = tfhe_amd.LutCircuit()
    x, y = c.input(), c.input()
    z = c.node2(16, [(x, 1)], [(y, 1)], 4)
    assert z == 6 and len(c.nodes) == 5 and c.m == 4
    assert [n[0] for n in c.nodes] == [16, 17, 18, 19, 0]
    s = c.select([(z, 1), (x, 2)], [x, ("const", 5), z, y], const=7)
    off, wire, konst = c.select_arrays()
    assert off.tolist() == [0, 0, 0, 0, 0, 4, 8]
    assert wire.tolist() == [2, 3, 4, 5, x, CONST, z, y] and konst.tolist() == [0, 0, 0, 0, 0, 5, 0, 0]
    levels, depth = c.schedule()
    assert levels.tolist() == [1, 1, 1, 1, 2, 3] and depth == 3 and s == 7
    with pytest.raises(ValueError):
        c.select([(x, 1)], [x, y])            # another m in the same circuit
    with pytest.raises(ValueError):
        c.select([(x, 1)], [x, y, z, 8])      # wire 8 does not exist yet
    with pytest.raises(ValueError):
        c.select([(8, 1)], [x, y, z, s])      # nor as a term
    with pytest.raises(ValueError):
        c.node2(0, [(x, 1)], [(y, 1)], 8)
    with pytest.raises(ValueError):
        tfhe_amd.LutCircuit().select([], [0, 0, 0])  # 3 entries
    with pytest.raises(ValueError):
        c.run(SimpleNamespace(params=UINT4), None, np.zeros((2, UINT4.n + 1), np.uint32))  # no packing key
    plain = tfhe_amd.LutCircuit()
    a = plain.input()
    plain.node(0, [(a, 1)])
    assert plain.select_arrays() is None and not plain.has_select


def test_lookup_builds_the_nested_tree():
    """k = 3, m = 4: 16 ordinary nodes on the last digit, 4 select nodes on the middle one, 1 on the first."""
    c = tfhe_amd.LutCircuit()
    d = [c.input() for _ in range(3)]
    out = c.lookup([[(w, 1)] for w in d], 8, 4)
    assert len(c.nodes) == 21 and out == 3 + 20
    assert [n[0] for n in c.nodes[:16]] == list(range(8, 24)) and all(n[1] == [(d[2], 1)] for n in c.nodes[:16])
    assert all(n[1] == [(d[1], 1)] for n in c.nodes[16:20]) and c.nodes[20][1] == [(d[0], 1)]
    assert c.sel[16] == [3, 4, 5, 6] and c.sel[19] == [15, 16, 17, 18] and c.sel[20] == [19, 20, 21, 22]
    levels, depth = c.schedule()
    assert levels.tolist() == [1] * 16 + [2] * 4 + [3] and depth == 3
    one = tfhe_amd.LutCircuit()
    a = one.input()
    assert one.lookup([[(a, 1)]], 5, 4) == 1 and one.nodes == [(5, [(a, 1)], 0)]  # k = 1: an ordinary node


# ---- the trivial-pack identity ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded_packing_key():
    """UINT4's default shape (5, 3): n * t * 2^basebit rows of 2N seeded random words, the k = 0 rows zero as in
    every packing key.  The identity below holds for any rows: the digits of a = 0 are all 0."""
    basebit, t = tfhe_amd.PackingKey.default_shape(UINT4)
    rows = rng(11100).integers(0, 1 << 32, (UINT4.n * t << basebit, 2 * N), dtype=np.uint32)
    rows[::1 << basebit] = 0
    return rows, basebit, t


@pytest.mark.parametrize("m", [2, 4, 16])
def test_pack_of_trivial_entries_then_spread_is_the_generators_table(seeded_packing_key, m):
    rows, basebit, t = seeded_packing_key
    f = lambda x: (7 * x * x + 3 * x + 1) % m  # noqa: E731 (non-monotone)
    w, off = N // m, N // (2 * m)
    c = np.array([((f(i) % m) << 32) // (2 * m) for i in range(m)], np.uint32)  # Encoder.new(m).encode(f(i)), exact
    entries = np.zeros((m, UINT4.n + 1), np.uint32)
    entries[:, -1] = c
    packed = tfhe_amd.pack_tlwe_host(UINT4, rows, basebit, t, entries, np.arange(m, dtype=np.uint32) * w)[0]
    assert not packed[:N].any()
    want_b = np.zeros(N, np.uint32)
    want_b[::w] = c
    assert np.array_equal(packed[N:], want_b)
    tv = tfhe_amd.lut_spread_host(UINT4, packed, w, 2 * N - off)[0]
    assert np.array_equal(tv, tfhe_amd.lut_generate(UINT4, m, f))
