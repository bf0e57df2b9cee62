"""The host-only half of the extended nodes (include/tfhe_gpu.h "Extended nodes"): the levels and the per-level eta
groups of tfhe_lut_circuit_schedule_ext, its refusals, the Python builders' eta arguments, and the identity the
extended select node rests on: for 2m <= N every component of tfhe_lut_generate_ext(eta, m, f) is
tfhe_lut_generate(m, f) word for word, and for m = N and 2N it is not.  No kernel runs here."""
import ctypes as C

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


def schedule_ext(n_inputs, term_off, term_wire, theta, m, sel_off, sel_wire, eta, groups=True):
    """tfhe_lut_circuit_schedule_ext on plain lists -> (status, levels, depth, groups as depth rows of 3)."""
    lib = tfhe_amd.load_library()
    B = len(term_off) - 1
    arrs = [u32(term_off), u32(term_wire), None if theta is None else u32(theta),
            None if sel_off is None else u32(sel_off), u32(sel_wire), None if eta is None else u32(eta)]
    ptr = [None if a is None else a.ctypes.data_as(u32p) for a in arrs]
    levels, depth, grp = np.zeros(max(B, 1), np.uint32), C.c_uint32(0), np.full(3 * max(B, 1), 99, np.uint32)
    rc = lib.tfhe_lut_circuit_schedule_ext(n_inputs, B, ptr[0], ptr[1], ptr[2], m, ptr[3], ptr[4], ptr[5],
                                           levels.ctypes.data_as(u32p), C.byref(depth),
                                           grp.ctypes.data_as(u32p) if groups else None)
    return rc, levels[:B].tolist(), depth.value, grp[:3 * depth.value].reshape(-1, 3).tolist()


# 3 inputs (wires 0..2), m = 2.
#   level 1: nodes 0, 1 ordinary eta = 2; node 2 select eta = 2, entries (w0, const)               -> wires 3, 4, 5
#   level 2: node 3 theta = 1 (wires 6, 7), node 4 ordinary eta = 0 (8), node 5 select eta = 0 (9),
#            node 6 ordinary eta = 1 (10), node 7 select eta = 1 (11), node 8 ordinary eta = 2 (12)
#   level 3: node 9 select eta = 1 whose entries are an extended node's wire (12) and an input wire (1) -> wire 13
MIXED = dict(
    n_inputs=3,
    term_off=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11],
    term_wire=[0, 1, 2, 3, 4, 5, 3, 4, 5, 7, 10],
    theta=[0, 0, 0, 1, 0, 0, 0, 0, 0, 0],
    m=2,
    sel_off=[0, 0, 0, 2, 2, 2, 4, 4, 6, 6, 8],
    sel_wire=[0, CONST, 3, 4, 5, CONST, 12, 1],
    eta=[2, 2, 2, 0, 0, 0, 1, 1, 2, 1],
)


def test_levels_and_groups_of_the_mixed_circuit():
    rc, levels, depth, groups = schedule_ext(**MIXED)
    assert rc == 0 and depth == 3
    assert levels == [1, 1, 1, 2, 2, 2, 2, 2, 2, 3]
    # a level with only eta = 2 nodes; one with all three etas, a theta > 0 node beside the extended ones; the last
    assert groups == [[0, 0, 3], [3, 2, 1], [0, 1, 0]]


def test_eta_does_not_change_a_level_and_null_eta_is_the_select_schedule():
    lib = tfhe_amd.load_library()
    args = {k: v for k, v in MIXED.items() if k != "eta"}
    rc, levels, depth, groups = schedule_ext(**args, eta=None)
    assert rc == 0 and groups == [[3, 0, 0], [6, 0, 0], [1, 0, 0]]
    want, wd = np.zeros(10, np.uint32), C.c_uint32(0)
    keep = [u32(args[k]) for k in ("term_off", "term_wire", "theta", "sel_off", "sel_wire")]
    ptr = [a.ctypes.data_as(u32p) for a in keep]
    assert lib.tfhe_lut_circuit_schedule_select(3, 10, *ptr[:3], 2, *ptr[3:], want.ctypes.data_as(u32p),
                                                C.byref(wd)) == 0
    assert levels == want.tolist() and depth == wd.value
    assert schedule_ext(**MIXED)[1:3] == (levels, depth)
    # no select descriptors either: the multi schedule, and the counts without a buffer are not written
    rc, lv, d, _ = schedule_ext(2, [0, 1, 2], [0, 2], [0, 0], 0, None, [], [1, 2], groups=False)
    assert (rc, lv, d) == (0, [1, 2], 2)


def test_random_circuits_group_counts_are_the_histogram():
    g = rng(15000)
    for _ in range(20):
        B, n_in = int(g.integers(1, 14)), 3
        eta = g.integers(0, 3, B).astype(np.uint32)
        off, wires = [0], []
        for b in range(B):
            wires += g.integers(0, n_in + b, int(g.integers(0, 3))).tolist()
            off.append(len(wires))
        rc, levels, depth, groups = schedule_ext(n_in, off, wires, None, 0, None, [], eta)
        assert rc == 0
        want = np.zeros((depth, 3), int)
        for lv, e in zip(levels, eta):
            want[lv - 1, e] += 1
        assert groups == want.tolist()


# ---- refusals --------------------------------------------------------------------------------------
def bad(**kw):
    return schedule_ext(**{**MIXED, **kw})[0]


@pytest.mark.parametrize("case", [
    dict(eta=[3, 2, 2, 0, 0, 0, 1, 1, 2, 1]),             # eta > TFHE_LUT_EXT_MAX_LOG on an ordinary node
    dict(eta=[2, 2, 2, 0, 0, 0, 1, 1, 2, 3]),             # ... on a select node
    dict(eta=[2, 2, 2, 1, 0, 0, 1, 1, 2, 1]),             # eta > 0 with theta > 0 on one node
    dict(theta=[0, 0, 0, 1, 0, 0, 0, 0, 1, 0]),           # the same from the other side
    dict(theta=[0, 0, 1, 0, 0, 0, 0, 0, 0, 0]),           # theta on a select node (the _select check)
    dict(m=3),                                            # m
    dict(sel_wire=[0, CONST, 3, 4, 5, CONST, 13, 1]),     # the select node's own wire as its entry
    dict(term_wire=[0, 1, 2, 3, 4, 5, 3, 4, 5, 7, 13]),   # a term wire that is not earlier
    dict(term_off=[1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11]),    # term_off not from 0
], ids=str)
def test_schedule_refusals(case):
    assert bad(**case) == INV


def test_null_arguments_and_zero_nodes():
    lib = tfhe_amd.load_library()
    off, so, lv, et = u32([0, 1]), u32([0, 2]), np.zeros(1, np.uint32), u32([1])
    p = lambda a: a.ctypes.data_as(u32p)  # noqa: E731
    w = u32([0, 1])
    f = lib.tfhe_lut_circuit_schedule_ext
    assert f(2, 1, p(off), p(w), None, 2, p(so), p(w), p(et), p(lv), None, None) == 0 and lv[0] == 1
    assert f(2, 1, None, p(w), None, 2, p(so), p(w), p(et), p(lv), None, None) == INV
    assert f(2, 1, p(off), p(w), None, 2, p(so), p(w), p(et), None, None, None) == INV
    assert f(2, 0, None, None, None, 2, p(so), None, None, None, None, None) == 0


def test_device_entries_refuse_a_null_context_and_are_exported():
    lib = tfhe_amd.load_library()
    x = np.zeros(4, np.uint32)
    xp = x.ctypes.data_as(u32p)
    ip = x.view(np.int32).ctypes.data_as(tfhe_amd.i32p)
    assert lib.tfhe_gpu_lut_circuit_eval_ext(None, None, None, 2, 1, xp, 1, xp, xp, ip, xp, xp, None, xp, xp, xp, xp, 1,
                                             xp, xp, None) == INV
    assert lib.tfhe_gpu_lut_circuit_eval_ext_dev(None, None, None, 2, 1, None, 1, xp, xp, ip, xp, xp, None, xp, xp, xp,
                                                 xp, 1, xp, None, None) == INV
    assert lib.tfhe_gpu_lut_select_ext_batch(None, None, 2, 1, xp, 1, xp, xp, ip, xp, xp, xp, xp, 1) == INV
    assert lib.tfhe_gpu_lut_select_ext_dev(None, None, 2, 1, None, 1, xp, xp, ip, xp, xp, xp, None, 1) == INV
    assert lib.tfhe_gpu_bootstrap_lut_each_ext_batch(None, 1, xp, xp, xp, 1) == INV
    assert lib.tfhe_gpu_bootstrap_lut_each_ext_dev(None, 1, None, None, None, 1) == INV
    for name in ("tfhe_gpu_lut_circuit_eval_ext", "tfhe_gpu_lut_circuit_eval_ext_dev", "tfhe_gpu_lut_select_ext_batch",
                 "tfhe_gpu_lut_select_ext_dev", "tfhe_gpu_bootstrap_lut_each_ext_batch",
                 "tfhe_gpu_bootstrap_lut_each_ext_dev", "tfhe_lut_circuit_schedule_ext"):
        assert name in tfhe_amd.EXPORTED_SYMBOLS
    assert lib.tfhe_gpu_abi_version() == 7  # additions only


# ---- the identity ----------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [1, 2])
@pytest.mark.parametrize("m", [2, 16, 32, 64, 512])
def test_every_component_of_the_extended_table_is_the_ordinary_one(m, eta):
    f = rng(15100 + m).integers(0, m, m).astype(np.uint32)
    ext = tfhe_amd.lut_generate_ext(UINT4, eta, m, lambda x: int(f[x])).reshape(1 << eta, 2 * N)
    one = tfhe_amd.lut_generate(UINT4, m, lambda x: int(f[x]))
    for j in range(1 << eta):
        assert np.array_equal(ext[j], one), (m, eta, j)


@pytest.mark.parametrize("eta", [1, 2])
@pytest.mark.parametrize("m", [1024, 2048])
def test_the_identity_stops_at_2m_above_N(m, eta):
    f = (np.arange(m, dtype=np.uint32) * 7 + 1) % m
    ext = tfhe_amd.lut_generate_ext(UINT4, eta, m, lambda x: int(f[x])).reshape(1 << eta, 2 * N)
    one = tfhe_amd.lut_generate(UINT4, m, lambda x: int(f[x]))
    assert any(not np.array_equal(ext[j], one) for j in range(1 << eta))


# ---- the Python builders ---------------------------------------------------------------------------
def test_builders_carry_eta_and_pick_the_entry():
    c = tfhe_amd.LutCircuit()
    x, y = c.input(), c.input()
    a = c.node(0, [(x, 1)], eta=2)
    z = c.node2(4, [(a, 1)], [(y, 1)], 4, eta=1)
    k = c.lookup([[(x, 1)], [(y, 1)]], 0, 4, eta=2)
    assert c.eta == [2, 0, 0, 0, 0, 1, 0, 0, 0, 0, 2] and c.has_ext and (z, k) == (7, 12)
    levels, depth, groups = c.schedule_ext()
    assert depth == 2 and groups.tolist() == [[8, 0, 1], [0, 1, 1]]
    assert c.schedule()[0].tolist() == levels.tolist()
    with pytest.raises(ValueError):
        c.node(0, [(x, 1)], eta=3)
    with pytest.raises(ValueError):
        c.node(0, [(x, 1)], outputs=2, eta=1)
    with pytest.raises(ValueError):
        c.select([(x, 1)], [x, y, x, y], eta=3)
    plain = tfhe_amd.LutCircuit()
    p = plain.input()
    plain.output(plain.node(0, [(p, 1)]))
    assert not plain.has_ext and plain.eta == [0]

    class Recorder:
        """Stands in for a Context: records which entry LutCircuit.run picks."""
        params = UINT4

        def __getattr__(self, name):
            return lambda *a, **kw: name

    assert plain.run(Recorder(), None, np.zeros((1, UINT4.n + 1), np.uint32)) == "lut_circuit_eval"
    assert plain.run_dev(Recorder(), None, 0, 0) == "lut_circuit_eval_dev"
    c.output(z)
    assert c.run(Recorder(), None, np.zeros((2, UINT4.n + 1), np.uint32), packing_key=object()) == "lut_circuit_eval_ext"
    assert c.run_dev(Recorder(), None, 0, 0, packing_key=object()) == "lut_circuit_eval_ext_dev"
