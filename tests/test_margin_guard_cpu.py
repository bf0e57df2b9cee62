"""The fixtures of tests/margin_guard_cases.py, proven on the oracle (no kernel runs here).  The GPU
tests of the margin guard (tests/test_margin_guard.py) count on three facts about
the crafted key of conftest.crafted_near_tie_case:

 - every HOT ciphertext of the pool parts: the oracle's fused arithmetic, in the whole form's MAC
   order and in the latency form's, gives other accumulator words than the reference's trees, so a
   fused kernel without the recompute launch returns wrong words for it;
 - every QUIET ciphertext never parts, with any test vector, and a hot ciphertext with a random
   table does not part either: such items bound the recompute counter from above;
 - the words that differ never include a[0] or b[0].  A key switch with a zero KSK returns
   (0, ..., 0, b[0]) and cannot see the recompute, which is why the GPU tests load a real KSK; the
   lv1-extracted a words 1 .. N-1 do differ.

Both parameter sets of the GPU tests: the 128-bit set (L = 3) and l2small (L = 2)."""
import numpy as np
import pytest

import margin_guard_cases as mg
import tfhe_amd
from conftest import rng

# (fused, regroup) of the oracle that model the product's fused forms: the whole form's MAC order
# and the latency form's (oracle.set_regroup)
FUSED_ORDERS = [0, 2]
# 128-bit set, whole-form order: the accumulator indices (of both halves) where the fused arithmetic
# parts from the reference on a hot ciphertext
PARTED_128 = [245, 249, 252, 254, 255, 737, 747, 748, 749, 750, 752, 753, 758, 759, 766, 767, 980, 986, 996, 1005, 1011]


@pytest.fixture(scope="module", params=["128", "l2small"])
def case(request, oracle):
    """(params, offset, crafted test vector, crafted BK, reference accumulators of the hot pool)."""
    p = mg.oracle_params(request.param)
    off, tv, bk = mg.crafted_key(oracle, p)
    hot = np.array([mg.hot(p, j) for j in range(len(mg.HOT_POOL))])
    return request.param, p, off, tv, bk, hot, mg.rotate(oracle, p, hot, tv, bk, off)


def test_pools_are_what_they_say(case):
    _, p, *_ = case
    for j, (w0, wn) in enumerate(mg.HOT_POOL):
        ct = mg.hot(p, j)
        assert mg.is_hot(p, ct) and (w0 is None or (ct[0], ct[p.n]) == (w0, wn))
        assert np.array_equal(ct, mg.hot(p, j + len(mg.HOT_POOL)))  # cyclic, deterministic
    for j in range(len(mg.QUIET_POOL)):
        ct = mg.quiet(p, j)
        assert mg.is_quiet(p, ct) and not mg.is_hot(p, ct)
    # the four window edges, and the words next to them outside
    assert [mg.switched(w) for w in (0x7FF00000, 0x800FFFFF, 0x7FEFFFFF, 0x80100000)] == [p.N, p.N, p.N - 1, p.N + 1]
    assert [mg.switched(w) for w in (0xFFF00000, 0xFFFFF, 0xFFEFFFFF, 0x100000)] == [2 * p.N, 0, 2 * p.N - 1, 1]
    # distinct pool entries differ in their free words, so a batch's neighbours are different inputs
    assert len({mg.hot(p, j)[1:p.n].tobytes() for j in range(8)} | {mg.quiet(p, j)[1:p.n].tobytes() for j in range(8)}) == 16


@pytest.mark.parametrize("regroup", FUSED_ORDERS)
def test_every_hot_ciphertext_parts(oracle, case, regroup):
    """Fused != reference for all 8 pool entries in both MAC orders; the differing words include
    lv1-extracted positions (a-half indices other than 0) and never a[0] or b[0]."""
    name, p, off, tv, bk, hot, ref = case
    fused = mg.rotate(oracle, p, hot, tv, bk, off, 1, regroup)
    diff = fused != ref
    assert diff.any(axis=1).all(), np.flatnonzero(~diff.any(axis=1)).tolist()
    assert diff[:, 1:p.N].any(axis=1).all()
    assert not diff[:, 0].any() and not diff[:, p.N].any()
    if name == "128" and regroup == 0:
        for d in diff:
            assert np.flatnonzero(d).tolist() == PARTED_128 + [p.N + i for i in PARTED_128]


def test_guarded_oracle_returns_the_reference_on_hot_ciphertexts(oracle, case):
    """The oracle's own model of the guard (set_fused(2)): the reference's words."""
    _, p, off, tv, bk, hot, ref = case
    assert np.array_equal(mg.rotate(oracle, p, hot[:3], tv, bk, off, 2), ref[:3])


def test_quiet_ciphertexts_never_part(oracle, case):
    """All 8 quiet pool entries with the crafted test vector, the first 4 (the window's edges among
    them) with a random table too, in both MAC orders."""
    _, p, off, tv, bk, _, _ = case
    quiet = np.array([mg.quiet(p, j) for j in range(len(mg.QUIET_POOL))])
    for table, cts in ((tv, quiet), (mg.words(rng(7200), 2 * p.N), quiet[:4])):
        ref = mg.rotate(oracle, p, cts, table, bk, off)
        for regroup in FUSED_ORDERS:
            assert np.array_equal(mg.rotate(oracle, p, cts, table, bk, off, 1, regroup), ref), regroup


@pytest.mark.parametrize("regroup", FUSED_ORDERS)
def test_a_hot_ciphertext_with_a_random_table_does_not_part(oracle, case, regroup):
    """The per-item-table cases lean on this: an item that reads a random table where its own is the
    crafted one is not recomputed into the right words by accident, and it is not a parting item."""
    _, p, off, tv, bk, hot, ref = case
    table = mg.words(rng(7201), 2 * p.N)
    got = mg.rotate(oracle, p, hot[:4], table, bk, off, 1, regroup)
    assert np.array_equal(got, mg.rotate(oracle, p, hot[:4], table, bk, off))
    assert (got != ref[:4]).any(axis=1).all()  # and the table matters to every item


def test_gate_pairs_combine_to_the_pool(oracle, case):
    """Every op the gate entries accept: hot_gate_pair solves exactly (XOR and XNOR too: a's coefficient
    is +-1), and gate_items reproduces ct_items word for word, so the gate tests' pre-combinations
    are pool entries."""
    _, p, *_ = case
    for op in mg.GATE_OPS:
        a, b = mg.hot_gate_pair(oracle, p, op, 7300 + op)
        assert mg.is_hot(p, oracle.gate_combine(p, op, a, b)), op
        assert not np.array_equal(a, b)
    ops = np.array(mg.GATE_OPS + [3, 4], np.uint8)
    hot_at = [0, 2, 3, 5, 6, 8, 9, 10, 11, 12]
    A, B = mg.gate_items(oracle, p, ops, hot_at, 7400)
    got = np.array([oracle.gate_combine(p, int(op), a, b) for op, a, b in zip(ops, A, B)])
    assert np.array_equal(got, mg.ct_items(p, len(ops), hot_at))
    assert [mg.is_hot(p, x) for x in got] == [i in hot_at for i in range(len(ops))]


def test_rounded_hot_inputs_stay_in_the_pool_windows(oracle):
    """round_theta (theta = 1, multiples of 2^22) of a hot ciphertext is hot (both windows round to
    their centres) and parts; of a quiet one, quiet.  Interleaving two copies of the crafted constant
    gives the crafted constant.  This is the multi-output node of the GPU tests (128-bit set)."""
    p = mg.oracle_params("128")
    off, tv, bk = mg.crafted_key(oracle, p)
    hot = np.array([mg.hot(p, j) for j in range(len(mg.HOT_POOL))])
    params = tfhe_amd.make_params("128")
    r = tfhe_amd.lut_round_tlwe(params, 1, hot)
    assert all(mg.is_hot(p, x) for x in r) and not np.array_equal(r, hot)
    assert all(x[0] == 1 << 31 and x[p.n] == 0 for x in r)
    q = tfhe_amd.lut_round_tlwe(params, 1, np.array([mg.quiet(p, j) for j in range(8)]))
    assert all(mg.is_quiet(p, x) for x in q)
    assert np.array_equal(tfhe_amd.lut_interleave(params, np.stack([tv, tv])), tv)
    ref = mg.rotate(oracle, p, r[:3], tv, bk, off)
    for regroup in FUSED_ORDERS:
        diff = mg.rotate(oracle, p, r[:3], tv, bk, off, 1, regroup) != ref
        # the fan-out extracts coefficients 0 and 1: a-half indices other than 0 reach both outputs
        assert diff[:, 1:p.N].any(axis=1).all()
