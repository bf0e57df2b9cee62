"""The margin guard's recompute launch on every fused launch path: each test puts
items the fused arithmetic is known to get wrong (HOT, tests/margin_guard_cases.py; proven on the
oracle by tests/test_margin_guard_cpu.py) at chosen positions of a batch of items no fused form can
flag (QUIET), forces the fused arithmetic, and compares every output word for word with the
reference's trees.  A hot item that the recompute launch misses, or redoes from the wrong ops,
operands, indices, table or flag offset, comes back with the fused kernel's words or another
item's, and the comparison fails; there is no tolerance anywhere.

Setup: one context at the 128-bit set with the crafted test vector and BK and the seeded key's
KSK.  The fused arithmetic parts from the reference in accumulator words other than a[0] and b[0]
only, so a zero KSK, whose key switch returns (0, ..., 0, b[0]), would hide the recompute.

Counter: delta, the rise of near_tie_items() over a call, satisfies parted <= delta <= hot, where
hot counts the items that are not quiet and parted the hot items whose oracle fused mode (in the
form's MAC order) differs from its reference mode.  Every pool entry parts, so this is delta == hot
wherever the batch is made of pool entries only."""
import types

import numpy as np
import pytest

import margin_guard_cases as mg
import tfhe_amd
from conftest import get_keys, rng
from test_lut_circuit import oracle_nodes
from test_lut_multi import oracle_composition

pytestmark = pytest.mark.gpu

FUSED, REFERENCE = tfhe_amd.ARITH_FUSED_FORCED, tfhe_amd.ARITH_REFERENCE
FUSED_KERNEL = {  # the first launch of a forced-fused call, per set and form (auto below 512 items: the latency form)
    ("128", "whole"): "k_blind_rotate_assist<true> (whole form, loader waves own polynomial b, fused)",
    ("128", "wide"): "k_blind_rotate_wide<3,true,true> (latency form, fused)",
    ("l2small", "whole"): "k_blind_rotate<2,true,true> (whole form, fused)",
    ("l2small", "wide"): "k_blind_rotate_wide<2,true,true> (latency form, fused)",
}
FUSED_KERNEL_TV = {"whole": "k_blind_rotate_assist<true,TV>", "wide": "k_blind_rotate_wide<3,true,true,TV>"}
SMALL_FORM = {"auto": "wide", "whole": "whole", "wide": "wide"}  # the form a batch below 512 items runs in


class Env:
    """A context with the crafted key of one set, the oracle's view of that key, and the oracle's
    accumulators computed so far (every batch here is made of the same 16 pool ciphertexts)."""

    def __init__(self, oracle, name):
        from oracle import CloudKeyArrays
        self.name, self.p = name, mg.oracle_params(name)
        p = self.p
        self.off, self.tv, self.bk = mg.crafted_key(oracle, p)
        if name == "128":
            ksk = get_keys(oracle, "128").ck.ksk
            self.c = tfhe_amd.Context("128", 0)
        else:  # only accumulators are compared at l2small: uniform words are as good a KSK as any
            ksk = mg.words(rng(7500), p.N * p.iks_t * (1 << p.basebit), p.n + 1)
            self.c = tfhe_amd.Context(tfhe_amd.make_params(mg.L2SMALL), 0)
        self.keys = CloudKeyArrays(self.off, self.tv, ksk, self.bk)
        self.k = types.SimpleNamespace(p=p, ck=self.keys)  # what the other modules' oracle helpers take
        self.c.load_cloud_key(self.off, self.tv, self.bk, ksk)
        self.acc = {}

    def rotate(self, oracle, cts, tvs=None, fused=0, regroup=0):
        """The oracle's accumulators of cts (test vector: the key's, one (2N,), or one per item), memoised."""
        tvs = np.asarray(self.tv if tvs is None else tvs, np.uint32)
        out = []
        for i, ct in enumerate(cts):
            tv = tvs if tvs.ndim == 1 else tvs[i]
            key = (ct.tobytes(), tv.tobytes(), fused, regroup if fused else 0)
            if key not in self.acc:
                self.acc[key] = mg.rotate(oracle, self.p, ct[None], tv, self.bk, self.off, fused, regroup)[0]
            out.append(self.acc[key])
        return np.array(out)

    def parted(self, oracle, cts, form, tvs=None):
        """How many of cts part in the oracle's fused mode with the form's MAC order."""
        regroup = mg.FORM_REGROUP[form]
        return int((self.rotate(oracle, cts, tvs, 1, regroup) != self.rotate(oracle, cts, tvs)).any(axis=1).sum())


@pytest.fixture(scope="module")
def env(oracle):
    e = Env(oracle, "128")
    yield e
    e.c.close()


def forced(c, call, form="auto", **opts):
    """call() under forced fused arithmetic in `form` -> (result, rise of near_tie_items, first kernel)."""
    before = c.near_tie_items()
    with c.options(br_form=form, arith=FUSED, **opts):
        out = call()
        c.sync()  # the _dev entries are asynchronous; the counter is read at a synchronisation
        kernel = c.last_kernels().split(" + ")[0]
    return out, c.near_tie_items() - before, kernel


def reference(c, call, form="auto", **opts):
    with c.options(br_form=form, arith=REFERENCE, **opts):
        out = call()
        c.sync()
        assert "fused" not in c.last_kernels()
    return out


def same(got, want, what=""):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))
    assert bad.size == 0, (what, bad[:12].tolist())


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).to("cuda:0")


def from_dev(t):
    return t.cpu().numpy().view(np.uint32)


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the setup itself ------------------------------------------------------------------------------
def test_default_arithmetic_refuses_the_crafted_key(oracle, env):
    """The key admission refuses the crafted key the fused arithmetic (its BK spectrum is past 2^39):
    the default runs the reference's trees over hot items and recomputes nothing.  Everything else in
    this module forces the fused arithmetic."""
    c, p = env.c, env.p
    assert c.get_option("fused_admitted") == 0
    cts = mg.ct_items(p, 6, [2, 5])
    before = c.near_tie_items()
    for form in ("auto", "whole"):
        with c.options(br_form=form):
            same(c.blind_rotate_batch(cts, env.tv), env.rotate(oracle, cts), form)
            assert "fused" not in c.last_kernels()
    assert c.near_tie_items() == before


def test_the_octo_form_does_not_exist_at_l3(env):
    """The octo form is instantiated at L = 1 only, outside the exact-integer regime, so its
    near_tie_flag site cannot run fused: the option is refused here.  If it ever is accepted, the
    positions test below needs an "octo" case."""
    with pytest.raises(tfhe_amd.TfheError):
        env.c.set_option("br_form", "octo")
    assert env.c.get_option("br_form") == 0


# ---- positions and the ragged group ----------------------------------------------------------------
POSITIONS_B, POSITIONS_HOT = 11, [0, 3, 4, 5, 10]


def positions_case(oracle, e, form):
    """B = 11, hot at {0, 3, 4, 5, 10}: two in one whole-form group of 4, two in the next, the last item
    in the ragged group (its three padding waves compute copies of item 10 with valid == false).  Full
    accumulators; then the same shape all quiet: nothing recomputed, so the first call left no flag."""
    c, p = e.c, e.p
    cts = mg.ct_items(p, POSITIONS_B, POSITIONS_HOT)
    got, delta, kernel = forced(c, lambda: c.blind_rotate_batch(cts, e.tv), form)
    assert kernel == FUSED_KERNEL[e.name, SMALL_FORM[form]]
    same(got, e.rotate(oracle, cts), form)
    hot = cts[POSITIONS_HOT]
    print(f"{e.name} {form}: {delta} of {len(hot)} hot items recomputed")
    assert e.parted(oracle, hot, form) <= delta <= len(hot)
    quiet = mg.ct_items(p, POSITIONS_B, [], first=3)
    got, delta, _ = forced(c, lambda: c.blind_rotate_batch(quiet, e.tv), form)
    assert delta == 0
    same(got, e.rotate(oracle, quiet), form + " quiet")


@pytest.mark.parametrize("form", ["auto", "whole", "wide"])
def test_positions_and_the_ragged_group(oracle, env, form):
    positions_case(oracle, env, form)


def test_positions_and_the_ragged_group_at_l2(oracle):
    """l2small: k_blind_rotate<2,true,true> is the plain whole form, another kernel than the assist form."""
    e = Env(oracle, "l2small")
    try:
        assert e.c.get_option("fused_admitted") == 0
        for form in ("whole", "auto"):
            positions_case(oracle, e, form)
    finally:
        e.c.close()


# ---- output modes and ops --------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["auto", "whole"])
def test_bootstrap_with_and_without_key_switch(oracle, env, form):
    """BR_OUT_LV1 with the key switch behind it, and BR_OUT_LV0_EXTRACT2: B = 7, hot at {1, 2, 6}."""
    c, p = env.c, env.p
    hot_at = [1, 2, 6]
    cts = mg.ct_items(p, 7, hot_at, first=5)
    parted = env.parted(oracle, cts[hot_at], form)
    got, delta, kernel = forced(c, lambda: c.bootstrap_batch(cts), form)
    assert kernel == FUSED_KERNEL["128", SMALL_FORM[form]]
    same(got, np.array([oracle.bootstrap(p, x, env.keys) for x in cts]), "bootstrap")
    assert parted <= delta <= len(hot_at)
    got, delta, kernel = forced(c, lambda: c.bootstrap_without_key_switch_batch(cts), form)
    assert kernel == FUSED_KERNEL["128", SMALL_FORM[form]]
    same(got, np.array([oracle.bootstrap_without_key_switch(p, x, env.keys) for x in cts]), "without key switch")
    assert parted <= delta <= len(hot_at)


@pytest.mark.parametrize("form", ["auto", "whole"])
def test_gate_batch_every_op(oracle, env, form):
    """One hot item per op (the ten gates and COPY), each followed by a quiet one of the same op:
    B = 22, hot at the even indices.  The recompute reads ops and in_b as the first launch did."""
    c, p = env.c, env.p
    ops = np.repeat(np.array(mg.GATE_OPS, np.uint8), 2)
    hot_at = list(range(0, len(ops), 2))
    assert len(ops) % 4 != 0
    A, Bv = mg.gate_items(oracle, p, ops, hot_at, 7600)
    got, delta, kernel = forced(c, lambda: c.gate_batch(ops, A, Bv), form)
    assert kernel == FUSED_KERNEL["128", SMALL_FORM[form]]
    same(got, oracle.gate_batch(p, ops, A, Bv, env.keys, threads=8), form)
    assert env.parted(oracle, mg.ct_items(p, len(ops), hot_at)[hot_at], form) <= delta <= len(hot_at)


# ---- the tail split and the pipeline ----------------------------------------------------------------
def big_gate_case(oracle, e, hot_at, seed):
    """B = 4 x CUs + 3 gates, ops cycling through all eleven, hot at hot_at."""
    B = 4 * cus() + 3
    ops = np.array([mg.GATE_OPS[i % 11] for i in range(B)], np.uint8)
    A, Bv = mg.gate_items(oracle, e.p, ops, hot_at, seed)
    return B, ops, A, Bv


def check_big_gate_batch(oracle, e, run, ops, A, Bv, hot_at, probe, what):
    """run() under forced fused arithmetic: the whole batch equals the same call in the reference's
    trees, the probes equal the oracle, the counter bound holds."""
    got, delta, kernel = forced(e.c, run)
    assert kernel == FUSED_KERNEL["128", "whole"], kernel
    same(got, reference(e.c, run), what + " vs reference trees")
    probe = np.array(sorted(set(probe)))
    same(got[probe], oracle.gate_batch(e.p, ops[probe], A[probe], Bv[probe], e.keys, threads=8), what + " vs oracle")
    hot = mg.ct_items(e.p, len(ops), hot_at)[hot_at]
    # the full rounds run the whole form, the 3-item tail the latency form: either order parts every pool entry
    parted = min(e.parted(oracle, hot, "whole"), e.parted(oracle, hot, "wide"))
    print(f"{what}: {delta} of {len(hot_at)} hot items recomputed")
    assert parted <= delta <= len(hot_at)


def test_tail_split_shifts_the_flags(oracle, env):
    """PLAN_WHOLE_TAIL through gate_batch_dev: the full rounds in the whole form, the 3-item tail in
    the latency form with tie_flags + full, and one recompute launch over all B items.  Hot on both
    sides of the split and at both ends; then the same shape all quiet recomputes nothing."""
    import torch
    c = env.c
    full = 4 * cus()
    hot_at = [0, full - 1, full, full + 1, full + 2]
    B, ops, A, Bv = big_gate_case(oracle, env, hot_at, 7700)
    assert hot_at[-1] == B - 1
    t_ops, t_a, t_b = to_dev(ops), to_dev(A), to_dev(Bv)
    t_out = torch.zeros_like(t_a)
    torch.cuda.synchronize()

    def run():
        t_out.zero_()
        torch.cuda.synchronize()
        c.gate_batch_dev(t_ops.data_ptr(), t_a.data_ptr(), t_b.data_ptr(), t_out.data_ptr(), B)
        c.sync()
        return from_dev(t_out)
    check_big_gate_batch(oracle, env, run, ops, A, Bv, hot_at, hot_at + [1, full - 2], "tail split")
    Aq, Bq = mg.gate_items(oracle, env.p, ops, [], 7700)
    t_a.copy_(to_dev(Aq))
    t_b.copy_(to_dev(Bq))
    torch.cuda.synchronize()
    got, delta, _ = forced(c, run)
    assert delta == 0
    same(got, reference(c, run), "tail split, all quiet")


def test_tail_split_shifts_the_selectors_with_the_flags(oracle, env):
    """The same shape through lut_apply with the set {random table, crafted test vector}: hot items
    select table 1, quiet ones table 0, so the tail launch needs tv_sel + full and tie_flags + full
    together (item full + 1 is hot where item 1 is quiet)."""
    c, p = env.c, env.p
    full = 4 * cus()
    B = full + 3
    hot_at = [0, full - 1, full, full + 1, full + 2]
    pool = mg.ct_items(p, B, hot_at)
    tables = np.stack([mg.words(rng(7701), 2 * p.N), env.tv])
    nodes = [(1 if i in hot_at else 0, [(i, 1)], 0) for i in range(B)]
    ls = tfhe_amd.LutSet(c, tables)
    try:
        run = lambda: c.lut_apply(ls, pool, nodes)
        got, delta, kernel = forced(c, run)
        assert kernel.startswith(FUSED_KERNEL_TV["whole"]) and kernel.endswith("fused)"), kernel
        same(got, reference(c, run), "vs reference trees")
    finally:
        ls.close()
    probe = sorted(hot_at + [1, full - 2])
    want = oracle_nodes(oracle, p, env.keys, pool, nodes, tables, only=probe)
    same(got[probe], want[probe], "vs oracle")
    parted = min(env.parted(oracle, pool[hot_at], form) for form in ("whole", "wide"))
    assert parted <= delta <= len(hot_at)


def test_pipeline_offsets_the_flags_per_chunk(oracle, env):
    """TFHE_OPT_HOST_PIPELINE: gate_batch on host buffers in chunks of #CUs items on four streams, each
    chunk's launches with tie_flags + k0.  Hot at chunk edges of every stream and in the short last
    chunk; the counter is read after the call, which sums it after all streams have synchronised."""
    c = env.c
    n = cus()
    hot_at = [0, n - 1, n, 2 * n, 4 * n, 4 * n + 2]
    B, ops, A, Bv = big_gate_case(oracle, env, hot_at, 7800)
    assert hot_at[-1] == B - 1

    def run():
        with c.options(host_pipeline=1):
            return c.gate_batch(ops, A, Bv)
    check_big_gate_batch(oracle, env, run, ops, A, Bv, hot_at, hot_at + [1, n - 2, n + 1, 4 * n + 1], "pipeline")
    # host buffers with the pipeline off (the default) take the tail split: the same words and count
    plain, delta, _ = forced(c, lambda: c.gate_batch(ops, A, Bv))
    same(plain, reference(c, run), "one stream vs pipeline")
    assert env.parted(oracle, mg.ct_items(env.p, B, hot_at)[hot_at], "whole") <= delta <= len(hot_at)


# ---- circuits --------------------------------------------------------------------------------------
def test_circuit_gathers_by_index_in_the_recompute(oracle, env):
    """Level 1: 13 gates of every op over a shared pool, read through indices (in_a != in_b, neither the
    gate's own position), hot and quiet; level 2: 6 gates over level 1's outputs, the hot ones
    included.  circuit_eval and circuit_eval_dev, latency and whole form: the oracle gate by gate."""
    import torch
    c, p = env.c, env.p
    ops1 = np.array(mg.GATE_OPS + [3, 0], np.uint8)
    G1, hot_at = len(ops1), [0, 2, 3, 7, 10, 12]
    target = mg.ct_items(p, G1, hot_at, first=1)
    shared = mg.words(rng(7900), 3, p.n + 1)  # the b operands: three ciphertexts every gate shares
    a_of = [mg.solve_gate_pair(oracle, p, int(op), t, shared[g % 3]) for g, (op, t) in enumerate(zip(ops1, target))]
    inputs = np.zeros((G1 + 3, p.n + 1), np.uint32)
    in_a1 = (np.arange(G1) + 5) % G1  # gate g's a operand sits at input (g + 5) mod 13
    inputs[in_a1], inputs[G1:] = np.array(a_of), shared
    in_b1 = G1 + np.arange(G1) % 3
    assert (in_a1 != np.arange(G1)).all() and (in_a1 != in_b1).all()
    w1 = len(inputs) + np.arange(G1)  # level 1's wires
    ops2 = np.array([0, 3, 7, 255, 4, 9], np.uint8)
    a2, b2 = w1[[0, 2, 1, 3, 12, 10]], w1[[1, 7, 0, 4, 5, 11]]
    ops = np.concatenate([ops1, ops2])
    in_a, in_b = np.concatenate([in_a1, a2]).astype(np.uint32), np.concatenate([in_b1, b2]).astype(np.uint32)
    out_wires = np.concatenate([(len(inputs) + np.arange(len(ops)))[::-1], [2]]).astype(np.uint32)

    lv1 = oracle.gate_batch(p, ops1, inputs[in_a1], inputs[in_b1], env.keys, threads=8)
    x2a, x2b = lv1[a2 - len(inputs)], lv1[b2 - len(inputs)]
    lv2 = oracle.gate_batch(p, ops2, x2a, x2b, env.keys, threads=6)
    want = np.concatenate([inputs, lv1, lv2])[out_wires]
    assert np.array_equal(np.array([oracle.gate_combine(p, int(o), inputs[i], inputs[j]) for o, i, j in zip(ops1, in_a1, in_b1)]), target)
    combined2 = np.array([oracle.gate_combine(p, int(o), x, y) for o, x, y in zip(ops2, x2a, x2b)])

    t_in = to_dev(inputs)
    t_out = torch.zeros((len(out_wires), p.n + 1), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()

    def run_dev():
        t_out.zero_()
        torch.cuda.synchronize()
        depth = c.circuit_eval_dev(t_in.data_ptr(), len(inputs), ops, in_a, in_b, out_wires, t_out.data_ptr())
        c.sync()
        return from_dev(t_out), depth
    for form in ("auto", "whole"):
        # level 2's inputs are key-switch outputs: neither hot nor quiet, they may be flagged and may part
        lo = env.parted(oracle, target[hot_at], form) + env.parted(oracle, combined2, form)
        for what, run in (("host", lambda: c.circuit_eval(inputs, ops, in_a, in_b, out_wires)), ("dev", run_dev)):
            (got, depth), delta, kernel = forced(c, run, form)
            assert depth == 2 and kernel == FUSED_KERNEL["128", SMALL_FORM[form]], (what, form, kernel)
            same(got, want, (what, form))
            assert lo <= delta <= len(hot_at) + len(ops2), (what, form, delta)


# ---- per-item test vectors -------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["auto", "whole"])
def test_bootstrap_lut_each_recomputes_with_the_items_table(oracle, env, form):
    """tv_each: B = 7, hot at {0, 3, 6} with the crafted test vector, the others quiet with a random one
    each.  Definition as in test_lut_tree: blind rotation with the item's table, extraction, key switch."""
    c, p = env.c, env.p
    hot_at = [0, 3, 6]
    cts = mg.ct_items(p, 7, hot_at, first=2)
    tvs = mg.words(rng(8000), 7, 2 * p.N)
    tvs[hot_at] = env.tv
    got, delta, kernel = forced(c, lambda: c.bootstrap_lut_each(cts, tvs), form)
    assert "TV" in kernel and kernel.endswith("fused)"), kernel
    acc = env.rotate(oracle, cts, tvs)
    want = np.array([oracle.identity_key_switch(p, oracle.sample_extract_index(a, 0), env.keys.ksk) for a in acc])
    same(got, want, form)
    assert env.parted(oracle, cts[hot_at], form) <= delta <= len(hot_at)


@pytest.mark.parametrize("form", ["auto", "whole"])
def test_lut_apply_multi_recomputes_before_the_fan_out(oracle, env, form):
    """RUN_TRLWE with the fan-out extraction behind it: theta = 1 on every node, the set {interleave of
    two crafted constants, interleave of two random tables}; hot inputs stay hot after round_theta
    (checked here on the host).  Definition as in test_lut_multi, on the oracle's reference mode."""
    c, p = env.c, env.p
    hot_at = [1, 2, 6]
    pool = mg.ct_items(p, 7, hot_at, first=4)
    crafted = tfhe_amd.lut_interleave(c.params, np.stack([env.tv, env.tv]))
    assert np.array_equal(crafted, env.tv)
    tables = np.stack([crafted, tfhe_amd.lut_interleave(c.params, mg.words(rng(8100), 2, 2 * p.N))])
    rounded = tfhe_amd.lut_round_tlwe(c.params, 1, pool)
    assert [mg.is_hot(p, x) for x in rounded] == [i in hot_at for i in range(7)] and all(mg.is_quiet(p, rounded[i]) for i in (0, 3, 4, 5))
    nodes = [(0 if i in hot_at else 1, [(i, 1)], 0) for i in range(7)]
    theta = np.ones(7, np.uint32)
    ls = tfhe_amd.LutSet(c, tables)
    try:
        got, delta, kernel = forced(c, lambda: c.lut_apply_multi(ls, pool, nodes, theta), form)
        kernels = c.last_kernels()
    finally:
        ls.close()
    assert kernel.startswith(FUSED_KERNEL_TV[SMALL_FORM[form]]) and kernel.endswith("fused)"), kernel
    assert "k_lut_fanout_extract" in kernels, kernels
    ref = oracle_composition(oracle, env.k, pool, nodes, theta, tables, range(7))
    same(got, np.concatenate([ref[i] for i in range(7)]), form)
    assert env.parted(oracle, rounded[hot_at], form) <= delta <= len(hot_at)


# ---- several devices -------------------------------------------------------------------------------
def test_two_shards_keep_flags_and_counters_apart(oracle, env):
    """Context.multi over [0, 0] with the crafted key: gate_batch with B = 9 and a hot item in each
    shard.  One device's words, and near_tie_items() is the sum over both shards."""
    p = env.p
    ops = np.array([mg.GATE_OPS[(3 * i) % 11] for i in range(9)], np.uint8)
    hot_at = [1, 7]
    A, Bv = mg.gate_items(oracle, p, ops, hot_at, 8200)
    single, d1, _ = forced(env.c, lambda: env.c.gate_batch(ops, A, Bv))
    same(single, oracle.gate_batch(p, ops, A, Bv, env.keys, threads=8), "one device")
    multi = tfhe_amd.Context.multi("128", devices=[0, 0])
    try:
        multi.load_cloud_key(env.off, env.tv, env.bk, env.keys.ksk)
        assert multi.num_devices == 2 and multi.near_tie_items() == 0
        ran = multi.device_bootstraps()
        got, d2, kernel = forced(multi, lambda: multi.gate_batch(ops, A, Bv))
        ran = multi.device_bootstraps() - ran
        assert kernel == FUSED_KERNEL["128", "wide"]
        assert ran.min() >= 4 and ran.sum() == 9  # item 1 on the first shard, item 7 on the second
        same(got, single, "two shards")
        assert d2 == d1 and multi.near_tie_items() == d2
        assert env.parted(oracle, mg.ct_items(p, 9, hot_at)[hot_at], "auto") <= d2 <= len(hot_at)
        quiet = mg.gate_items(oracle, p, ops, [], 8200)
        _, d3, _ = forced(multi, lambda: multi.gate_batch(ops, *quiet))
        assert d3 == 0
    finally:
        multi.close()
