"""GPU tests of the CMUX graphs (k_cmux_rot, include/tfhe_gpu.h "CMUX graphs"): word for word (np.array_equal)
against the definition, Context.cmux node by node on inputs rotated on the host by oracle.poly_mul_with_xk; against
table_lookup with the tree written as a graph; chunked, on device buffers and extracted; then what the builders
compute on real ciphertexts (less_than, popcount, a DFA) and the noise of a 64-level chain.  Keys: the oracle's
seeded ones on the shared contexts (ctx_for)."""
import ctypes as C

import numpy as np
import pytest

import tfhe_amd
from conftest import rng
from test_cmux_graph_cpu import DELTA_101, contains_101
from test_lut_circuit import ctx_for
from tfhe_amd import CmuxGraph

pytestmark = pytest.mark.gpu
u32p = C.POINTER(C.c_uint32)
INV = tfhe_amd.ERR_INVALID
N = 1024
ROTS = [0, 1, 63, 64, 1023, 1024, 1025, 2047, 2048]
# 7 nodes hold 7 rotations per side, so the 9 values take two assignments: between them every value stands on the
# lo side and on the hi side at least once.
RLO = {"a": [ROTS[i] for i in (0, 1, 2, 3, 4, 5, 6)], "b": [ROTS[i] for i in (7, 8, 0, 3, 5, 1, 6)]}
RHI = {"a": [ROTS[i] for i in (2, 3, 4, 5, 6, 7, 8)], "b": [ROTS[i] for i in (0, 1, 8, 4, 7, 2, 5)]}
assert set(RLO["a"] + RLO["b"]) == set(ROTS) and set(RHI["a"] + RHI["b"]) == set(ROTS)


def u32rand(g, *shape):
    return g.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def from_dev(t):
    return t.cpu().numpy().view(np.uint32)


def status(call):
    with pytest.raises(tfhe_amd.TfheError) as e:
        call()
    return e.value.status


_ENV, _CASE = {}, {}


class Env:
    """The shared context of a parameter set with the oracle's cloud key, and three selectors (encryptions of 0, 1
    and 1 under the oracle's level-1 key, seeds 900..902) from the oracle, resident as a TrgswSet."""

    def __init__(self, oracle, pname):
        self.ctx, self.k = ctx_for(oracle, pname)
        self.p, self.k1 = self.k.p, self.k.k1
        self.off = oracle.decomposition_offset(self.p)
        self.sel_bits = [0, 1, 1]
        self.trgsw = np.array([oracle.trgsw_encrypt_torus_fft(self.p, mu, self.p.alpha_bsk, self.k1, 900 + s)
                               for s, mu in enumerate(self.sel_bits)])
        self.set = tfhe_amd.TrgswSet(self.ctx, self.trgsw)


def env(oracle, pname):
    if pname not in _ENV:
        _ENV[pname] = Env(oracle, pname)
    return _ENV[pname]


def seven_nodes(which):
    """3 leaves (ids 0..2), 7 nodes (ids 3..9) over 3 variables: node 3 stands on two leaves; it is shared by nodes
    4, 5 and 7; node 5 has lo == hi; node 7's child 3 is three levels down and node 9's child 4 four; the roots
    are a leaf, an inner node and the last node."""
    gr = CmuxGraph(3, 3)
    shape = [(0, 0, 1), (1, 3, 2), (2, 3, 3), (0, 4, 5), (1, 6, 3), (2, 1, 7), (0, 8, 4)]
    for (var, lo, hi), rlo, rhi in zip(shape, RLO[which], RHI[which]):
        gr.node(var, lo, hi, rlo, rhi)
    return gr.root(2, 6, 9)


ADDR5 = np.array([[0, 1, 2], [1, 0, 0], [2, 2, 1], [0, 0, 0], [1, 2, 0]], np.uint32)  # Q = 5: a ragged last workgroup


def mulxk(oracle, x, r):
    return np.concatenate([oracle.poly_mul_with_xk(x[:N], r), oracle.poly_mul_with_xk(x[N:], r)])


def by_definition(oracle, e, gr, leaves, addr):
    """value[nL + v] for every query, node by node: Context.cmux on the host-rotated children.  -> (Q, nL + V, 2N)."""
    Q = addr.shape[0]
    val = [np.broadcast_to(leaf, (Q, 2 * N)) for leaf in leaves]
    for v in range(gr.n_nodes):
        in0 = np.array([mulxk(oracle, val[gr.lo[v]][q], gr.rlo[v]) for q in range(Q)])
        in1 = np.array([mulxk(oracle, val[gr.hi[v]][q], gr.rhi[v]) for q in range(Q)])
        val.append(e.ctx.cmux(e.set, addr[:, gr.var[v]], in0, in1))
    return np.stack(val, axis=1)


def case(oracle, pname, which="a"):
    """The seven-node graph on random leaves for Q = 5, with its definition's words, computed once."""
    if (pname, which) not in _CASE:
        e = env(oracle, pname)
        gr = seven_nodes(which)
        leaves = u32rand(rng(520 + e.p.L), 3, 2 * N)
        _CASE[pname, which] = (gr, leaves, by_definition(oracle, e, gr, leaves, ADDR5))
    return _CASE[pname, which]


# ---- 1. word for word against the definition, L = 3, 2, 1 ---------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("pname", ["128", "uint1", "uint4"])
def test_graph_matches_definition(oracle, pname, which):
    e = env(oracle, pname)
    gr, leaves, val = case(oracle, pname, which)
    level, slot, depth, n_slots = gr.plan()
    assert list(level) == [1, 2, 2, 3, 4, 5, 6] and depth == 6
    got = e.ctx.cmux_graph(e.set, ADDR5, gr, leaves)
    assert e.ctx.last_kernels() == f"k_cmux_rot<{e.p.L}>"
    assert got.shape == (5, 3, 2 * N)
    assert np.array_equal(got, val[:, gr.roots])
    assert np.array_equal(got[:, 0], np.broadcast_to(leaves[2], (5, 2 * N)))  # the leaf root
    # two nodes against the oracle itself: node 3 (on two leaves) and, through the definition's children, node 9
    for q, v in ((0, 0), (4, 6)):
        in0, in1 = mulxk(oracle, val[q, gr.lo[v]], gr.rlo[v]), mulxk(oracle, val[q, gr.hi[v]], gr.rhi[v])
        assert np.array_equal(val[q, 3 + v], oracle.cmux(e.p, in0, in1, e.trgsw[ADDR5[q, gr.var[v]]], e.off)), v
    assert np.array_equal(got[4, 2], val[4, 9])


# ---- 2. no rotation: the table lookup's tree as a graph -----------------------------------------------------------
def tree_graph(k):
    gr = CmuxGraph(k, 1 << k)
    cur = list(range(1 << k))
    for j in range(k):
        cur = [gr.node(j, cur[2 * i], cur[2 * i + 1]) for i in range(len(cur) // 2)]
    return gr.root(cur[0])


def test_unrotated_graph_is_the_table_lookup(oracle):
    e = env(oracle, "128")
    table = u32rand(rng(530), 8, 2 * N)
    want = e.ctx.table_lookup(e.set, ADDR5, table)
    got = e.ctx.cmux_graph(e.set, ADDR5, tree_graph(3), table)
    assert np.array_equal(got[:, 0], want)
    assert len({w.tobytes() for w in want}) == 5


# ---- 3. chunks, 4. device buffers, 5. extraction ----------------------------------------------------------------
def test_chunks_change_no_word(oracle):
    e = env(oracle, "128")
    gr, leaves, val = case(oracle, "128")
    assert e.ctx.get_option("graph_chunk_queries") == 0
    with e.ctx.options(graph_chunk_queries=2):  # 2 + 2 + 1 queries
        assert e.ctx.get_option("graph_chunk_queries") == 2
        got = e.ctx.cmux_graph(e.set, ADDR5, gr, leaves)
        ext = e.ctx.cmux_graph(e.set, ADDR5, gr, leaves, extract=1)
    assert e.ctx.get_option("graph_chunk_queries") == 0
    assert np.array_equal(got, val[:, gr.roots])
    assert np.array_equal(ext.reshape(15, N + 1), e.ctx.sample_extract(got.reshape(15, 2 * N), [0])[:, 0])
    assert status(lambda: e.ctx.set_option("graph_chunk_queries", -1)) == INV


def test_dev_matches_host(oracle):
    import torch
    e = env(oracle, "128")
    gr, leaves, val = case(oracle, "128")
    lv = to_dev(leaves)
    out = torch.zeros((5, 3, 2 * N), dtype=torch.int32, device="cuda:0")
    e.ctx.cmux_graph_dev(e.set, ADDR5, gr, lv.data_ptr(), out.data_ptr())
    e.ctx.sync()
    assert np.array_equal(from_dev(out), val[:, gr.roots])
    low = torch.zeros((5, 3, e.ctx.n1), dtype=torch.int32, device="cuda:0")
    e.ctx.cmux_graph_dev(e.set, ADDR5, gr, lv.data_ptr(), low.data_ptr(), extract=2)
    e.ctx.sync()
    assert np.array_equal(from_dev(low), e.ctx.cmux_graph(e.set, ADDR5, gr, leaves, extract=2))
    assert np.array_equal(from_dev(lv), leaves)
    # out over the leaves is refused
    assert status(lambda: e.ctx.cmux_graph_dev(e.set, ADDR5, gr, lv.data_ptr(), lv.data_ptr() + 8192)) == INV


@pytest.mark.parametrize("pname", ["128", "uint4"])
def test_extract_is_sample_extract(oracle, pname):
    e = env(oracle, pname)
    gr, leaves, val = case(oracle, pname)
    roots = np.ascontiguousarray(val[:, gr.roots]).reshape(15, 2 * N)
    for extract, ks in ((1, False), (2, True)):
        got = e.ctx.cmux_graph(e.set, ADDR5, gr, leaves, extract=extract)
        want = e.ctx.sample_extract(roots, [0], key_switch=ks)
        assert got.shape == (5, 3, want.shape[2])
        assert np.array_equal(got.reshape(15, -1), want[:, 0]), extract
    assert e.ctx.last_kernels().startswith(f"k_cmux_rot<{e.p.L}> + k_")  # then the key switch's form


# ---- 7. what the builders compute, on ciphertexts ------------------------------------------------------------------
PAIRS = [(0, 0), (0xFFFF, 0xFFFF), (0x1234, 0x1235), (0x1235, 0x1234), (0x8000, 0x0000), (0x7FFF, 0xFFFF),
         (0xBEEF, 0xBEEF), (0x00FF, 0x0100)]  # equal; the lowest bit apart, both ways; the highest bit apart, both ways


class Bits:
    """256 selectors encrypted on the device under the oracle's level-1 key: selector 32 q + j encrypts variable j of
    pair q of less_than(16).  pick(bits) names, for any other list of plain bits, selectors that encrypt them,
    walking through the set so that a query's selectors are distinct while there are enough."""

    def __init__(self, oracle):
        e = env(oracle, "128")
        self.plain = np.zeros((8, 32), np.uint32)
        for q, (a, b) in enumerate(PAIRS):
            for i in range(16):
                self.plain[q, 2 * i], self.plain[q, 2 * i + 1] = (a >> (15 - i)) & 1, (b >> (15 - i)) & 1
        self.set = tfhe_amd.TrgswSet(e.ctx, e.ctx.trgsw_encrypt(e.k1, self.plain.reshape(-1), seed0=7000))
        flat = self.plain.reshape(-1)
        self.of = [np.flatnonzero(flat == 0), np.flatnonzero(flat == 1)]
        self.at = [0, 0]

    def pick(self, bits):
        out = []
        for b in bits:
            out.append(self.of[int(b)][self.at[int(b)] % len(self.of[int(b)])])
            self.at[int(b)] += 1
        return np.array(out, np.uint32)


def bits_env(oracle):
    if "bits" not in _ENV:
        _ENV["bits"] = Bits(oracle)
    return _ENV["bits"]


def decrypt(e, cts):
    sk = tfhe_amd.SecretKey(e.ctx.params, e.k.k0, e.k.k1)
    return sk.decrypt_bool(cts.reshape(-1, e.ctx.n1))


def test_less_than_decrypts(oracle):
    e, b = env(oracle, "128"), bits_env(oracle)
    gr = CmuxGraph.less_than(16)
    addr = np.arange(256, dtype=np.uint32).reshape(8, 32)
    got = e.ctx.cmux_graph(b.set, addr, gr, CmuxGraph.bool_leaves(), extract=2)
    assert list(decrypt(e, got)) == [x < y for x, y in PAIRS]
    assert [gr.evaluate_plain(row)[0][0] for row in b.plain] == [int(x < y) for x, y in PAIRS]


def test_popcount_threshold_decrypts(oracle):
    e, b = env(oracle, "128"), bits_env(oracle)
    gr = CmuxGraph.popcount(10)
    xs = [0, 1023, 0b0000011111, 0b1111100000, 0b0101010101, 0b0000001111, 0b1110111011, 0b1000000000]
    plain = [[(x >> j) & 1 for j in range(10)] for x in xs]
    addr = np.array([b.pick(row) for row in plain])
    tv = CmuxGraph.testvec_leaf([c >= 5 for c in range(11)])  # at least 5 of the 10 bits set
    got = e.ctx.cmux_graph(b.set, addr, gr, tv, extract=2)
    assert list(decrypt(e, got)) == [bin(x).count("1") >= 5 for x in xs]
    assert [bin(x).count("1") for x in xs] == [0, 10, 5, 5, 5, 4, 8, 1]


def test_dfa_decrypts(oracle):
    e, b = env(oracle, "128"), bits_env(oracle)
    gr = CmuxGraph.dfa(4, DELTA_101, {3}, 24, 1)
    g = rng(77)
    strings = [[0] * 24, [1] * 24, [1, 0] * 12, [1, 1, 0, 0] * 6, [0] * 21 + [1, 0, 1], [1, 0, 0, 1] * 6,
               list(g.integers(0, 2, 24)), [1, 0, 1] + [0] * 21]
    addr = np.array([b.pick(s) for s in strings])
    got = e.ctx.cmux_graph(b.set, addr, gr, CmuxGraph.bool_leaves(), extract=2)
    want = [contains_101(s) for s in strings]
    assert list(decrypt(e, got)) == want
    assert want[:6] == [False, False, True, False, True, False] and want[7]


# ---- 8. noise --------------------------------------------------------------------------------------------------------
def phase_error(e, cts, want):
    """b - a * s of every coefficient against the torus word `want`, exactly (in integers), as signed fractions."""
    s = e.k1.astype(np.int64)
    i, j = np.meshgrid(np.arange(N), np.arange(N))  # M[j, i] = s[i - j] (i >= j), -s[N + i - j] below: a @ M = a * s
    M = np.where(i >= j, s[(i - j) % N], -s[(i - j) % N])
    phase = (cts[:, N:].astype(np.int64) - cts[:, :N].astype(np.int64) @ M) & 0xFFFFFFFF
    return (phase.astype(np.uint32) - np.uint32(want)).view(np.int32) / 2.0 ** 32


def test_noise_of_a_64_level_chain(oracle):
    """64 pass-through CMUXes (lo = hi = the previous value) under selectors that encrypt 0 and 1 in turn, over the
    trivial leaf "true", Q = 64 queries with their own selectors.  Measured on gfx950: sigma = max = 0, exactly.
    With both sides the same words the difference the CMUX decomposes is 0, its digits are all zero and the
    external product is exactly zero (test_leveled.py's ragged-tail test uses the same fact), so this chain carries
    no noise at all; test_noise_of_a_64_level_ladder below is the measurement of the noise rule."""
    e, b = env(oracle, "128"), bits_env(oracle)
    gr = CmuxGraph(2, 1)
    cur = 0
    for j in range(64):
        cur = gr.node(j % 2, cur, cur)
    gr.root(cur)
    assert gr.plan()[2] == 64
    addr = np.array([b.pick([0, 1]) for _ in range(64)])
    leaf = CmuxGraph.bool_leaves()[1:]
    got = e.ctx.cmux_graph(b.set, addr, gr, leaf)[:, 0]
    err = phase_error(e, got, 0x20000000)
    sigma, worst = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
    print(f"64-level pass-through chain, 128-bit set, 64 x {N} coefficients: sigma = {sigma:.3e}, max = {worst:.3e}, "
          f"margin = {1 / 8:.3e}")
    assert sigma < 1.0 / 64


def test_noise_of_a_64_level_ladder(oracle):
    """The same depth with work in every CMUX: two rails x, y that both carry "true" in different words (leaf 0 the
    trivial +1/8, leaf 1 an encryption of +1/8 at every coefficient under alpha_lv1), and level j crosses them,
    x' = cmux(x, y, bit j), y' = cmux(y, x, bit j), so every CMUX decomposes a difference with uniformly random
    words and adds a full external product's error; 64 levels, 64 selectors per query (32 of each bit), Q = 64.
    Two parts add up (include/tfhe_gpu.h, the noise rule):
      - the reference's decomposition truncates (its offset, key.zig:121-131, carries no rounding half), so what a
        selector of 1 passes on is short of its input by r in [0, 2^(32 - L bgbit)) on every word, 2^-(L bgbit + 1)
        of the torus on average.  On the phase that is 2^-(L bgbit + 1) * ((1 * s)[i] - 1) at coefficient i, with
        1 * s the negacyclic product of the all-ones polynomial and the key: the same at every such CMUX, so it
        adds up linearly in the number of one-bits on the path (32 here).  Computed below from the key, not
        measured;
      - what is left is random: the gadget rows' noise and the spread of r, growing with the square root of the
        depth.  The chain's bound is asserted on it: sigma < 1/64, an eighth of the +-1/8 margin.
    And every coefficient stays inside the margin: max |error| < 1/8.  Measured on gfx950 at the 128-bit set: total
    rms 1.750e-2 (max 3.07e-2), the truncation term's own rms 1.749e-2 (-3.02e-2 at coefficient 0), residual sigma
    2.18e-4 (the noise rule of include/tfhe_gpu.h).  The total rms alone is above 1/64."""
    e, b = env(oracle, "128"), bits_env(oracle)
    gr = CmuxGraph(64, 2)
    x, y = 0, 1
    for j in range(64):
        x, y = gr.node(j, x, y), gr.node(j, y, x)
    gr.root(x, y)
    level, slot, depth, n_slots = gr.plan()
    assert depth == 64 and n_slots == 4
    addr = np.array([b.pick([j % 2 for j in range(64)]) for _ in range(64)])
    leaves = np.concatenate([CmuxGraph.bool_leaves()[1:], e.ctx.trlwe_encrypt(e.k1, np.full((1, N), 0.125), seed0=7900)])
    got = e.ctx.cmux_graph(b.set, addr, gr, leaves).reshape(128, 2 * N)
    err = phase_error(e, got, 0x20000000)
    s = e.k1.astype(np.int64)
    ones_times_s = np.array([s[:i + 1].sum() - s[i + 1:].sum() for i in range(N)])  # (1 * s)[i], negacyclic
    shift = 32 * 2.0 ** -(e.p.L * e.p.bgbit + 1) * (ones_times_s - 1)
    rest = err - shift[None, :]
    total, worst = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
    sigma = float(np.sqrt(np.mean(rest ** 2)))
    print(f"64-level ladder, 128-bit set, 128 x {N} coefficients, 32 one-bits: total rms = {total:.3e}, max = {worst:.3e}; "
          f"truncation term rms = {np.sqrt(np.mean(shift ** 2)):.3e}, at coefficient 0 = {shift[0]:+.3e}; "
          f"residual sigma = {sigma:.3e}, margin = {1 / 8:.3e}")
    assert sigma < 1.0 / 64
    assert worst < 1.0 / 8


# ---- 9. refusals ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(oracle):
    import torch
    e = env(oracle, "128")
    c = e.ctx
    gr, leaves, val = case(oracle, "128")
    other = tfhe_amd.Context("128", 0)  # no cloud key
    multi = tfhe_amd.Context.multi("128", devices=[0, 0])
    set_other, set_multi = tfhe_amd.TrgswSet(other, e.trgsw), tfhe_amd.TrgswSet(multi, e.trgsw)
    try:
        def run(shape=None, nL=3, k=3, roots=(2, 6, 9), addr=ADDR5, ctx=c, s=e.set, extract=0, lv=leaves):
            g = CmuxGraph(k, nL)
            for n in (shape or [(0, 0, 1, 0, 0)]):
                g.node(*n)
            g.root(*roots)
            return ctx.cmux_graph(s, addr, g, lv, extract=extract)

        one = [(0, 0, 1, 0, 0)]
        assert run(one, roots=(3,)).shape == (5, 1, 2 * N)
        assert status(lambda: run([(0, 3, 1, 0, 0)], roots=(3,))) == INV  # a child id >= own id
        assert status(lambda: run([(0, 0, 4, 0, 0)], roots=(3,))) == INV
        assert status(lambda: run([(3, 0, 1, 0, 0)], roots=(3,))) == INV  # var >= k
        assert status(lambda: run([(0, 0, 1, 2 * N + 1, 0)], roots=(3,))) == INV  # a rotation > 2N
        assert status(lambda: run([(0, 0, 1, 0, 2 * N + 1)], roots=(3,))) == INV
        assert status(lambda: run(one, roots=(4,))) == INV  # a root >= nL + V
        assert status(lambda: run(one, roots=(3,), addr=ADDR5 + 1)) == INV  # addr[] >= the set's size
        assert status(lambda: run(one, roots=(3,), s=set_other)) == INV  # a set of another context
        assert status(lambda: run(one, roots=(3,), ctx=other, s=set_other, extract=2)) == tfhe_amd.ERR_NO_KEY
        assert run(one, roots=(3,), ctx=other, s=set_other, extract=1).shape == (5, 1, N + 1)  # needs no key
        lib, h = c.lib, c.h
        V, var, lo, hi, rlo, rhi, R, roots = gr.pointers()
        ap, lp = ADDR5.ctypes.data_as(u32p), leaves.ctypes.data_as(u32p)
        out = np.zeros((5, 3, 2 * N), np.uint32)
        op = out.ctypes.data_as(u32p)
        call = lib.tfhe_gpu_cmux_graph_batch
        assert call(h, e.set.h, ap, 3, lp, 3, V, var, lo, hi, rlo, rhi, R, roots, 0, op, 5) == 0
        assert np.array_equal(out, val[:, gr.roots])
        assert call(h, e.set.h, ap, 3, lp, 0, V, var, lo, hi, rlo, rhi, R, roots, 0, op, 5) == INV  # nL = 0
        assert call(h, None, ap, 3, lp, 3, V, var, lo, hi, rlo, rhi, R, roots, 0, op, 5) == INV
        assert call(h, e.set.h, None, 3, lp, 3, V, var, lo, hi, rlo, rhi, R, roots, 0, op, 5) == INV
        assert call(h, e.set.h, ap, 3, None, 3, V, var, lo, hi, rlo, rhi, R, roots, 0, op, 5) == INV
        assert call(h, e.set.h, ap, 3, lp, 3, V, None, lo, hi, rlo, rhi, R, roots, 0, op, 5) == INV
        assert call(h, e.set.h, ap, 3, lp, 3, V, var, lo, hi, rlo, None, R, roots, 0, op, 5) == INV
        assert call(h, e.set.h, ap, 3, lp, 3, V, var, lo, hi, rlo, rhi, R, None, 0, op, 5) == INV
        assert call(h, e.set.h, ap, 3, lp, 3, V, var, lo, hi, rlo, rhi, R, roots, 0, None, 5) == INV
        assert call(h, e.set.h, ap, 3, lp, 3, V, var, lo, hi, rlo, rhi, R, roots, 3, op, 5) == INV  # extract
        assert call(h, e.set.h, None, 3, lp, 3, V, var, lo, hi, rlo, rhi, R, roots, 0, None, 0) == 0  # Q = 0
        # V = 0: the roots are leaves
        leaf_only = c.cmux_graph(e.set, ADDR5, CmuxGraph(3, 3).root(1, 0), leaves)
        assert np.array_equal(leaf_only, np.broadcast_to(leaves[[1, 0]], (5, 2, 2 * N)))
        # _dev on a multi-device context
        t = torch.zeros((8, 2 * N), dtype=torch.int32, device="cuda:0")
        assert status(lambda: multi.cmux_graph_dev(set_multi, ADDR5, gr, t.data_ptr(), t[3:].data_ptr())) == INV
        assert multi.cmux_graph(set_multi, ADDR5[:1], gr, leaves).shape == (1, 3, 2 * N)  # the host call runs there
        # and the context still works
        assert np.array_equal(c.cmux_graph(e.set, ADDR5, gr, leaves), val[:, gr.roots])
    finally:
        set_other.close()
        set_multi.close()
        other.close()
        multi.close()
