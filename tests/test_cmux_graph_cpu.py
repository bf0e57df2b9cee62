"""CPU tests of the CMUX graphs' host-only half: tfhe_cmux_graph_plan on random DAGs (levels against a Python
longest-path restatement, the slot assignment replayed level by level), its refusals, and evaluate_plain of
every builder (less_than, equals_const, dfa, popcount) against the plain Python function on all inputs."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import CmuxGraph

u32p = C.POINTER(C.c_uint32)
INV = tfhe_amd.ERR_INVALID
N = 1024


def random_graph(seed):
    """V <= 40 nodes over 1..4 leaves and k <= 6 variables; children drawn from all earlier values with a bias to
    recent ones (deep graphs) or uniformly (wide ones); 0..4 roots, leaves among them."""
    g = np.random.default_rng(seed)
    nL, V, k = int(g.integers(1, 5)), int(g.integers(0, 41)), int(g.integers(1, 7))
    gr = CmuxGraph(k, nL)
    recent = seed % 2 == 0
    for v in range(V):
        ids = nL + v
        pick = (lambda: int(ids - 1 - min(g.geometric(0.4) - 1, ids - 1))) if recent else (lambda: int(g.integers(0, ids)))
        gr.node(int(g.integers(0, k)), pick(), pick(), int(g.integers(0, 2 * N + 1)), int(g.integers(0, 2 * N + 1)))
    gr.root(*(int(r) for r in g.integers(0, nL + V, int(g.integers(0, 5)))))
    return gr


def longest_path_levels(gr):
    level = []
    for v in range(gr.n_nodes):
        kids = [level[c - gr.n_leaves] for c in (gr.lo[v], gr.hi[v]) if c >= gr.n_leaves]
        level.append(1 + max(kids, default=0))
    return level


def replay(gr, level, slot, depth, n_slots):
    """The level-by-level schedule with the slots as dictionary keys: a level first reads (every child of its
    nodes must still be in its slot), then writes; no slot is written in a level that reads it."""
    held = {}  # slot -> node
    readers_left = [0] * gr.n_nodes
    for v in range(gr.n_nodes):
        for c in {gr.lo[v], gr.hi[v]}:
            if c >= gr.n_leaves:
                readers_left[c - gr.n_leaves] += 1
    root_nodes = {r - gr.n_leaves for r in gr.roots if r >= gr.n_leaves}
    for l in range(1, depth + 1):
        nodes = [v for v in range(gr.n_nodes) if level[v] == l]
        assert nodes, f"level {l} is empty"
        read = set()
        for v in nodes:
            for c in {gr.lo[v], gr.hi[v]}:
                if c >= gr.n_leaves:
                    assert held.get(slot[c - gr.n_leaves]) == c - gr.n_leaves, "a child was overwritten before its last reader"
                    read.add(slot[c - gr.n_leaves])
                    readers_left[c - gr.n_leaves] -= 1
        written = [slot[v] for v in nodes]
        assert len(set(written)) == len(written), "two nodes of a level share a slot"
        assert not read & set(written), "a slot is written in the level that reads it"
        for v in nodes:
            assert slot[v] < n_slots
            old = held.get(slot[v])
            if old is not None:
                assert readers_left[old] == 0 and old not in root_nodes
            held[slot[v]] = v
    for r in root_nodes:
        assert held.get(slot[r]) == r, "a root did not survive"


@pytest.mark.parametrize("block", range(4))
def test_plan_on_random_graphs(block):
    """200 graphs, seeds 0 .. 199."""
    for seed in range(50 * block, 50 * block + 50):
        gr = random_graph(seed)
        level, slot, depth, n_slots = gr.plan()
        assert list(level) == longest_path_levels(gr), seed
        assert depth == max(level, default=0)
        assert n_slots == (max(slot) + 1 if gr.n_nodes else 0)
        replay(gr, [int(x) for x in level], [int(x) for x in slot], depth, n_slots)


def test_layered_graphs_take_slots_by_width_not_size():
    for nbits in (8, 32):
        gr = CmuxGraph.less_than(nbits)
        level, slot, depth, n_slots = gr.plan()
        assert gr.n_nodes == 3 * nbits - 1 and depth == 2 * nbits  # the lowest pair's a_i = 1 side is the leaf "false"
        assert n_slots <= 8
        replay(gr, list(level), list(slot), depth, n_slots)
    dfa = CmuxGraph.dfa(4, [[(s + a) % 4 for a in (0, 1)] for s in range(4)], {3}, 16, 1)
    level, slot, depth, n_slots = dfa.plan()
    assert depth == 16 and n_slots <= 8
    one = CmuxGraph(1, 2)
    one.node(0, 0, 1)
    assert [list(x) if hasattr(x, "__len__") else x for x in one.root(2).plan()] == [[1], [0], 1, 1]


def plan_status(nL, k, nodes, roots, level=True, slot=True, arrays=None):
    lib = tfhe_amd.load_library()
    cols = [np.array([n[i] for n in nodes], np.uint32) for i in range(5)]
    ptr = [c.ctypes.data_as(u32p) for c in cols]
    if arrays is not None:
        ptr = [p if keep else None for p, keep in zip(ptr, arrays)]
    r = np.array(roots, np.uint32)
    lv, sl = np.zeros(len(nodes) + 1, np.uint32), np.zeros(len(nodes) + 1, np.uint32)
    return lib.tfhe_cmux_graph_plan(nL, len(nodes), k, *ptr, len(roots), r.ctypes.data_as(u32p) if roots is not None and len(roots) else None,
                                    N, lv.ctypes.data_as(u32p) if level else None, sl.ctypes.data_as(u32p) if slot else None,
                                    None, None)


def test_plan_refusals():
    ok = [(0, 0, 1, 0, 0), (1, 2, 0, 5, 2 * N)]
    assert plan_status(2, 2, ok, [3, 0]) == 0
    assert plan_status(0, 2, ok, [0]) == INV  # no leaves
    assert plan_status(2, 2, [(0, 2, 1, 0, 0)], [2]) == INV  # lo is the node itself
    assert plan_status(2, 2, [(0, 0, 3, 0, 0)], [2]) == INV  # hi is a later value
    assert plan_status(2, 2, [ok[0], (0, 3, 0, 0, 0)], [2]) == INV  # child id == own id
    assert plan_status(2, 2, [(2, 0, 1, 0, 0)], [2]) == INV  # var >= k
    assert plan_status(2, 0, [(0, 0, 1, 0, 0)], [2]) == INV  # k = 0 with a node
    assert plan_status(2, 2, [(0, 0, 1, 2 * N + 1, 0)], [2]) == INV
    assert plan_status(2, 2, [(0, 0, 1, 0, 2 * N + 1)], [2]) == INV
    assert plan_status(2, 2, ok, [4]) == INV  # root >= nL + V
    for i in range(5):
        assert plan_status(2, 2, ok, [3], arrays=[j != i for j in range(5)]) == INV  # a null node array
    assert plan_status(2, 2, ok, [3], level=False) == INV
    assert plan_status(2, 2, ok, [3], slot=False) == INV
    lib = tfhe_amd.load_library()
    x = np.zeros(4, np.uint32).ctypes.data_as(u32p)
    assert lib.tfhe_cmux_graph_plan(2, 0, 0, None, None, None, None, None, 2, None, N, None, None, None, None) == INV  # null roots
    d, s = C.c_uint32(9), C.c_uint32(9)
    assert lib.tfhe_cmux_graph_plan(2, 0, 0, None, None, None, None, None, 1, x, N, None, None, C.byref(d), C.byref(s)) == 0
    assert (d.value, s.value) == (0, 0)  # V = 0: the roots are leaves
    bad = CmuxGraph(1, 1)
    bad.node(1, 0, 0)
    with pytest.raises(tfhe_amd.TfheError) as e:
        bad.plan()
    assert e.value.status == INV


def test_entries_refuse_a_null_context_and_are_exported():
    lib = tfhe_amd.load_library()
    x = np.zeros(2048, np.uint32).ctypes.data_as(u32p)
    assert lib.tfhe_gpu_cmux_graph_batch(None, None, x, 1, x, 1, 0, None, None, None, None, None, 1, x, 0, x, 1) == INV
    assert lib.tfhe_gpu_cmux_graph_dev(None, None, x, 1, None, 1, 0, None, None, None, None, None, 1, x, 0, None, 1) == INV
    for name in ("tfhe_cmux_graph_plan", "tfhe_gpu_cmux_graph_batch", "tfhe_gpu_cmux_graph_dev"):
        assert name in tfhe_amd.EXPORTED_SYMBOLS
    assert tfhe_amd.OPTIONS["graph_chunk_queries"] == 21 and tfhe_amd.OPTION_DEFAULTS["graph_chunk_queries"] == 0


# ---- the builders, on plain bits -----------------------------------------------------------------------------
def test_less_than_all_inputs():
    nbits = 4
    gr = CmuxGraph.less_than(nbits)
    for a, b in itertools.product(range(1 << nbits), repeat=2):
        bits = np.zeros(2 * nbits, int)
        for i in range(nbits):  # most significant first, interleaved
            bits[2 * i], bits[2 * i + 1] = (a >> (nbits - 1 - i)) & 1, (b >> (nbits - 1 - i)) & 1
        assert gr.evaluate_plain(bits) == [(int(a < b), 0)], (a, b)


@pytest.mark.parametrize("c", [0, 1, 37, 42, 63])
def test_equals_const_all_inputs(c):
    gr = CmuxGraph.equals_const(6, c)
    assert gr.n_nodes == 6
    for x in range(64):
        assert gr.evaluate_plain([(x >> j) & 1 for j in range(6)]) == [(int(x == c), 0)], x


def test_popcount_all_inputs():
    gr = CmuxGraph.popcount(6)
    assert gr.n_nodes == 6 and gr.n_leaves == 1
    for x in range(64):
        pop = bin(x).count("1")
        assert gr.evaluate_plain([(x >> j) & 1 for j in range(6)]) == [(0, (2 * N - pop) % (2 * N))], x
    tv = CmuxGraph.testvec_leaf([c >= 4 for c in range(7)])
    assert tv.shape == (1, 2 * N) and not tv[0, :N].any()
    assert list(tv[0, N:N + 8]) == [0xE0000000] * 4 + [0x20000000] * 3 + [0xE0000000]


def contains_101(bits):
    return "101" in "".join(str(int(b)) for b in bits)


# 3 states + the accepting sink: the number of characters of "101" matched so far
DELTA_101 = [[0, 1], [2, 1], [0, 3], [3, 3]]


def test_dfa_all_strings():
    gr = CmuxGraph.dfa(4, DELTA_101, {3}, 6, 1)
    for x in range(64):
        bits = [(x >> (5 - p)) & 1 for p in range(6)]
        assert gr.evaluate_plain(bits) == [(int(contains_101(bits)), 0)], bits
    # a 3-state automaton over 2-bit symbols: the sum of the symbols mod 3 is 0
    mod3 = CmuxGraph.dfa(3, [[(s + a) % 3 for a in range(4)] for s in range(3)], {0}, 3, 2)
    for x in range(64):
        sym = [(x >> (2 * p)) & 3 for p in range(3)]
        bits = [(x >> j) & 1 for j in range(6)]  # variable 2p + b is bit b of symbol p
        assert mod3.evaluate_plain(bits) == [(int(sum(sym) % 3 == 0), 0)], sym


def test_bool_leaves():
    lv = CmuxGraph.bool_leaves()
    assert lv.shape == (2, 2 * N) and not lv[:, :N].any()
    assert (lv[0, N:] == 0xE0000000).all() and (lv[1, N:] == 0x20000000).all()
