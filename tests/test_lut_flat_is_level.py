"""A flat LUT batch is one level of a circuit: tfhe_lut.cpp runs both through the same level step, the flat entry with
the caller's pool for the wire table and the caller's out for the level's run of slots.  Every flat entry, host and
_dev form, is word-equal (np.array_equal) to lut_circuit_eval_ext on the depth-1 circuit whose inputs are the pool
and whose outputs are all node wires in order.  The smallest shapes that take every branch of the step: a pool of 4,
B = 3 nodes with 0, 1 and 2 terms, m = 4, on the synthetic n = 8 sets of test_lut_ext.py (L = 1 and L = 2).
bootstrap_lut_each[_ext], which has no nodes, equals lut_select[_ext] on nodes whose entries are the constants packed
into its test vectors."""
import numpy as np
import pytest

import tfhe_amd
from test_lut_circuit import combine
from test_lut_circuit_ext import entry_cts, select_tvs, small_env
from test_lut_ext import words
from test_lut_select import const, enc
from test_lut_tree import from_dev, to_dev

pytestmark = pytest.mark.gpu

N, M, P = 1024, 4, 4
# (terms, const) of the three nodes: none, one and two terms
XS = [([], enc(M, 3)), ([(1, 1)], 0), ([(0, 2), (3, -1)], enc(M, 1))]
LUT = [1, 0, 1]  # also extended tables at eta = 2 of a set of 8 (4 * 1 + 4 <= 8)
# the select nodes' entries: one constant among pool ciphertexts, constants only, pool ciphertexts only
ENTRIES = [[0, const(M, 2), 2, 3], [const(M, i) for i in (3, 0, 2, 1)], [3, 1, 1, 0]]
SETS = ["l2small", "uint4"]

# case -> (the host entry's name, what goes in front of the pool after the set or key, theta)
TABLE_CASES = {"apply": ("lut_apply", (), None), "multi": ("lut_apply_multi", (), (0, 1, 0)),
               "ext1": ("lut_apply_ext", (1,), None), "ext2": ("lut_apply_ext", (2,), None)}
SELECT_CASES = {"select": ("lut_select", ()), "select_ext1": ("lut_select_ext", (1,)),
                "select_ext2": ("lut_select_ext", (2,))}


def flat_both(c, entry, head, pool, nodes, n_out, tail=()):
    """The flat entry on host buffers, and its _dev form on torch buffers filled with -1."""
    import torch
    host = getattr(c, entry)(*head, pool, nodes, *tail)
    t_pool = to_dev(pool)
    t_out = torch.full((n_out, c.n1), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()  # the fill runs on torch's stream, the batch on the context's
    getattr(c, entry + "_dev")(*head, t_pool.data_ptr(), len(pool), nodes, *tail, t_out.data_ptr())
    c.sync()
    return host, from_dev(t_out)


def level(c, ls, key, circ, pool):
    """lut_circuit_eval_ext on circ, every node wire an output in order."""
    ow = np.arange(circ.n_inputs, circ.n_wires, dtype=np.uint32)
    got, depth = c.lut_circuit_eval_ext(ls, key, circ.m, pool, circ.packed(), circ.theta, circ.select_arrays(), circ.eta,
                                        ow)
    assert depth == 1
    return got


def pool_circuit():
    circ = tfhe_amd.LutCircuit()
    for _ in range(P):
        circ.input()
    return circ


@pytest.mark.parametrize("case", list(TABLE_CASES))
@pytest.mark.parametrize("name", SETS)
def test_table_batches_are_one_level(oracle, name, case):
    """lut_apply, lut_apply_multi with theta = (0, 1, 0) (the level's multi-output launch, four outputs) and
    lut_apply_ext with eta 1 and 2 (the level's extended group alone)."""
    c, p, ck, sk, key, rows, basebit, t = small_env(oracle, name)
    entry, eta, theta = TABLE_CASES[case]
    pool = words(15000, P, p.n + 1)
    nodes = [(lut, terms, k) for lut, (terms, k) in zip(LUT, XS)]
    circ = pool_circuit()
    for i, (lut, terms, k) in enumerate(nodes):
        circ.node(lut, terms, k, outputs=1 << theta[i] if theta else 1, eta=eta[0] if eta else 0)
    ls = tfhe_amd.LutSet(c, words(15001, 8, 2 * N))
    try:
        want = level(c, ls, None, circ, pool)
        kernels = c.last_kernels()
        host, dev = flat_both(c, entry, (ls, *eta), pool, nodes, len(want), (theta,) if theta else ())
        assert c.last_kernels() == kernels
    finally:
        ls.close()
    assert len(want) == (4 if theta else 3)
    assert np.array_equal(host, want), np.flatnonzero((host != want).any(axis=1)).tolist()
    assert np.array_equal(dev, want), np.flatnonzero((dev != want).any(axis=1)).tolist()


@pytest.mark.parametrize("case", list(SELECT_CASES))
@pytest.mark.parametrize("name", SETS)
def test_select_batches_are_one_level(oracle, name, case):
    """lut_select and lut_select_ext with eta 1 and 2: the flat entries have no set, the circuit has one it never
    reads."""
    c, p, ck, sk, key, rows, basebit, t = small_env(oracle, name)
    entry, eta = SELECT_CASES[case]
    pool = words(15100, P, p.n + 1)
    nodes = [(terms, ents, k) for (terms, k), ents in zip(XS, ENTRIES)]
    circ = pool_circuit()
    for terms, ents, k in nodes:
        circ.select(terms, ents, k, eta=eta[0] if eta else 0)
    ls = tfhe_amd.LutSet(c, words(15101, 1, 2 * N))
    try:
        want = level(c, ls, key, circ, pool)
        kernels = c.last_kernels()
    finally:
        ls.close()
    host, dev = flat_both(c, entry, (key, M, *eta), pool, nodes, 3)
    assert c.last_kernels() == kernels
    assert np.array_equal(host, want), np.flatnonzero((host != want).any(axis=1)).tolist()
    assert np.array_equal(dev, want), np.flatnonzero((dev != want).any(axis=1)).tolist()


@pytest.mark.parametrize("eta", [0, 1, 2])
@pytest.mark.parametrize("name", SETS)
def test_each_is_select_on_constant_entries(oracle, name, eta):
    """Three nodes of four trivial constants each: the host pack and spread of the entries give the test vectors of
    bootstrap_lut_each (eta 0) and bootstrap_lut_each_ext, the host combination their inputs."""
    import torch
    c, p, ck, sk, key, rows, basebit, t = small_env(oracle, name)
    pool = words(15200, P, p.n + 1)
    g = np.random.default_rng(15201)
    nodes = [(terms, [const(M, int(v)) for v in g.integers(0, M, M)], k) for terms, k in XS]
    want = c.lut_select_ext(key, M, eta, pool, nodes) if eta else c.lut_select(key, M, pool, nodes)
    kernels = c.last_kernels()
    x = combine(pool, [(0, terms, k) for terms, _, k in nodes])
    tvs = select_tvs(c, rows, basebit, t, M, [entry_cts(c, pool, e) for _, e, _ in nodes])
    got = c.bootstrap_lut_each_ext(eta, x, tvs) if eta else c.bootstrap_lut_each(x, tvs)
    assert c.last_kernels() == kernels
    t_x, t_tv = to_dev(x), to_dev(tvs)
    t_out = torch.full((3, c.n1), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    if eta:
        c.bootstrap_lut_each_ext_dev(eta, t_x.data_ptr(), t_tv.data_ptr(), t_out.data_ptr(), 3)
    else:
        c.bootstrap_lut_each_dev(t_x.data_ptr(), t_tv.data_ptr(), t_out.data_ptr(), 3)
    c.sync()
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1)).tolist()
    assert np.array_equal(from_dev(t_out), want)
