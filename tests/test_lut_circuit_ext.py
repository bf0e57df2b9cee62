"""Extended nodes of LUT circuits on the device (include/tfhe_gpu.h "Extended nodes"): bootstrap_lut_each_ext,
lut_select_ext and lut_circuit_eval_ext.  Word for word (np.array_equal) against compositions of entries that
existed before them: blind_rotate_ext (the stage entry, with E copies of the item's test vector) and sample_extract
for the per-item bootstrap; pack_tlwe_host and lut_spread_host in front of that for a select node; lut_apply,
lut_apply_multi, lut_apply_ext and the select composition, node by node, for a circuit.  The word-exact tests run on
the synthetic n = 8 sets of test_lut_ext.py (L = 1, 3 and 2) with a packing key of their own; one test reads messages
at the real UINT4 key."""
import numpy as np
import pytest

import tfhe_amd
from conftest import rng
from test_lut_circuit import combine
from test_lut_ext import SMALL, blind_rotate_ext_ref, check_inputs_survive, crafted_inputs, small_ctx, words
from test_lut_select import const, enc, trivial
from test_lut_tree import env, from_dev, status, to_dev

pytestmark = pytest.mark.gpu

INV = tfhe_amd.ERR_INVALID
N = 1024
_PK = {}


def small_env(oracle, name):
    """(context, oracle params, cloud key, secret key, packing key, its host rows and shape) of a synthetic set."""
    c, p, ck = small_ctx(oracle, name)
    if name not in _PK:
        k0, k1 = oracle.secret_key(p, 42)
        sk = tfhe_amd.SecretKey(c.params, k0, k1)
        rows, basebit, t = tfhe_amd.PackingKey.generate_rows(c, sk, 7300)
        _PK[name] = (sk, tfhe_amd.PackingKey(c, rows, basebit, t), rows, basebit, t)
    return (c, p, ck) + _PK[name]


def each_ext_want(c, eta, x, tvs):
    """The definition from the stage entry: per item the blind rotation over E copies of its test vector, then
    sampleExtractIndex(acc_0, 0) and the key switch.  -> (words (B, n+1), accumulators (B, E, 2N))."""
    E = 1 << eta
    acc = np.concatenate([c.blind_rotate_ext(eta, x[i:i + 1], np.tile(tvs[i], (E, 1))) for i in range(len(x))])
    return c.sample_extract(acc[:, 0], [0], key_switch=True).reshape(len(x), c.n1), acc


def select_tvs(c, rows, basebit, t, m, entries):
    """Steps 1 and 2 of a select node on the host: entries (B, m, n+1) in pack order -> (B, 2N) test vectors."""
    w = N // m
    packed = tfhe_amd.pack_tlwe_host(c.params, rows, basebit, t, np.asarray(entries, np.uint32).reshape(-1, m, c.n1),
                                     np.arange(m, dtype=np.uint32) * w)
    return tfhe_amd.lut_spread_host(c.params, packed, w, 2 * N - N // (2 * m))


def entry_cts(c, pool, entries):
    return [trivial(c, e[1]) if isinstance(e, tuple) else pool[e] for e in entries]


# ---- 1. a test vector per item, extended -----------------------------------------------------------
@pytest.mark.parametrize("eta", [1, 2])
@pytest.mark.parametrize("name", ["uint4", "128", "l2small"])
def test_each_ext_is_the_stage_entry_per_item(oracle, name, eta):
    """5 items with random TRLWE test vectors (a != 0): b~ = 2N E, 0, 1 and 2N E - 5, every mask residue at
    q = 2N - 1 and at q = 0 (crafted_inputs).  Host and device buffers; item 2's accumulators also equal the oracle's
    composition of the definition."""
    import torch
    oracle.set_fused(0)
    c, p, ck = small_ctx(oracle, name)
    E = 1 << eta
    x = crafted_inputs(p.n, eta, 14000 + eta)
    tvs = words(14010 + eta, 5, 2 * N)
    want, acc = each_ext_want(c, eta, x, tvs)
    got = c.bootstrap_lut_each_ext(eta, x, tvs)
    assert c.last_kernels().startswith(f"k_blind_rotate_ext<{p.L},{E}> + k_key_switch"), c.last_kernels()
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1)).tolist()
    t_x, t_tv = to_dev(x), to_dev(tvs)
    t_out = torch.full((5, c.n1), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    c.bootstrap_lut_each_ext_dev(eta, t_x.data_ptr(), t_tv.data_ptr(), t_out.data_ptr(), 5)
    c.sync()
    assert np.array_equal(from_dev(t_out), want)
    ref = blind_rotate_ext_ref(oracle, p, ck, x[2], np.tile(tvs[2], (E, 1)), eta)
    assert np.array_equal(acc[2], ref)


def test_each_ext_eta_zero_is_bootstrap_lut_each(oracle):
    c, p, ck = small_ctx(oracle, "uint4")
    x, tvs = words(14020, 5, p.n + 1), words(14021, 5, 2 * N)
    want = c.bootstrap_lut_each(x, tvs)
    kernels = c.last_kernels()
    assert np.array_equal(c.bootstrap_lut_each_ext(0, x, tvs), want)
    assert c.last_kernels() == kernels and "ext" not in kernels


# ---- 2. the flat select node -----------------------------------------------------------------------
@pytest.mark.parametrize("m,eta", [(4, 1), (4, 2), (64, 1), (64, 2)])
@pytest.mark.parametrize("name", ["uint4", "128"])
def test_select_ext_is_pack_spread_and_each_ext(oracle, name, m, eta):
    """Three nodes whose entries mix pool ciphertexts and constants: the host pack and spread, then the per-item
    extended bootstrap composed from the stage entry.  Host and device buffers."""
    import torch
    c, p, ck, sk, key, rows, basebit, t = small_env(oracle, name)
    g = rng(14100 + m + eta)
    pool = words(14110 + m + eta, 6, p.n + 1)
    nodes = []
    for b in range(3):
        ents = [int(g.integers(0, 6)) if g.integers(0, 3) else const(m, int(g.integers(0, m))) for _ in range(m)]
        nodes.append(([(b, 1), (b + 3, 2 - b)], ents, enc(m, b)))
    x = combine(pool, [(0, tm, k) for tm, _, k in nodes])
    tvs = select_tvs(c, rows, basebit, t, m, [entry_cts(c, pool, e) for _, e, _ in nodes])
    want, _ = each_ext_want(c, eta, x, tvs)
    got = c.lut_select_ext(key, m, eta, pool, nodes)
    assert c.last_kernels().startswith(f"k_blind_rotate_ext<{p.L},{1 << eta}>"), c.last_kernels()
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1)).tolist()
    t_pool = to_dev(pool)
    t_out = torch.full((3, c.n1), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    c.lut_select_ext_dev(key, m, eta, t_pool.data_ptr(), 6, nodes, t_out.data_ptr())
    c.sync()
    assert np.array_equal(from_dev(t_out), want)


@pytest.mark.parametrize("m,eta", [(4, 2), (64, 1), (64, 2)])
def test_select_ext_constant_entries_equal_lut_apply_ext(oracle, m, eta):
    """The E-copies identity on the device: entries Encoder.encode(f(i)) give the words of lut_apply_ext with
    lut_generate_ext(eta, m, f); eta = 0 gives lut_select's words and kernels."""
    c, p, ck, sk, key, rows, basebit, t = small_env(oracle, "uint4")
    f = lambda x: (7 * x * x + 3 * x + 1) % m  # noqa: E731
    pool = words(14200 + m, 4, p.n + 1)
    xs = [([(0, 1), (1, 1)], enc(m, 1)), ([(2, 2), (3, -1)], enc(m, 3)), ([(1, 1)], 0)]
    entries = [const(m, f(i)) for i in range(m)]
    ls = tfhe_amd.LutSet(c, tfhe_amd.lut_generate_ext(c.params, eta, m, f))
    try:
        want = c.lut_apply_ext(ls, eta, pool, [(0, tm, k) for tm, k in xs])
    finally:
        ls.close()
    got = c.lut_select_ext(key, m, eta, pool, [(tm, entries, k) for tm, k in xs])
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1)).tolist()
    flat = c.lut_select(key, m, pool, [(tm, entries, k) for tm, k in xs])
    kernels = c.last_kernels()
    assert np.array_equal(c.lut_select_ext(key, m, 0, pool, [(tm, entries, k) for tm, k in xs]), flat)
    assert c.last_kernels() == kernels and "ext" not in kernels


# ---- 3. the circuit --------------------------------------------------------------------------------
def mixed_circuit(m, seed):
    """Inputs a, b, d.  Level 1 holds eta = 2 nodes only (two ordinary, one select).  Level 2 holds all three etas:
    a theta = 1 node, an ordinary node and a select node at eta = 0, an ordinary and a select node at eta = 1 and at
    eta = 2.  Level 3 holds an eta = 0 node and an eta = 1 select node whose entries are extended nodes' wires, input
    wires and constants.  In every extended launch the first item reads the set and the last its own test vector."""
    g = rng(seed)
    circ = tfhe_amd.LutCircuit()
    a, b, d = circ.input(), circ.input(), circ.input()

    def ents(wires):
        return [int(wires[g.integers(0, len(wires))]) if g.integers(0, 4) else const(m, int(g.integers(0, m)))
                for _ in range(m)]

    e0 = circ.node(1, [(a, 1)], eta=2)
    e1 = circ.node(0, [(b, 1), (a, 2)], enc(m, 1), eta=2)
    s0 = circ.select([(d, 1)], ents([a, b, d]), eta=2)
    t = circ.node(0, [(e0, 1)], outputs=2)
    o = circ.node(3, [(e1, 1)])
    sa = circ.select([(e0, 1)], ents([e1, a, s0]))
    x1 = circ.node(2, [(e0, 1), (s0, 1)], eta=1)
    s1 = circ.select([(e1, 1)], ents([e0, e1, s0]), enc(m, 2), eta=1)
    x2 = circ.node(1, [(s0, 1)], enc(m, 3), eta=2)
    s2 = circ.select([(b, 1), (e0, 1)], ents([s0, a, e0, e1]), eta=2)
    f = circ.node(4, [(sa, 1), (o, 1), (t[1], 1)])
    s3 = circ.select([(t[0], 1), (x1, 1)], ents([x2, s2, a, s1, d]), eta=1)
    circ.output(e0, e1, s0, *t, o, sa, x1, s1, x2, s2, f, s3)
    return circ


def node_by_node(c, key, ls, circ, inputs):
    """Every wire from the flat entries, one call per node over the wires so far."""
    wires = list(np.asarray(inputs, np.uint32))
    for (lut, terms, k), theta, sel, eta in zip(circ.nodes, circ.theta, circ.sel, circ.eta):
        pool = np.array(wires)
        if sel is not None:
            out = (c.lut_select_ext(key, circ.m, eta, pool, [(terms, sel, k)]) if eta
                   else c.lut_select(key, circ.m, pool, [(terms, sel, k)]))
        elif eta:
            out = c.lut_apply_ext(ls, eta, pool, [(lut, terms, k)])
        elif theta:
            out = c.lut_apply_multi(ls, pool, [(lut, terms, k)], theta=[theta])
        else:
            out = c.lut_apply(ls, pool, [(lut, terms, k)])
        wires += list(out)
    return np.array(wires)


@pytest.mark.parametrize("name,m", [("uint4", 64), ("128", 4), ("l2small", 64)])
def test_circuit_matches_the_per_node_composition(oracle, name, m):
    """m = 64: level 2's three select nodes stage 192 entries, more than the 128 that TFHE_OPT_PACK_SCRATCH_MB = 1
    lets one chunk hold, so the level packs in several chunks; the words do not change.  Host and _dev forms."""
    import torch
    c, p, ck, sk, key, rows, basebit, t = small_env(oracle, name)
    circ = mixed_circuit(m, 14300 + m)
    levels, depth, groups = circ.schedule_ext()
    assert depth == 3 and groups.tolist() == [[0, 0, 3], [3, 2, 2], [1, 1, 0]]
    inputs = words(14310 + m, 3, p.n + 1)
    ls = tfhe_amd.LutSet(c, words(14320 + m, 8, 2 * N))  # any words: eight tables, two extended ones at eta = 2
    before = c.get_option("pack_scratch_mb")
    try:
        want = node_by_node(c, key, ls, circ, inputs)[[w for w in circ.outputs]]
        boots = int(c.device_bootstraps()[0])
        got, d1 = circ.run(c, ls, inputs, packing_key=key)
        assert int(c.device_bootstraps()[0]) == boots + len(circ.nodes)
        assert c.last_kernels().startswith(f"k_blind_rotate_ext<{p.L},2> + k_key_switch"), c.last_kernels()
        c.set_option("pack_scratch_mb", 1)
        chunked, _ = circ.run(c, ls, inputs, packing_key=key)
        t_in = to_dev(inputs)
        t_out = torch.full((len(circ.outputs), c.n1), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        d2 = circ.run_dev(c, ls, t_in.data_ptr(), t_out.data_ptr(), packing_key=key, m=m)
        c.sync()
    finally:
        c.set_option("pack_scratch_mb", before)
        ls.close()
    assert d1 == 3 and d2 == 3
    bad = np.flatnonzero((got != want).any(axis=1)).tolist()
    assert not bad, bad
    assert np.array_equal(chunked, want)
    assert np.array_equal(from_dev(t_out), want)


def test_circuit_without_eta_is_the_select_entry(oracle):
    """eta = None and all-zero etas: the words and the kernels of lut_circuit_eval_select."""
    c, p, ck, sk, key, rows, basebit, t = small_env(oracle, "uint4")
    m = 4
    circ = tfhe_amd.LutCircuit()
    a, b = circ.input(), circ.input()
    n0 = circ.node(0, [(a, 1)], outputs=2)
    n1 = circ.node(1, [(b, 1), (a, 1)])
    s = circ.select([(n1, 1)], [a, n0[0], const(m, 1), n0[1]])
    circ.output(*n0, n1, s, circ.node(2, [(s, 1)]))
    inputs = words(14400, 2, p.n + 1)
    ls = tfhe_amd.LutSet(c, words(14401, 3, 2 * N))
    try:
        want, depth = circ.run(c, ls, inputs, packing_key=key)
        kernels = c.last_kernels()
        args = (ls, key, m, inputs, circ.packed(), circ.theta, circ.select_arrays())
        ow = np.array(circ.outputs, np.uint32)
        got_null, d_null = c.lut_circuit_eval_ext(*args, None, ow)
        assert c.last_kernels() == kernels
        got_zero, d_zero = c.lut_circuit_eval_ext(*args, [0] * len(circ.nodes), ow)
        assert c.last_kernels() == kernels and "ext" not in kernels
    finally:
        ls.close()
    assert depth == d_null == d_zero == 3
    assert np.array_equal(got_null, want) and np.array_equal(got_zero, want)


# ---- 4. messages at the real key -------------------------------------------------------------------
def test_table_of_32_read_at_a_computed_address_decrypts(oracle):
    """UINT4, m = 32: 32 client words; every address x 4 encryptions goes through an eta = 1 node (a bijection f) in
    level 1, and its output addresses an eta = 2 select node over the 32 input wires in level 2.  All 128 outputs
    decrypt to words[f(x)].  The inputs of both levels are first checked against the half-spacing from the key, so
    a wrong word blames the bootstrap.  Margins from DESIGN.md 4.9e's measured output sigma 7.5e-4: half-spacing
    1/(4m) = 7.8e-3, about 10 sigma."""
    e = env(oracle)
    c, m = e.c, 32
    f = lambda x: (5 * x + 3) % m  # noqa: E731
    g = rng(14500)
    table = g.integers(0, m, m).astype(np.uint32)
    addr = np.repeat(np.arange(m, dtype=np.uint32), 4)
    inputs = np.concatenate([e.sk.encrypt_lwe_message(table, m, seed0=14500),
                             e.sk.encrypt_lwe_message(addr, m, seed0=14600)])
    check_inputs_survive(inputs[m:], addr, m, e.k.k0, 1)
    circ = tfhe_amd.LutCircuit()
    wires = [circ.input() for _ in range(m + len(addr))]
    mids = [circ.node(0, [(wires[m + i], 1)], eta=1) for i in range(len(addr))]
    reads = [circ.select([(w, 1)], wires[:m], eta=2) for w in mids]
    circ.output(*mids, *reads)
    assert circ.schedule_ext()[2].tolist() == [[0, len(addr), 0], [0, 0, len(addr)]]
    ls = tfhe_amd.LutSet(c, tfhe_amd.lut_generate_ext(c.params, 1, m, f))
    try:
        got, depth = circ.run(c, ls, inputs, packing_key=e.key)
        assert c.last_kernels().startswith("k_blind_rotate_ext<1,4>"), c.last_kernels()
    finally:
        ls.close()
    assert depth == 2
    mid_want = np.array([f(int(x)) for x in addr], np.uint32)
    mid, out = got[:len(addr)], got[len(addr):]
    assert np.array_equal(e.sk.decrypt_lwe_message(mid, m), mid_want)
    check_inputs_survive(mid, mid_want, m, e.k.k0, 2)
    dec = e.sk.decrypt_lwe_message(out, m)
    wrong = np.flatnonzero(dec != table[mid_want])
    assert wrong.size == 0, addr[wrong].tolist()


# ---- 5. refusals -----------------------------------------------------------------------------------
def test_refusals_before_any_launch(oracle):
    import torch
    c, p, ck, sk, key, rows, basebit, t = small_env(oracle, "uint4")
    m = 4
    params = tfhe_amd.make_params(SMALL["uint4"])
    other = tfhe_amd.Context(params, 0)  # no cloud key
    multi = tfhe_amd.Context(params, devices=[0, 0])
    tables = words(14700, 8, 2 * N)
    pool = words(14701, 2, p.n + 1)
    ls = tfhe_amd.LutSet(c, tables)
    circ = tfhe_amd.LutCircuit()
    a, b = circ.input(), circ.input()
    n = circ.node(1, [(a, 1)], eta=2)
    circ.output(n, circ.select([(b, 1)], [a, n, const(m, 1), b], eta=1))
    flat = [([(0, 1)], [0, 1, const(m, 1), 1])]
    try:
        ls_other, ls_multi = tfhe_amd.LutSet(other, tables), tfhe_amd.LutSet(multi, tables)
        key_other = tfhe_amd.PackingKey(other, rows, basebit, t)
        key_multi = tfhe_amd.PackingKey(multi, rows, basebit, t)
        want, _ = circ.run(c, ls, pool, packing_key=key)
        boots = int(c.device_bootstraps()[0])
        d, sel, ow = circ.packed(), circ.select_arrays(), np.array(circ.outputs, np.uint32)
        ev = lambda **kw: c.lut_circuit_eval_ext(  # noqa: E731
            kw.get("ls", ls), kw.get("key", key), kw.get("m", m), pool, kw.get("d", d), kw.get("theta", [0, 0]),
            kw.get("sel", sel), kw.get("eta", [2, 1]), ow)
        lut = lambda v: tfhe_amd.LutNodes(d.term_off, d.src, d.coef, d.konst, v)  # noqa: E731
        # eta itself
        assert status(lambda: ev(eta=[3, 1])) == INV
        assert status(lambda: ev(eta=[2, 3])) == INV
        assert status(lambda: ev(eta=[2, 1], theta=[1, 0])) == INV  # eta > 0 with theta > 0
        assert status(lambda: ev(d=lut([2, 0]))) == INV  # 2 * 4 + 4 = 12 > 8
        assert status(lambda: ev(d=lut([4, 0]), eta=[1, 1])) == INV  # 4 * 2 + 2 = 10 > 8
        assert ev(d=lut([3, 0]), eta=[1, 1])[0].shape == (2, c.n1)  # 3 * 2 + 2 = 8: the last extended table
        boots += 2
        assert status(lambda: c.bootstrap_lut_each_ext(3, pool, tables[:2])) == INV
        assert status(lambda: c.lut_select_ext(key, m, 3, pool, flat)) == INV
        # what the entry without eta refuses
        assert status(lambda: ev(d=lut([1, 1]))) == INV  # lut on a select node
        assert status(lambda: ev(theta=[0, 1])) == INV  # theta on a select node
        assert status(lambda: ev(sel=(np.array([0, 0, 3]), sel[1][:3], sel[2][:3]))) == INV
        assert status(lambda: ev(sel=(sel[0], np.array([0, 3, 0, 1]), sel[2]))) == INV  # a forward entry wire
        assert status(lambda: ev(ls=ls_other)) == INV and status(lambda: ev(key=key_other)) == INV
        assert status(lambda: c.lut_select_ext(key_other, m, 1, pool, flat)) == INV
        for bad_m in (0, 3, 1024):
            assert status(lambda: ev(m=bad_m)) == INV, bad_m
            assert status(lambda: c.lut_select_ext(key, bad_m, 2, pool, [([(0, 1)], [0] * bad_m)])) == INV, bad_m
        assert status(lambda: c.lut_select_ext(key, m, 2, pool, [([(0, 1)], [0, 1, 2, 0])])) == INV  # entry 2: no such
        # no cloud key, zero nodes, a multi-device context
        assert status(lambda: circ.run(other, ls_other, pool, packing_key=key_other)) == tfhe_amd.ERR_NO_KEY
        assert status(lambda: other.lut_select_ext(key_other, m, 2, pool, flat)) == tfhe_amd.ERR_NO_KEY
        assert status(lambda: other.bootstrap_lut_each_ext(1, pool, tables[:2])) == tfhe_amd.ERR_NO_KEY
        assert c.lut_select_ext(key, m, 2, pool, []).shape == (0, c.n1)
        assert c.bootstrap_lut_each_ext(2, np.zeros((0, c.n1), np.uint32), np.zeros((0, 2 * N), np.uint32)).shape == (0, c.n1)
        empty = tfhe_amd.LutCircuit()
        empty.input()
        empty.output(0)
        assert np.array_equal(other.lut_circuit_eval_ext(ls_other, None, 0, pool[:1], empty.packed(), None, None, [],
                                                         [0])[0], pool[:1])
        tt = torch.zeros((4, c.n1), dtype=torch.int32, device="cuda:0")
        assert status(lambda: circ.run_dev(multi, ls_multi, tt.data_ptr(), tt.data_ptr(), packing_key=key_multi)) == INV
        assert status(lambda: multi.lut_select_ext_dev(key_multi, m, 2, tt.data_ptr(), 2, flat, tt.data_ptr())) == INV
        assert status(lambda: multi.bootstrap_lut_each_ext_dev(2, tt.data_ptr(), tt.data_ptr(), tt.data_ptr(), 1)) == INV
        # nothing was launched by a refused call, and the context still works
        assert int(c.device_bootstraps()[0]) == boots
        assert np.array_equal(circ.run(c, ls, pool, packing_key=key)[0], want)
        for x_ in (ls_other, ls_multi, key_other, key_multi):
            x_.close()
    finally:
        ls.close()
        other.close()
        multi.close()
