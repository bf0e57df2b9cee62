"""Select nodes on the device (include/tfhe_gpu.h "Select nodes") at UINT4: LUT-circuit nodes whose table is packed
from m earlier wires or constants.  Word for word (np.array_equal) against what the definition reduces to: an
ordinary node for constant entries, lut_apply2 for node2, and the per-level composition from lut_apply, pack_tlwe,
lut_spread and bootstrap_lut_each for a level that mixes both kinds, with a theta = 1 node beside a select node and
under the smallest pack scratch.  Two tests read messages: a read of 16 client words by a computed address, and a
three-digit tree over a random 64-entry table with the outputs' measured phase error."""
import numpy as np
import pytest

import tfhe_amd
from conftest import rng
from test_lut_circuit import combine, tables_for
from test_lut_tree import env, from_dev, status, to_dev, two_tables

pytestmark = pytest.mark.gpu

INV = tfhe_amd.ERR_INVALID
N = 1024


def enc(m, v):
    """Encoder.new(m).encode(v) as a Torus word: v / (2m), exact for a power of two m."""
    return ((int(v) % m) << 32) // (2 * m)


def const(m, v):
    return ("const", enc(m, v))


def trivial(c, word):
    ct = np.zeros(c.n1, np.uint32)
    ct[-1] = word
    return ct


def select_definition(e, m, pool, x_nodes, entries):
    """Steps 1-3 of the header from the separate device entries: entries is (B, m, n+1) ciphertexts in pack order,
    x_nodes the (0, terms, const) of the B digits over pool."""
    c, w = e.c, N // m
    packed = c.pack_tlwe(e.key, np.asarray(entries, np.uint32).reshape(-1, m, c.n1), np.arange(m, dtype=np.uint32) * w)
    tv = c.lut_spread(packed, w, 2 * N - N // (2 * m))
    return c.bootstrap_lut_each(combine(pool, x_nodes), tv)


# ---- 1. constant entries are an ordinary node ------------------------------------------------------
@pytest.mark.parametrize("m", [4, 16])
def test_constant_entries_equal_an_ordinary_node(oracle, m):
    """Three nodes with different x (two terms and a konst each), entries Encoder.encode(f(i)) for a non-monotone f:
    the words of lut_apply with lut_generate(m, f), through the flat call and through a circuit."""
    e = env(oracle)
    c = e.c
    f = lambda x: (7 * x * x + 3 * x + 1) % m  # noqa: E731
    pool = e.sk.encrypt_lwe_message(rng(12000 + m).integers(0, m, 4).astype(np.uint32), m, seed0=12000 + 10 * m)
    xs = [([(0, 1), (1, 1)], enc(m, 1)), ([(2, 2), (3, -1)], enc(m, 3)), ([(1, 1), (3, 1)], enc(m, m - 1))]
    entries = [const(m, f(i)) for i in range(m)]
    ls = tfhe_amd.LutSet(c, tfhe_amd.lut_generate(c.params, m, f)[None])
    try:
        want = c.lut_apply(ls, pool, [(0, t, k) for t, k in xs])
        flat = c.lut_select(e.key, m, pool, [(t, entries, k) for t, k in xs])
        circ = tfhe_amd.LutCircuit()
        for _ in range(4):
            circ.input()
        circ.output(*[circ.select(t, entries, k) for t, k in xs])
        got, depth = circ.run(c, ls, pool, packing_key=e.key, m=m)
    finally:
        ls.close()
    assert depth == 1
    assert np.array_equal(flat, want), np.flatnonzero((flat != want).any(axis=1)).tolist()
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1)).tolist()


# ---- 2. node2 is lut_apply2 ------------------------------------------------------------------------
@pytest.mark.parametrize("m", [4, 16])
def test_node2_equals_lut_apply2(oracle, m):
    """F = 2 (low and high digit of x * y), three (x, y) pairs: one circuit of six node2 gives lut_apply2's words,
    also through run_dev on torch buffers."""
    import torch
    e = env(oracle)
    c = e.c
    g = rng(12100 + m)
    pool = e.sk.encrypt_lwe_message(g.integers(0, m, 6).astype(np.uint32), m, seed0=12100 + 10 * m)
    pairs = [(0, 1), (2, 3), (5, 4)]
    nodes = [(fn, x, y) for x, y in pairs for fn in (0, 1)]
    circ = tfhe_amd.LutCircuit()
    for _ in range(6):
        circ.input()
    circ.output(*[circ.node2(fn * m, [(x, 1)], [(y, 1)], m) for fn, x, y in nodes])
    ls = tfhe_amd.LutSet(c, two_tables(c.params, m))
    try:
        want = c.lut_apply2(ls, e.key, m, pool, nodes)
        got, depth = circ.run(c, ls, pool, packing_key=e.key)
        t_in = to_dev(pool)
        t_out = torch.full((6, c.n1), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the circuit on the context's
        depth_dev = circ.run_dev(c, ls, t_in.data_ptr(), t_out.data_ptr(), packing_key=e.key, m=m)
        c.sync()
    finally:
        ls.close()
    assert depth == 2 and depth_dev == 2
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1)).tolist()
    assert np.array_equal(from_dev(t_out), want)


# ---- 3. a level of both kinds ----------------------------------------------------------------------
def mixed_circuit(m, with_level3):
    """Inputs a, b, d (wires 0..2).  Level 1: n0, n1, n2 (wires 3..5).  Level 2: the ordinary o1, o2 (6, 7) and the
    select nodes s1, s2 (8, 9): s1's entries are an input wire, a constant and two level-1 outputs.  Level 3: one
    ordinary node over o1, s1 and s2."""
    circ = tfhe_amd.LutCircuit()
    a, b, d = circ.input(), circ.input(), circ.input()
    n0, n1, n2 = circ.node(0, [(a, 1)]), circ.node(1, [(b, 1)]), circ.node(2, [(a, 1), (b, 1)])
    o1, o2 = circ.node(3, [(n0, 1)]), circ.node(4, [(n1, 1), (n2, 1)], enc(m, 1))
    s1 = circ.select([(n0, 1)], [d, const(m, 2), n1, n2])
    s2 = circ.select([(b, 1), (n2, 1)], [n2, n1, n0, n1], enc(m, 3))
    outs = [n0, n1, n2, o1, o2, s1, s2]
    if with_level3:
        outs.append(circ.node(5, [(o1, 1), (s1, 1), (s2, 1)]))
    circ.output(*outs)
    return circ


def test_mixed_level_matches_the_per_level_composition(oracle):
    e = env(oracle)
    c, m = e.c, 4
    inputs = e.sk.encrypt_lwe_message(np.array([1, 3, 2], np.uint32), m, seed0=12200)
    ls = tfhe_amd.LutSet(c, tables_for(c.params, m, 6))
    try:
        # the composition, level by level, the wires routed by hand
        l1 = c.lut_apply(ls, inputs, [(0, [(0, 1)]), (1, [(1, 1)]), (2, [(0, 1), (1, 1)])])
        w2 = np.concatenate([inputs, l1])  # wires 0..5
        ord2 = c.lut_apply(ls, w2, [(3, [(3, 1)]), (4, [(4, 1), (5, 1)], enc(m, 1))])
        ents = [[w2[2], trivial(c, enc(m, 2)), w2[4], w2[5]], [w2[5], w2[4], w2[3], w2[4]]]
        sel2 = select_definition(e, m, w2, [(0, [(3, 1)], 0), (0, [(1, 1), (5, 1)], enc(m, 3))], ents)
        w3 = np.concatenate([w2, ord2, sel2])  # wires 0..9
        l3 = c.lut_apply(ls, w3, [(5, [(6, 1), (8, 1), (9, 1)])])
        want = np.concatenate([l1, ord2, sel2, l3])
        # what a per-item-test-vector launch of the mixed level's size reports
        c.bootstrap_lut_each(w2[:4], np.tile(tables_for(c.params, m, 1), (4, 1)))
        each_kernels = c.last_kernels()

        c.profile_begin()
        got, depth = mixed_circuit(m, True).run(c, ls, inputs, packing_key=e.key)
        launches = c.profile_end()[2]
        c.profile_begin()
        got2, depth2 = mixed_circuit(m, False).run(c, ls, inputs, packing_key=e.key)
        launches2 = c.profile_end()[2]
        level2_kernels = c.last_kernels()  # the last bootstrap launch of the two-level circuit: its mixed level
    finally:
        ls.close()
    assert depth == 3 and depth2 == 2
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1)).tolist()
    assert np.array_equal(got2, want[:7])
    # one bootstrap launch per level, the mixed level's the per-item-test-vector kernel bootstrap_lut_each runs
    assert launches == 3 and launches2 == 2, (launches, launches2)
    assert level2_kernels == each_kernels, (level2_kernels, each_kernels)
    assert "TV" in level2_kernels.split(" + ")[0], level2_kernels


# ---- 4. a multi-output node and a select node in one level -----------------------------------------
def test_theta_node_and_select_node_share_a_level(oracle):
    """m = 8: a theta = 1 node, a theta = 0 node and a select node, all of level 1, then a node over all of them;
    each result is word-equal to its separate call."""
    e = env(oracle)
    c, m = e.c, 8
    tabs = tables_for(c.params, m, 3)
    tables = np.concatenate([tfhe_amd.lut_interleave(c.params, tabs[:2])[None], tabs])  # 0: interleaved, 1..3 plain
    pool = e.sk.encrypt_lwe_message(np.array([2, 6], np.uint32), m, seed0=12300)
    entries = [0, 1, const(m, 5), const(m, 0), 1, 0, const(m, 7), const(m, 3)]
    circ = tfhe_amd.LutCircuit()
    a, b = circ.input(), circ.input()
    hi_lo = circ.node(0, [(a, 1)], outputs=2)
    plain = circ.node(2, [(b, 1)], enc(m, 1))
    sel = circ.select([(b, 1)], entries, enc(m, 2))
    last = circ.node(3, [(hi_lo[1], 1), (sel, 1)])
    circ.output(*hi_lo, plain, sel, last)
    ls = tfhe_amd.LutSet(c, tables)
    try:
        got, depth = circ.run(c, ls, pool, packing_key=e.key)
        multi = c.lut_apply_multi(ls, pool, [(0, [(0, 1)])], theta=[1])
        one = c.lut_apply(ls, pool, [(2, [(1, 1)], enc(m, 1))])
        flat = c.lut_select(e.key, m, pool, [([(1, 1)], entries, enc(m, 2))])
        after = c.lut_apply(ls, np.concatenate([multi, flat]), [(3, [(1, 1), (2, 1)])])
    finally:
        ls.close()
    assert depth == 2 and circ.schedule()[0].tolist() == [1, 1, 1, 2]
    assert np.array_equal(got[:2], multi)
    assert np.array_equal(got[2], one[0])
    assert np.array_equal(got[3], flat[0])
    assert np.array_equal(got[4], after[0])


# ---- 5. chunking -----------------------------------------------------------------------------------
def test_chunked_pack_changes_no_word(oracle):
    """Five select nodes at m = 16 in one level: 80 entries, more than the 32 items' sums TFHE_OPT_PACK_SCRATCH_MB = 1
    (the smallest value) holds, so the level packs in three chunks of two nodes."""
    e = env(oracle)
    c, m = e.c, 16
    g = rng(12400)
    pool = e.sk.encrypt_lwe_message(g.integers(0, m, 8).astype(np.uint32), m, seed0=12400)
    circ = tfhe_amd.LutCircuit()
    for _ in range(8):
        circ.input()
    for k in range(5):
        ents = [int(w) if i % 3 else const(m, int(w)) for i, w in enumerate(g.integers(0, 8, m))]
        circ.output(circ.select([(k, 1), (k + 1, 1)], ents, enc(m, k)))
    ls = tfhe_amd.LutSet(c, tables_for(c.params, m, 1))
    before = c.get_option("pack_scratch_mb")
    try:
        want, _ = circ.run(c, ls, pool, packing_key=e.key)
        c.set_option("pack_scratch_mb", 1)
        got, _ = circ.run(c, ls, pool, packing_key=e.key)
        flat = c.lut_select(e.key, m, pool, [(n[1], s, n[2]) for n, s in zip(circ.nodes, circ.sel)])
    finally:
        c.set_option("pack_scratch_mb", before)
        ls.close()
    assert np.array_equal(got, want)
    assert np.array_equal(flat, want)


# ---- 6. a read by a computed address ---------------------------------------------------------------
def test_computed_address_read_decrypts(oracle):
    """16 client words and all 16 addresses, each (a + b) mod 16 from its own two fresh digits by a node2, then 16
    independent select nodes over the 16 input wires in one level: every output decrypts to the addressed word."""
    e = env(oracle)
    c, m = e.c, 16
    g = rng(12500)
    words = g.integers(0, m, m).astype(np.uint32)
    a = g.integers(0, m, m).astype(np.uint32)
    b = (np.arange(m, dtype=np.uint32) - a) % m  # address i = (a_i + b_i) mod 16
    inputs = np.concatenate([e.sk.encrypt_lwe_message(words, m, seed0=12500), e.sk.encrypt_lwe_message(a, m, seed0=12600),
                             e.sk.encrypt_lwe_message(b, m, seed0=12700)])
    circ = tfhe_amd.LutCircuit()
    wires = [circ.input() for _ in range(3 * m)]
    for i in range(m):
        addr = circ.node2(0, [(wires[m + i], 1)], [(wires[2 * m + i], 1)], m)
        circ.output(circ.select([(addr, 1)], wires[:m]))
    ls = tfhe_amd.LutSet(c, tfhe_amd.lut_generate2(c.params, m, lambda x, y: (x + y) % m))
    try:
        got, depth = circ.run(c, ls, inputs, packing_key=e.key)
    finally:
        ls.close()
    assert depth == 3
    dec = e.sk.decrypt_lwe_message(got, m)
    assert np.array_equal(dec, words), np.flatnonzero(dec != words).tolist()


# ---- 7. a three-digit tree -------------------------------------------------------------------------
def test_three_digit_tree_decrypts_and_its_output_noise(oracle):
    """m = 4, a random 64-entry table, all 64 addresses each from its own three fresh digits: 64 * (16 + 4 + 1)
    bootstraps in three levels, every output right.  The outputs' phase error against the slot centre is printed.
    Measured on the MI355X with these keys and seeds: sigma = 1.324e-3, max = 2.579e-3 over the 64 outputs, against
    a decision margin of 1/16 (messages are 1/8 apart): 47 sigma."""
    e = env(oracle)
    c, m = e.c, 4
    g = rng(12800)
    table = g.integers(0, m, m ** 3).astype(np.uint32)
    addr = np.arange(m ** 3, dtype=np.uint32)
    digits = np.stack([addr // 16, (addr // 4) % 4, addr % 4], axis=1).reshape(-1)  # most significant first
    inputs = e.sk.encrypt_lwe_message(digits, m, seed0=12800)
    tables = np.array([tfhe_amd.lut_generate(c.params, m, lambda x, r=r: int(table[4 * r + x])) for r in range(16)])
    circ = tfhe_amd.LutCircuit()
    wires = [circ.input() for _ in range(3 * 64)]
    for k in range(64):
        circ.output(circ.lookup([[(wires[3 * k + j], 1)] for j in range(3)], 0, m))
    assert len(circ.nodes) == 64 * 21
    ls = tfhe_amd.LutSet(c, tables)
    try:
        got, depth = circ.run(c, ls, inputs, packing_key=e.key)
    finally:
        ls.close()
    assert depth == 3
    dec = e.sk.decrypt_lwe_message(got, m)
    assert np.array_equal(dec, table), np.flatnonzero(dec != table).tolist()
    k0 = np.asarray(e.k.k0, np.uint64)
    ph = (got[:, -1].astype(np.uint64) - (got[:, :-1].astype(np.uint64) * k0).sum(axis=1)) & np.uint64(0xFFFFFFFF)
    err = (ph.astype(np.float64) / 2.0 ** 32 - table / (2.0 * m) + 0.5) % 1.0 - 0.5
    sigma, worst = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
    print(f"three-digit tree, output phase error: sigma = {sigma:.3e}, max = {worst:.3e}; message spacing 1/8 = "
          f"{1 / 8:.3e}, decision margin 1/16 = {1 / 16:.3e} ({1 / 16 / sigma:.1f} sigma)")


# ---- 8. refusals -----------------------------------------------------------------------------------
def test_device_entries_refuse_before_any_launch(oracle):
    import torch
    e = env(oracle)
    c, m = e.c, 4
    pool = e.sk.encrypt_lwe_message(np.array([1, 2], np.uint32), m, seed0=12900)
    tables = tables_for(c.params, m, 2)
    other = tfhe_amd.Context("uint4", 0)  # no cloud key
    multi = tfhe_amd.Context.multi("uint4", devices=[0, 0])
    ls = tfhe_amd.LutSet(c, tables)
    circ = tfhe_amd.LutCircuit()
    a, b = circ.input(), circ.input()
    n = circ.node(1, [(a, 1)])
    circ.output(circ.select([(b, 1)], [a, n, const(m, 1), b]))
    flat_nodes = [([(0, 1)], [0, 1, const(m, 1), 1])]
    try:
        ls_other, ls_multi = tfhe_amd.LutSet(other, tables), tfhe_amd.LutSet(multi, tables)
        key_other = tfhe_amd.PackingKey(other, e.rows, e.basebit, e.t)
        boots = int(c.device_bootstraps()[0])
        want, _ = circ.run(c, ls, pool, packing_key=e.key)
        assert int(c.device_bootstraps()[0]) == boots + 2
        boots += 2
        # a packing key or a set of another context
        assert status(lambda: circ.run(c, ls_other, pool, packing_key=e.key)) == INV
        assert status(lambda: circ.run(c, ls, pool, packing_key=key_other)) == INV
        assert status(lambda: c.lut_select(key_other, m, pool, flat_nodes)) == INV
        # theta (or lut) on a select node, a wrong entry count, a forward entry wire, m
        d, sel, ow = circ.packed(), circ.select_arrays(), np.array(circ.outputs, np.uint32)
        ev = lambda **kw: c.lut_circuit_eval_select(  # noqa: E731
            ls, e.key, kw.get("m", m), pool, kw.get("d", d), kw.get("theta", [0, 0]), kw.get("sel", sel), ow)
        assert np.array_equal(ev()[0], want)
        boots += 2
        assert status(lambda: ev(theta=[0, 1])) == INV
        assert status(lambda: ev(d=tfhe_amd.LutNodes(d.term_off, d.src, d.coef, d.konst, [1, 1]))) == INV
        assert status(lambda: ev(sel=(np.array([0, 0, 3]), sel[1][:3], sel[2][:3]))) == INV
        assert status(lambda: ev(sel=(sel[0], np.array([0, 3, 0, 1]), sel[2]))) == INV
        assert status(lambda: ev(sel=(np.array([0, 4, 4]), sel[1], sel[2]))) == INV  # node 0 reading wire 2
        assert status(lambda: ev(sel=(np.array([1, 1, 4]), sel[1], sel[2]))) == INV
        for bad_m in (0, 1, 3, 1024):
            assert status(lambda: ev(m=bad_m)) == INV, bad_m
            assert status(lambda: c.lut_select(e.key, bad_m, pool, [([(0, 1)], [0] * bad_m)])) == INV, bad_m
        assert status(lambda: c.lut_select(e.key, m, pool, [([(0, 1)], [0, 1, 2, 0])])) == INV  # entry 2: not in the pool
        assert status(lambda: c.lut_select(e.key, m, pool, [([(2, 1)], [0, 1, 1, 0])])) == INV  # term 2: not in the pool
        # sel_off = NULL runs the _multi entry, whatever the key and m
        plain = tfhe_amd.LutCircuit()
        pa = plain.input()
        plain.output(plain.node(1, [(pa, 1)]))
        got_null = c.lut_circuit_eval_select(ls, None, 0, pool[:1], plain.packed(), None, None, [1])[0]
        assert np.array_equal(got_null, plain.run(c, ls, pool[:1])[0])
        boots += 2
        # zero nodes
        assert c.lut_select(e.key, m, pool, []).shape == (0, c.n1)
        # no cloud key
        assert status(lambda: circ.run(other, ls_other, pool, packing_key=key_other)) == tfhe_amd.ERR_NO_KEY
        assert status(lambda: other.lut_select(key_other, m, pool, flat_nodes)) == tfhe_amd.ERR_NO_KEY
        # _dev on a multi-device context
        t = torch.zeros((4, c.n1), dtype=torch.int32, device="cuda:0")
        key_multi = tfhe_amd.PackingKey(multi, e.rows, e.basebit, e.t)
        assert status(lambda: circ.run_dev(multi, ls_multi, t.data_ptr(), t.data_ptr(), packing_key=key_multi)) == INV
        assert status(lambda: multi.lut_select_dev(key_multi, m, t.data_ptr(), 2, flat_nodes, t.data_ptr())) == INV
        # nothing was launched by a refused call, and the context still works
        assert int(c.device_bootstraps()[0]) == boots
        assert np.array_equal(circ.run(c, ls, pool, packing_key=e.key)[0], want)
        for x_ in (ls_other, ls_multi, key_other, key_multi):
            x_.close()
    finally:
        ls.close()
        other.close()
        multi.close()
