"""The multi-output LUT bootstrap on the device (include/tfhe_gpu.h "Multi-output LUT bootstrap"):
output j of a node with theta is identityKeySwitching(sampleExtractIndex(blindRotateWithTestvec(
round_theta(x), set[lut]), j)).  Every check is word for word: against the same composition made of
the engine's own single-purpose entries (lut_round_tlwe on the host, blind_rotate_batch,
sample_extract with key_switch) and, for a few nodes, against the oracle's.  Nothing but the circuit
test decrypts: parity holds whatever the tables mean."""
import numpy as np
import pytest

import tfhe_amd
from conftest import rng
from test_lut_circuit import combine, ctx_for, tables_for

pytestmark = pytest.mark.gpu


def status(call):
    with pytest.raises(tfhe_amd.TfheError) as e:
        call()
    return e.value.status


def composition(c, pool, nodes, theta, tables):
    """The definition out of the existing entries, on context c: one blind_rotate_batch per table (it takes
    one test vector per call) and one sample_extract per theta.  -> (sum 2^theta, n+1), node-major."""
    theta, lut = np.asarray(theta, np.int64), np.array([n[0] for n in nodes])
    x = combine(pool, nodes)
    for t in np.unique(theta):
        x[theta == t] = tfhe_amd.lut_round_tlwe(c.params, int(t), x[theta == t])
    acc = np.zeros((len(nodes), 2 * c.params.N), np.uint32)
    for j in np.unique(lut):
        acc[lut == j] = c.blind_rotate_batch(x[lut == j], testvec=tables[j])
    first = np.concatenate([[0], np.cumsum(1 << theta)])
    out = np.zeros((first[-1], c.n1), np.uint32)
    for t in np.unique(theta):
        ext = c.sample_extract(acc[theta == t], np.arange(1 << t, dtype=np.uint32), key_switch=True)
        for row, i in zip(ext, np.flatnonzero(theta == t)):
            out[first[i]:first[i + 1]] = row
    return out


def oracle_composition(oracle, k, pool, nodes, theta, tables, only):
    """The oracle's own composition for the nodes `only` -> {node: (2^theta, n+1)}."""
    params = tfhe_amd.make_params({820: "uint4", 700: "128"}[k.p.n])
    x = combine(pool, nodes)
    out = {}
    for i in only:
        acc = oracle.blind_rotate(k.p, tfhe_amd.lut_round_tlwe(params, int(theta[i]), x[i])[0], tables[nodes[i][0]],
                                  k.ck.bk, k.ck.offset)
        out[i] = np.array([oracle.identity_key_switch(k.p, oracle.sample_extract_index(acc, j), k.ck.ksk)
                           for j in range(1 << int(theta[i]))])
    return out


def interleaved_tables(params, m, T):
    """T test vectors, table t the interleave of 8 tables of message modulus m (any theta <= 3 reads it)."""
    base = tables_for(params, m, 8)
    return np.array([tfhe_amd.lut_interleave(params, np.roll(base, t, axis=0)) for t in range(T)])


def random_nodes(g, B, P, T):
    """B nodes of 1-3 terms over a pool of P, coefficients in {-2, ..., 4}, a constant on every third."""
    return [((3 * i + 1) % T, [(int(g.integers(0, P)), int(g.integers(-2, 5))) for _ in range(1 + i % 3)],
             int(g.integers(0, 16)) << 27 if i % 3 == 0 else 0) for i in range(B)]


def test_parity_with_the_definition(oracle):
    """37 nodes (ragged against every workgroup and wave size in play), thetas cycling 0, 1, 2, 3 (136
    outputs), 4 interleaved tables: the composition on the same context, and the oracle's for 6 nodes."""
    c, k = ctx_for(oracle, "uint4")
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    g = rng(1401)
    pool = sk.encrypt_lwe_message(g.integers(0, 4, 8).astype(np.uint32), 16, seed0=1400)
    nodes, theta = random_nodes(g, 37, 8, 4), np.arange(37) % 4
    tables = interleaved_tables(c.params, 16, 4)
    ls = tfhe_amd.LutSet(c, tables)
    try:
        got = c.lut_apply_multi(ls, pool, nodes, theta)
        kernels = c.last_kernels()
        want = composition(c, pool, nodes, theta, tables)
    finally:
        ls.close()
    assert got.shape == (9 * 15 + 1, c.n1) == want.shape  # 9 full cycles of 15 outputs and one theta 0
    assert kernels.startswith("k_blind_rotate") and "k_lut_fanout_extract + " in kernels, kernels
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, bad.tolist()
    first = np.concatenate([[0], np.cumsum(1 << theta)])
    for i, ref in oracle_composition(oracle, k, pool, nodes, theta, tables, range(6)).items():
        assert np.array_equal(got[first[i]:first[i + 1]], ref), i


def test_theta_zero_is_lut_apply(oracle):
    """All thetas 0, and theta = NULL: lut_apply's words and lut_apply's kernels."""
    c, k = ctx_for(oracle, "uint4")
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    g = rng(1402)
    pool = sk.encrypt_lwe_message(g.integers(0, 4, 6).astype(np.uint32), 16, seed0=1410)
    nodes = random_nodes(g, 13, 6, 5)
    ls = tfhe_amd.LutSet(c, tables_for(c.params, 16, 5))
    try:
        want = c.lut_apply(ls, pool, nodes)
        kernels = c.last_kernels()
        for theta in (np.zeros(13, np.uint32), None):
            got = c.lut_apply_multi(ls, pool, nodes, theta)
            assert c.last_kernels() == kernels and "fanout" not in kernels, c.last_kernels()
            assert np.array_equal(got, want)
    finally:
        ls.close()


ADD_PAIRS = [(0xB7, 0x5E), (0xFF, 0xFF), (0, 0), (0xFF, 1), (0x3C, 0xC4)]


def test_fused_adder_circuit(oracle):
    """5 additions of 8-bit numbers as four base-4 digits at m = 8 (2 message bits, 1 bit of carry room, 1 bit
    paid for theta = 1): 20 two-output nodes at depth 4, and one theta = 0 node (a digit's message through the
    plain table) mixed into level 2.  The evaluator's wires equal level-by-level lut_apply_multi word for word,
    the _dev variant on torch buffers gives the same words, and the sums decrypt."""
    import torch
    c, k = ctx_for(oracle, "uint4")
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    m = 8
    msg, carry = (tfhe_amd.lut_generate(c.params, m, f) for f in (lambda x: x % 4, lambda x: x // 4))
    tables = np.array([tfhe_amd.lut_interleave(c.params, [msg, carry]), msg])
    circ = tfhe_amd.LutCircuit()
    ins = [[circ.input() for _ in range(8)] for _ in ADD_PAIRS]  # a's digits, then b's, LSB first
    sums = [circ.radix_add_fused(w[:4], w[4:], lut=0) for w in ins]
    again = circ.node(1, [(sums[1][0], 1)])  # theta = 0, level 2
    circ.output(*range(circ.n_wires))
    digits = lambda v: np.array([(v >> (2 * i)) & 3 for i in range(4)], np.uint32)
    inputs = np.concatenate([np.concatenate([sk.encrypt_lwe_message(digits(a), m, seed0=100 * q),
                                             sk.encrypt_lwe_message(digits(b), m, seed0=100 * q + 50)])
                             for q, (a, b) in enumerate(ADD_PAIRS)])
    levels, depth = circ.schedule()
    assert len(circ.nodes) == 21 and depth == 4 and levels[-1] == 2 and circ.n_wires == 40 + 41
    theta = np.array(circ.theta)
    first = circ.n_inputs + np.concatenate([[0], np.cumsum(1 << theta)])
    t_in = torch.from_numpy(inputs.view(np.int32)).to("cuda:0")
    t_out = torch.zeros((circ.n_wires, c.n1), dtype=torch.int32, device="cuda:0")
    ls = tfhe_amd.LutSet(c, tables)
    try:
        wires, ran = circ.run(c, ls, inputs)
        kernels = c.last_kernels()
        want = np.zeros_like(wires)
        want[:circ.n_inputs] = inputs
        for lv in range(1, depth + 1):
            idx = np.flatnonzero(levels == lv)
            out = c.lut_apply_multi(ls, want, [circ.nodes[i] for i in idx], theta[idx])
            at = 0
            for i in idx:
                want[first[i]:first[i + 1]] = out[at:at + (1 << theta[i])]
                at += 1 << theta[i]
        try:
            c.set_stream(torch.cuda.current_stream().cuda_stream)
            ran_dev = circ.run_dev(c, ls, t_in.data_ptr(), t_out.data_ptr())
            c.sync()
        finally:
            c.set_stream(None)
    finally:
        ls.close()
    assert ran == 4 and ran_dev == 4
    assert "k_lut_fanout_extract + " in kernels, kernels
    bad = np.flatnonzero((wires != want).any(axis=1))
    assert bad.size == 0, bad.tolist()
    assert np.array_equal(t_out.cpu().numpy().view(np.uint32), wires)
    got = [sum(int(d) << (2 * i) for i, d in enumerate(sk.decrypt_lwe_message(wires[s], m))) for s in sums]
    assert got == [a + b for a, b in ADD_PAIRS], [hex(s) for s in got]
    assert int(sk.decrypt_lwe_message(wires[again], m)[0]) == (0xFF + 0xFF) & 3


def test_tail_split_with_a_table_per_item(oracle):
    """128-bit, B = 4 x CUs + 3, theta = 1, every node its own table index: the blind rotation (to the
    accumulators, a table per item) runs the full rounds in the whole form and the ragged tail in the
    latency form, whose launch reads the selectors and writes the accumulators from `full` on.  Parity with
    the composition, whose blind rotations are single-table batches below the split size."""
    import torch
    c, k = ctx_for(oracle, "128")
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 4 * cus + 3
    g = rng(1403)
    pool = sk.encrypt_lwe_message(g.integers(0, 2, 5).astype(np.uint32), 4, seed0=2400)
    T = 5
    lut = np.arange(B) % T  # neighbours differ everywhere, across the split too
    src, coef = g.integers(0, 5, B), g.integers(1, 4, B)
    nodes = [(int(lut[i]), [(int(src[i]), int(coef[i]))], 0) for i in range(B)]
    theta = np.ones(B, np.uint32)
    tables = interleaved_tables(c.params, 4, T)
    ls = tfhe_amd.LutSet(c, tables)
    try:
        got = c.lut_apply_multi(ls, pool, nodes, theta)
        kernels = c.last_kernels()
        want = composition(c, pool, nodes, theta, tables)
    finally:
        ls.close()
    assert kernels.startswith("k_blind_rotate_assist<true,TV>"), kernels
    assert got.shape == (2 * B, c.n1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad[:10] // 2).tolist()


def test_128_bit_set_fused_and_reference(oracle):
    """9 nodes, theta = 1, m = 4 at the 128-bit set (n = 700: margin 128 positions against sigma 10.8), under
    forced fused arithmetic (the margin guard's recompute launch runs over the accumulators with a table per
    item) and under the reference trees: the same words, and the oracle's for 3 nodes."""
    c, k = ctx_for(oracle, "128")
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    g = rng(1404)
    pool = sk.encrypt_lwe_message(g.integers(0, 2, 5).astype(np.uint32), 4, seed0=2410)
    nodes, theta = random_nodes(g, 9, 5, 3), np.ones(9, np.uint32)
    tables = interleaved_tables(c.params, 4, 3)
    ls = tfhe_amd.LutSet(c, tables)
    try:
        got = {}
        for name, arith in (("fused", tfhe_amd.ARITH_FUSED_FORCED), ("reference", tfhe_amd.ARITH_REFERENCE)):
            for form in ("auto", "whole"):
                with c.options(arith=arith, br_form=form):
                    got[name, form] = c.lut_apply_multi(ls, pool, nodes, theta)
                    if name == "fused":
                        assert c.last_kernels().split(" + ")[0].endswith("fused)"), c.last_kernels()
    finally:
        ls.close()
    ref = got["reference", "auto"]
    for key, words in got.items():
        assert np.array_equal(words, ref), key
    for i, want in oracle_composition(oracle, k, pool, nodes, theta, tables, (0, 4, 8)).items():
        assert np.array_equal(ref[2 * i:2 * i + 2], want), i


def test_errors_leave_the_context_usable(oracle):
    """theta = 4, a term wire at or past the node's first output wire, a set from another context and a _dev
    call on a multi-device context: TFHE_ERR_INVALID each, and a valid call afterwards gives the right words."""
    import torch
    c, k = ctx_for(oracle, "uint4")
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    g = rng(1405)
    pool = sk.encrypt_lwe_message(g.integers(0, 4, 4).astype(np.uint32), 8, seed0=1450)
    nodes, theta = random_nodes(g, 5, 4, 2), np.array([1, 0, 2, 1, 3], np.uint32)
    tables = interleaved_tables(c.params, 8, 2)
    ls = tfhe_amd.LutSet(c, tables)
    other = tfhe_amd.Context("uint4", 0)
    multi = tfhe_amd.Context.multi("uint4", devices=[0, 0])
    try:
        ls_other, ls_multi = tfhe_amd.LutSet(other, tables), tfhe_amd.LutSet(multi, tables)
        want = c.lut_apply_multi(ls, pool, nodes, theta)
        bad_theta = theta.copy()
        bad_theta[3] = 4
        assert status(lambda: c.lut_apply_multi(ls, pool, nodes, bad_theta)) == tfhe_amd.ERR_INVALID
        assert status(lambda: c.lut_apply_multi(ls_other, pool, nodes, theta)) == tfhe_amd.ERR_INVALID
        t = torch.zeros((17, c.n1), dtype=torch.int32, device="cuda:0")
        assert status(lambda: multi.lut_apply_multi_dev(ls_multi, t.data_ptr(), 4, nodes, theta, t.data_ptr())) \
            == tfhe_amd.ERR_INVALID
        # a circuit of 2 inputs: node 0 (theta 1) drives wires 2, 3, node 1 wire 4
        def circuit(wire0, wire1, th=(1, 0), ctx=c, s=ls):
            d = tfhe_amd.LutNodes([0, 1, 2], [wire0, wire1], [1, 1], [0, 0], [0, 1])
            return ctx.lut_circuit_eval_multi(s, pool[:2], d, np.array(th, np.uint32), [2, 3, 4])
        assert status(lambda: circuit(2, 3)) == tfhe_amd.ERR_INVALID  # node 0 reads its own first wire
        assert status(lambda: circuit(3, 3)) == tfhe_amd.ERR_INVALID  # ... its second
        assert status(lambda: circuit(0, 4)) == tfhe_amd.ERR_INVALID  # node 1 reads its own wire
        assert status(lambda: circuit(0, 3, th=(1, 4))) == tfhe_amd.ERR_INVALID
        assert status(lambda: circuit(0, 3, s=ls_other)) == tfhe_amd.ERR_INVALID
        d = tfhe_amd.LutNodes([0, 1, 2], [0, 3], [1, 1], [0, 0], [0, 1])
        assert status(lambda: multi.lut_circuit_eval_multi_dev(ls_multi, t.data_ptr(), 2, d, np.array([1, 0], np.uint32),
                                                               [2, 3, 4], t.data_ptr())) == tfhe_amd.ERR_INVALID
        # and the context still works: the batch's words again, and the small circuit equals its two batches
        assert np.array_equal(c.lut_apply_multi(ls, pool, nodes, theta), want)
        outs, depth = circuit(0, 3)
        assert depth == 2
        lv1 = c.lut_apply_multi(ls, pool[:2], [(0, [(0, 1)], 0)], [1])
        assert np.array_equal(outs[:2], lv1)
        assert np.array_equal(outs[2:], c.lut_apply_multi(ls, lv1, [(1, [(1, 1)], 0)], [0]))
        assert np.array_equal(want, composition(c, pool, nodes, theta, tables))
        ls_other.close()
        ls_multi.close()
    finally:
        ls.close()
        other.close()
        multi.close()
