"""LUT circuits on the device (include/tfhe_gpu.h "LUT circuits"): node i computes the integer
combination x_i = sum coef * pool[src] + konst (wrapping u32, TLWELv0.add / addMul / subMul,
tlwe.zig:120-240) and bootstraps it with ITS OWN table of a resident set.  Every check is
bit-exact against the oracle: numpy computes x_i, oracle.gate_batch(COPY, x_i, testvec = the
node's table) the words tfhe_gpu_bootstrap_lut_batch would return (blindRotateWithTestvec,
sampleExtractIndex(0), identityKeySwitching).  The oracle costs ~60 ms per item on the host, so
each test compares a few dozen items at most and the references are computed once per module."""
import numpy as np
import pytest

import tfhe_amd
from conftest import crafted_near_tie_case, get_keys, rng

pytestmark = pytest.mark.gpu

COPY = 255
_CTX, _CACHE = {}, {}


def ctx_for(oracle, pname):
    """Context with the oracle's seeded cloud key loaded (sk 42, ck 43)."""
    if pname not in _CTX:
        k = get_keys(oracle, pname)
        c = tfhe_amd.Context(pname, 0)
        c.load_cloud_key(k.ck.offset, k.ck.testvec, k.ck.bk, k.ck.ksk)
        _CTX[pname] = (c, k)
    return _CTX[pname]


def tables_for(params, m, T):
    """T tables f_j(x) = ((j + 1) x + j) mod m."""
    return np.array([tfhe_amd.lut_generate(params, m, lambda x, j=j: ((j + 1) * x + j) % m) for j in range(T)])


def combine(pool, nodes):
    """x_i of every node, u32 wraparound on all n + 1 words."""
    pool = np.asarray(pool, np.uint32)
    x = np.zeros((len(nodes), pool.shape[1]), np.uint32)
    for i, (_, terms, konst) in enumerate(nodes):
        acc = np.zeros(pool.shape[1], np.uint64)
        for s, c in terms:
            acc += (pool[s].astype(np.uint64) * np.uint64(c % (1 << 32))) & np.uint64(0xFFFFFFFF)
        acc[-1] += np.uint64(konst)
        x[i] = (acc & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return x


def oracle_bootstrap(oracle, p, keys, x, lut, tables, only=None):
    """The oracle's LUT bootstrap of x[i] with tables[lut[i]] for i in `only` (default: all), one
    gate_batch call per table (the same words as one call per item)."""
    lut = np.asarray(lut)
    only = np.arange(len(lut)) if only is None else np.asarray(only)
    out = np.zeros((len(lut), x.shape[1]), np.uint32)
    for j in np.unique(lut[only]):
        sel = only[lut[only] == j]
        out[sel] = oracle.gate_batch(p, np.full(sel.size, COPY, np.uint8), x[sel], x[sel], keys, threads=8,
                                     testvec=tables[j])
    return out


def oracle_nodes(oracle, p, keys, pool, nodes, tables, only=None):
    return oracle_bootstrap(oracle, p, keys, combine(pool, nodes), [n[0] for n in nodes], tables, only)


def case1(oracle):
    """13 nodes (not a multiple of 4 or 8) over 8 fresh UINT4 encryptions and 5 tables; lut[i] =
    (3i + 1) mod 5, so neighbours in any 4- or 8-item workgroup differ; 1-3 terms with coefficients
    in {-2, ..., 4}, some konst != 0, node 6 without terms."""
    if "case1" not in _CACHE:
        c, k = ctx_for(oracle, "uint4")
        sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
        g = rng(1301)
        pool = sk.encrypt_lwe_message(g.integers(0, 4, 8).astype(np.uint32), 16, seed0=1300)
        nodes = []
        for i in range(13):
            nt = 0 if i == 6 else int(g.integers(1, 4))
            terms = [(int(g.integers(0, 8)), int(g.integers(-2, 5))) for _ in range(nt)]
            konst = 5 << 27 if i == 6 else (int(g.integers(0, 16)) << 27 if i % 3 == 0 else 0)
            nodes.append(((3 * i + 1) % 5, terms, konst))
        tables = tables_for(c.params, 16, 5)
        want = oracle_nodes(oracle, k.p, k.ck, pool, nodes, tables)
        _CACHE["case1"] = (pool, nodes, tables, want)
    return _CACHE["case1"]


def test_forms_at_uint4(oracle):
    """Per-item tables in the latency (auto at this size), whole and octo forms: the same words
    from each, the forced form's kernel, and all 13 items equal the oracle."""
    c, _ = ctx_for(oracle, "uint4")
    pool, nodes, tables, want = case1(oracle)
    assert sum(1 for n in nodes if n[2]) >= 2 and not nodes[6][1] and {len(n[1]) for n in nodes} == {0, 1, 2, 3}
    ls = tfhe_amd.LutSet(c, tables)
    try:
        prefix = {"auto": "k_blind_rotate_wide<1", "whole": "k_blind_rotate<1", "octo": "k_blind_rotate_octo<1"}
        for form in ("auto", "whole", "octo"):
            with c.options(br_form=form):
                got = c.lut_apply(ls, pool, nodes)
                assert c.last_kernels().startswith(prefix[form]), (form, c.last_kernels())
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (form, bad.tolist())
    finally:
        ls.close()


def case2(oracle):
    """6 nodes at the 128-bit set over 3 tables of m = 4."""
    if "case2" not in _CACHE:
        c, k = ctx_for(oracle, "128")
        sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
        g = rng(1302)
        pool = sk.encrypt_lwe_message(g.integers(0, 2, 5).astype(np.uint32), 4, seed0=2300)
        nodes = [((2 * i + 1) % 3, [(int(g.integers(0, 5)), int(g.integers(-2, 5))) for _ in range(1 + i % 3)],
                  (1 << 29) if i == 4 else 0) for i in range(6)]
        tables = tables_for(c.params, 4, 3)
        want = oracle_nodes(oracle, k.p, k.ck, pool, nodes, tables)
        _CACHE["case2"] = (pool, nodes, tables, want)
    return _CACHE["case2"]


def test_128_bit_set_and_a_flipped_selector(oracle):
    """The default 128-bit set: the latency form (auto) and the whole form, which is the fused assist
    form (gate waves read polynomial a of the item's table, loader waves polynomial b) plus the
    margin guard's recompute launch.  All 6 items equal the oracle; changing the last item's table
    changes exactly that item's words."""
    c, k = ctx_for(oracle, "128")
    pool, nodes, tables, want = case2(oracle)
    ls = tfhe_amd.LutSet(c, tables)
    try:
        prefix = {"auto": "k_blind_rotate_wide<3", "whole": "k_blind_rotate_assist<true,TV>"}
        for form in ("auto", "whole"):
            with c.options(br_form=form):
                got = c.lut_apply(ls, pool, nodes)
                assert c.last_kernels().startswith(prefix[form]), (form, c.last_kernels())
                assert np.array_equal(got, want), form
                flipped = nodes[:-1] + [((nodes[-1][0] + 1) % 3, nodes[-1][1], nodes[-1][2])]
                got2 = c.lut_apply(ls, pool, flipped)
            changed = np.flatnonzero((got2 != got).any(axis=1))
            assert changed.tolist() == [5], (form, changed.tolist())
            assert np.array_equal(got2[5], oracle_nodes(oracle, k.p, k.ck, pool, flipped, tables, only=[5])[5])
    finally:
        ls.close()


def test_tail_split_shifts_the_selectors(oracle):
    """128-bit, B = 4 x CUs + 3: the plan runs the full rounds in the whole form and the ragged tail
    in the latency form, whose launch reads the selectors from `full` on.  The items on both sides
    of the split and the last one use different tables and equal the oracle; the whole batch equals
    the same call forced to the whole form (one launch, no shift)."""
    import torch
    c, k = ctx_for(oracle, "128")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    full, B = 4 * cus, 4 * cus + 3
    pool, _, tables, _ = case2(oracle)
    g = rng(1303)
    lut = g.integers(0, 3, B)
    lut[[full - 1, full, full + 1, B - 1]] = [0, 1, 2, 0]  # neighbours across the split differ
    src, coef = g.integers(0, 5, B), g.integers(1, 4, B)
    nodes = [(int(lut[i]), [(int(src[i]), int(coef[i]))], 0) for i in range(B)]
    ls = tfhe_amd.LutSet(c, tables)
    try:
        got = c.lut_apply(ls, pool, nodes)
        assert c.last_kernels().startswith("k_blind_rotate_assist<true,TV>"), c.last_kernels()
        with c.options(br_form="whole"):
            whole = c.lut_apply(ls, pool, nodes)
    finally:
        ls.close()
    probe = [full - 1, full, full + 1, B - 1]
    want = oracle_nodes(oracle, k.p, k.ck, pool, nodes, tables, only=probe)
    for i in probe:
        assert np.array_equal(got[i], want[i]), i
    bad = np.flatnonzero((got != whole).any(axis=1))
    assert bad.size == 0, bad[:10].tolist()


def test_recompute_reads_the_items_table(oracle):
    """The margin guard's recompute launch carries the selector: under the crafted near-tie key
    (conftest.crafted_near_tie_case) and a set {random table, crafted test vector}, the
    crafted ciphertext selects table 1 and the others table 0.  Forced fused arithmetic flags the
    crafted item, the reference-tree recompute redoes it (near_tie_items rises), and every output is
    the oracle's reference-mode words for its own table.  The KSK is the seeded key's: the fused
    arithmetic parts from the reference in accumulator words other than a[0] and b[0] only
    (tests/test_margin_guard_cpu.py), and a zero KSK's key switch returns (0, ..., 0, b[0])."""
    from oracle import CloudKeyArrays
    p = get_keys(oracle, "128").p
    tv, bk, ct = crafted_near_tie_case(oracle, p)
    ksk = get_keys(oracle, "128").ck.ksk
    off = oracle.decomposition_offset(p)
    g = rng(1304)
    u32 = lambda *shape: g.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    tables = np.stack([u32(2 * p.N), tv])
    cts = np.concatenate([u32(2, p.n + 1), ct[None], u32(3, p.n + 1)])
    nodes = [(1 if i == 2 else 0, [(i, 1)], 0) for i in range(len(cts))]
    want = oracle_nodes(oracle, p, CloudKeyArrays(off, tv, ksk, bk), cts, nodes, tables)
    c = tfhe_amd.Context("128", 0)
    try:
        c.load_cloud_key(off, tv, bk, ksk)
        ls = tfhe_amd.LutSet(c, tables)
        before = c.near_tie_items()
        for form in ("auto", "whole"):
            with c.options(br_form=form, arith=tfhe_amd.ARITH_FUSED_FORCED):
                got = c.lut_apply(ls, cts, nodes)
                assert c.last_kernels().split(" + ")[0].endswith("fused)")
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (form, bad.tolist())
            assert c.near_tie_items() > before, form
            before = c.near_tie_items()
        ls.close()
    finally:
        c.close()


def random_dag(seed=1306, n_inputs=6, n_nodes=30, T=5):
    """A seeded DAG: 1-3 terms per node over the 6 most recent wires (so chains form), coefficients
    in {-2, ..., 4} without 0, a constant on every fifth node."""
    g = rng(seed)
    c = tfhe_amd.LutCircuit()
    for _ in range(n_inputs):
        c.input()
    for i in range(n_nodes):
        w = n_inputs + i
        lo = max(0, w - 6)
        terms = [(int(g.integers(lo, w)), int(g.choice([-2, -1, 1, 2, 3, 4]))) for _ in range(int(g.integers(1, 4)))]
        c.node(int(g.integers(0, T)), terms, const=int(g.integers(0, 16)) << 27 if i % 5 == 0 else 0)
    c.output(*range(n_inputs + n_nodes))  # every wire
    return c


def case6(oracle):
    if "case6" not in _CACHE:
        c, k = ctx_for(oracle, "uint4")
        sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
        circ = random_dag()
        inputs = sk.encrypt_lwe_message(rng(1307).integers(0, 4, circ.n_inputs).astype(np.uint32), 16, seed0=6300)
        tables = tables_for(c.params, 16, 5)
        levels, depth = circ.schedule()
        # the oracle's own composition, node by node in level order (a level's nodes in one call per table)
        wires = np.zeros((circ.n_inputs + len(circ.nodes), c.n1), np.uint32)
        wires[:circ.n_inputs] = inputs
        for lv in range(1, depth + 1):
            idx = np.flatnonzero(levels == lv)
            wires[circ.n_inputs + idx] = oracle_nodes(oracle, k.p, k.ck, wires, [circ.nodes[i] for i in idx], tables)
        _CACHE["case6"] = (circ, inputs, tables, wires, depth)
    return _CACHE["case6"]


def test_circuit_parity(oracle):
    """A random DAG of 30 nodes over 6 inputs and 5 tables, depth >= 4, every wire an output: all of
    them equal the oracle's composition.  Bit-exactness holds whether or not a node's message
    survives the noise, so nothing is decrypted here."""
    c, _ = ctx_for(oracle, "uint4")
    circ, inputs, tables, want, depth = case6(oracle)
    assert depth >= 4
    ls = tfhe_amd.LutSet(c, tables)
    try:
        got, ran = circ.run(c, ls, inputs)
    finally:
        ls.close()
    assert ran == depth
    assert np.array_equal(got[:circ.n_inputs], inputs)  # an output that is an input wire
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, bad.tolist()


def test_dev_variants(oracle):
    """tfhe_gpu_lut_apply_dev and tfhe_gpu_lut_circuit_eval_dev on torch tensors and torch's stream:
    the host-buffer calls' words (case 1's batch, the random DAG)."""
    import torch
    c, _ = ctx_for(oracle, "uint4")
    pool, nodes, tables, want = case1(oracle)
    circ, inputs, ctables, cwant, depth = case6(oracle)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")
    t_pool, t_in = dev(pool), dev(inputs)
    t_out = torch.zeros((len(nodes), c.n1), dtype=torch.int32, device="cuda:0")
    t_cout = torch.zeros((len(circ.outputs), c.n1), dtype=torch.int32, device="cuda:0")
    ls, cls = tfhe_amd.LutSet(c, tables), tfhe_amd.LutSet(c, ctables)
    try:
        host = c.lut_apply(ls, pool, nodes)
        chost, _ = circ.run(c, cls, inputs)
        try:
            c.set_stream(torch.cuda.current_stream().cuda_stream)
            c.lut_apply_dev(ls, t_pool.data_ptr(), pool.shape[0], nodes, t_out.data_ptr())
            ran = circ.run_dev(c, cls, t_in.data_ptr(), t_cout.data_ptr())
            c.sync()
        finally:
            c.set_stream(None)
    finally:
        ls.close()
        cls.close()
    assert ran == depth
    assert np.array_equal(t_out.cpu().numpy().view(np.uint32), host) and np.array_equal(host, want)
    assert np.array_equal(t_cout.cpu().numpy().view(np.uint32), chost) and np.array_equal(chost, cwant)


ADD_PAIRS = [(0xB7, 0x5E), (0xFF, 0xFF), (0, 0), (0xFF, 1)]


def test_radix_adder_decrypts(oracle):
    """16 additions of 8-bit numbers as four base-4 digits (UINT4, m = 16: 2 message bits, 2 bits
    of carry room) in ONE circuit run: 128 nodes at depth 4.  Digit i of pair q is encrypted with
    seed 100 q + i for a and 100 q + 50 + i for b.  All 16 sums decrypt correctly, no allowance:
    the three-term sum of bootstrap outputs has phase error std 1.35e-3 against a half slot of
    1/64 = 1.56e-2 (measured on the oracle).  8 nodes are compared bit-exact with the oracle."""
    c, k = ctx_for(oracle, "uint4")
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    g = rng(7)
    pairs = ADD_PAIRS + [tuple(int(v) for v in g.integers(0, 256, 2)) for _ in range(12)]
    tables = np.array([tfhe_amd.lut_generate(c.params, 16, lambda x: x % 4),
                       tfhe_amd.lut_generate(c.params, 16, lambda x: x // 4)])
    circ = tfhe_amd.LutCircuit()
    ins = [[circ.input() for _ in range(8)] for _ in pairs]  # a's digits, then b's, LSB first
    sums = [circ.radix_add(w[:4], w[4:], msg_lut=0, carry_lut=1) for w in ins]
    circ.output(*range(circ.n_inputs + len(circ.nodes)))  # every wire: the sums are picked below
    digits = lambda v: np.array([(v >> (2 * i)) & 3 for i in range(4)], np.uint32)
    inputs = np.concatenate([np.concatenate([sk.encrypt_lwe_message(digits(a), 16, seed0=100 * q),
                                             sk.encrypt_lwe_message(digits(b), 16, seed0=100 * q + 50)])
                             for q, (a, b) in enumerate(pairs)])
    levels, depth = circ.schedule()
    assert len(circ.nodes) == 128 and depth == 4
    ls = tfhe_amd.LutSet(c, tables)
    try:
        wires, ran = circ.run(c, ls, inputs)
    finally:
        ls.close()
    assert ran == 4
    got = [sum(int(d) << (2 * i) for i, d in enumerate(sk.decrypt_lwe_message(wires[s], 16))) for s in sums]
    assert got == [a + b for a, b in pairs], [(hex(a), hex(b), hex(s)) for (a, b), s in zip(pairs, got)]
    # 8 nodes, two of every level, against the oracle over the device's own earlier wires
    probe = np.concatenate([np.flatnonzero(levels == lv)[[1, -2]] for lv in range(1, 5)])
    want = oracle_nodes(oracle, k.p, k.ck, wires, circ.nodes, tables, only=probe)
    for i in probe:
        assert np.array_equal(wires[circ.n_inputs + i], want[i]), int(i)


def test_errors_leave_the_context_usable(oracle):
    """Descriptor and context errors return their status before any launch, and a valid call
    afterwards still gives the oracle's words."""
    import torch
    c, _ = ctx_for(oracle, "uint4")
    pool, nodes, tables, want = case1(oracle)
    T, P = len(tables), len(pool)
    ls = tfhe_amd.LutSet(c, tables)
    other = tfhe_amd.Context("uint4", 0)  # no key, and a set of its own
    multi = tfhe_amd.Context.multi("uint4", devices=[0, 0])
    try:
        ls_other = tfhe_amd.LutSet(other, tables)
        ls_multi = tfhe_amd.LutSet(multi, tables)

        def status(call):
            with pytest.raises(tfhe_amd.TfheError) as e:
                call()
            return e.value.status

        bad_lut = nodes[:4] + [(T, nodes[4][1], 0)] + nodes[5:]
        bad_src = nodes[:7] + [(0, [(0, 1), (P, 1)], 0)] + nodes[8:]
        assert status(lambda: c.lut_apply(ls, pool, bad_lut)) == tfhe_amd.ERR_INVALID
        assert status(lambda: c.lut_apply(ls, pool, bad_src)) == tfhe_amd.ERR_INVALID
        assert status(lambda: c.lut_apply(ls_other, pool, nodes)) == tfhe_amd.ERR_INVALID  # another context's set
        assert status(lambda: other.lut_apply(ls_other, pool, nodes)) == tfhe_amd.ERR_NO_KEY
        circ = tfhe_amd.LutCircuit()
        a = circ.input()
        circ.output(circ.node(T, [(a, 1)]))
        assert status(lambda: circ.run(c, ls, pool[:1])) == tfhe_amd.ERR_INVALID
        t = torch.zeros((len(nodes), c.n1), dtype=torch.int32, device="cuda:0")
        assert status(lambda: multi.lut_apply_dev(ls_multi, t.data_ptr(), P, nodes, t.data_ptr())) == tfhe_amd.ERR_INVALID
        ok = tfhe_amd.LutCircuit()
        a = ok.input()
        ok.output(ok.node(0, [(a, 1)]))
        assert status(lambda: ok.run_dev(multi, ls_multi, t.data_ptr(), t.data_ptr())) == tfhe_amd.ERR_INVALID
        # empty calls are no-ops
        assert c.lut_apply(ls, pool, []).shape == (0, c.n1)
        # and the context still works
        assert np.array_equal(c.lut_apply(ls, pool, nodes), want)
        ls_other.close()
        ls_multi.close()
    finally:
        ls.close()
        other.close()
        multi.close()
