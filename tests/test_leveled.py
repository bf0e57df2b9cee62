"""GPU tests of the leveled operations (CMUX, TRGSW selector sets, table lookup
by a CMUX tree, sample extraction, TRLWE / TRGSW encryption): every result
bit-exact (np.array_equal; +0.0 == -0.0 for the f64 spectra) against the CPU
oracle's restatement of the reference on the same seeded inputs."""
import ctypes as C

import numpy as np
import pytest

import tfhe_amd
from conftest import get_keys, rng

pytestmark = pytest.mark.gpu
u32p = C.POINTER(C.c_uint32)


def u32rand(g, *shape):
    return g.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


_ENV = {}


class Env:
    """A context without a cloud key, the oracle's secret key (seed 42) and three selectors
    (encryptions of 0, 1 and 1, seeds 900..902) from the oracle, resident as a TrgswSet."""

    def __init__(self, oracle, pname):
        from oracle import params
        self.p = params(pname)
        self.tp = tfhe_amd.make_params(pname)
        self.k0, self.k1 = oracle.secret_key(self.p, 42)
        self.off = oracle.decomposition_offset(self.p)
        self.ctx = tfhe_amd.Context(pname, 0)
        self.sel_bits = [0, 1, 1]
        self.trgsw = np.array([oracle.trgsw_encrypt_torus_fft(self.p, mu, self.p.alpha_bsk, self.k1, 900 + s)
                               for s, mu in enumerate(self.sel_bits)])
        self.set = tfhe_amd.TrgswSet(self.ctx, self.trgsw)


def env(oracle, pname):
    if pname not in _ENV:
        _ENV[pname] = Env(oracle, pname)
    return _ENV[pname]


def oracle_lookup(oracle, e, table, addr_row):
    """The CMUX tree level by level with oracle.cmux: level j pairs entries 2i, 2i + 1 under address bit j."""
    cur = [t for t in table]
    for j, s in enumerate(addr_row):
        cur = [oracle.cmux(e.p, cur[2 * i], cur[2 * i + 1], e.trgsw[s], e.off) for i in range(len(cur) // 2)]
    assert len(cur) == 1
    return cur[0]


# ---- TRLWE / TRGSW encryption (trlwe.zig:30-98, trgsw.zig:35-91) ------------
@pytest.mark.parametrize("pname", ["128", "uint4"])
def test_trlwe_encrypt_decrypt_match_oracle(oracle, pname):
    e = env(oracle, pname)
    g = rng(11)
    bits = g.integers(0, 2, (3, e.p.N)).astype(bool)
    mu = np.where(bits, 0.125, -0.125)
    got = e.ctx.trlwe_encrypt(e.k1, mu, alpha=e.p.alpha_lv1, seed0=700)
    want = np.array([oracle.trlwe_encrypt_f64(e.p, mu[i], e.p.alpha_lv1, e.k1, 700 + i) for i in range(3)])
    assert np.array_equal(got, want)
    dec = e.ctx.trlwe_decrypt_bool(e.k1, got)
    assert np.array_equal(dec, np.array([oracle.trlwe_decrypt_bool(e.p, ct, e.k1) for ct in want]))
    assert np.array_equal(dec, bits)
    # decryption of words that are no encryption of anything: still the oracle's bits
    junk = u32rand(g, 2, 2 * e.p.N)
    assert np.array_equal(e.ctx.trlwe_decrypt_bool(e.k1, junk),
                          np.array([oracle.trlwe_decrypt_bool(e.p, ct, e.k1) for ct in junk]))


@pytest.mark.parametrize("pname", ["128", "uint4"])
def test_trgsw_encrypt_matches_oracle(oracle, pname):
    e = env(oracle, pname)
    got = e.ctx.trgsw_encrypt(e.k1, [0, 1], alpha=e.p.alpha_bsk, seed0=900)
    assert got.shape == (2, 2 * e.p.L, 2, e.p.N)
    assert np.array_equal(got, e.trgsw[:2])


# ---- CMUX (trgsw.zig:260-284) -------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 9])
@pytest.mark.parametrize("pname", ["128", "uint4"])
def test_cmux_matches_oracle(oracle, pname, B):
    e = env(oracle, pname)
    g = rng(20 + B)
    in0, in1 = u32rand(g, B, 2 * e.p.N), u32rand(g, B, 2 * e.p.N)
    sel = np.array([(2 * i + 1) % 3 for i in range(B)], np.uint32)  # 1, 0, 2, 1, ...: mixed order
    got = e.ctx.cmux(e.set, sel, in0, in1)
    assert e.ctx.last_kernels() == f"k_cmux<{e.p.L}>"
    for i in range(B):
        assert np.array_equal(got[i], oracle.cmux(e.p, in0[i], in1[i], e.trgsw[sel[i]], e.off)), i


def test_cmux_selects(oracle):
    """Semantics on real ciphertexts: the selector's bit picks in1 (1) or in0 (0)."""
    e = env(oracle, "128")
    g = rng(5)
    bits = g.integers(0, 2, (2, e.p.N)).astype(bool)
    cts = e.ctx.trlwe_encrypt(e.k1, np.where(bits, 0.125, -0.125), seed0=40)
    out = e.ctx.cmux(e.set, [0, 1, 2], [cts[0]] * 3, [cts[1]] * 3)
    dec = e.ctx.trlwe_decrypt_bool(e.k1, out)
    for i, s in enumerate(e.sel_bits):
        assert np.array_equal(dec[i], bits[s])


def test_cmux_large_batch_and_ragged_tail(oracle):
    """B = 1030: more than 256 workgroups of 4 items plus a ragged tail of 2.  With in1 == in0 the
    digits of the bare decomposition offset are all zero, so out == in0 exactly; three items of a
    non-degenerate run against the oracle."""
    e = env(oracle, "128")
    g = rng(31)
    B = 1030
    in0 = u32rand(g, B, 2 * e.p.N)
    sel = (np.arange(B) % 3).astype(np.uint32)
    assert np.array_equal(e.ctx.cmux(e.set, sel, in0, in0), in0)
    in1 = u32rand(g, B, 2 * e.p.N)
    got = e.ctx.cmux(e.set, sel, in0, in1)
    for i in (0, 515, 1029):
        assert np.array_equal(got[i], oracle.cmux(e.p, in0[i], in1[i], e.trgsw[sel[i]], e.off)), i


# ---- table lookup ---------------------------------------------------------------
def lookup_addresses(k, Q, g):
    """Q addresses with 0, 2^k - 1 and a repeat among them, as (Q, k) selector indices: bit value 0 ->
    selector 0, bit value 1 -> selector 1 or 2 (both encrypt 1)."""
    vals = [0, (1 << k) - 1, 0] + [int(v) for v in g.integers(0, 1 << k, max(Q - 3, 0))]
    vals = vals[:Q]
    addr = np.array([[((v >> j) & 1) * (1 + (j + q) % 2) for j in range(k)] for q, v in enumerate(vals)], np.uint32)
    return vals, addr


FORMS = [(tfhe_amd.CMUX_AUTO, "auto"), (tfhe_amd.CMUX_PER_WAVE, "wave"), (tfhe_amd.CMUX_SHARED, "shared")]


def expected_kernels(form, k, L):
    """Level j has 2^(k-1-j) pairs per query; the workgroup form (auto's choice too) takes the levels with >= 4."""
    first = "k_cmux_shared" if form != tfhe_amd.CMUX_PER_WAVE and (1 << (k - 1)) >= 4 else "k_cmux"
    return f"{first}<{L}>" + (f" + k_cmux<{L}>" if first != "k_cmux" else "")


@pytest.mark.parametrize("form", [f for f, _ in FORMS], ids=[n for _, n in FORMS])
@pytest.mark.parametrize("k,Q", [(1, 3), (3, 5), (5, 2)])
@pytest.mark.parametrize("pname", ["128", "uint4"])
def test_table_lookup_matches_oracle_tree(oracle, pname, k, Q, form):
    e = env(oracle, pname)
    g = rng(100 + k)
    table = u32rand(g, 1 << k, 2 * e.p.N)
    _, addr = lookup_addresses(k, Q, g)
    with e.ctx.options(cmux_form=form):
        got = e.ctx.table_lookup(e.set, addr, table)
        assert e.ctx.last_kernels() == expected_kernels(form, k, e.p.L)
    for q in range(Q):
        assert np.array_equal(got[q], oracle_lookup(oracle, e, table, addr[q])), q


def test_table_lookup_forms_agree(oracle):
    e = env(oracle, "128")
    g = rng(7)
    table = u32rand(g, 32, 2 * e.p.N)
    _, addr = lookup_addresses(5, 6, g)
    outs = []
    for form in (tfhe_amd.CMUX_AUTO, tfhe_amd.CMUX_PER_WAVE, tfhe_amd.CMUX_SHARED):
        with e.ctx.options(cmux_form=form):
            outs.append(e.ctx.table_lookup(e.set, addr, table))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2])


@pytest.mark.parametrize("pname", ["128", "80", "uint4"])
def test_table_lookup_returns_the_addressed_entry(oracle, pname):
    """k = 3, all 8 addresses, a pack_bits table: decrypting the output gives the entry's bits."""
    e = env(oracle, pname)
    values = np.array([0xA5, 0x3C, 0xFF, 0x00, 0x81, 0x7E, 0x12, 0xC9], np.uint64)
    table = tfhe_amd.lookup_table_pack_bits(e.tp, values, 8)
    addr = np.array([[((v >> j) & 1) * (1 + j % 2) for j in range(3)] for v in range(8)], np.uint32)
    out = e.ctx.table_lookup(e.set, addr, table)
    dec = e.ctx.trlwe_decrypt_bool(e.k1, out)
    for v in range(8):
        assert tfhe_amd.bit_utils.convert(dec[v][:8]) == int(values[v]), v


_REF = {}


def address_rows(vals, k):
    """(Q, k) selector indices of the addresses vals: bit value 0 -> selector 0, 1 -> selector 1 or 2."""
    return np.array([[((v >> j) & 1) * (1 + (j + q) % 2) for j in range(k)] for q, v in enumerate(vals)], np.uint32)


def test_table_lookup_second_chunk_at_the_maximum_k(oracle):
    """k = 12 (LOOKUP_MAX_K), Q = 17 at UINT4: table_lookup_on takes 16 queries per chunk at k = 12
    (2,048 level-0 pairs of 8 KB per query against the scratch cap), so query 16 runs alone in a
    second chunk, with the selector offsets sel_at[j] + 16 cnt, index tables sized for the chunk and
    the ping-pong buffers reused.  Queries 0, 15 and 16 address 0x000, 0xFFF and 0x5A5: 0 and 15
    differ in every bit, and 16 differs from 0 in six bits and from 15 in the other six, so a second
    chunk that re-read the first chunk's selectors (or its last query's) cannot pass.  The oracle's
    CMUX tree on those three; all 17 outputs equal between the per-wave, workgroup and auto forms,
    and again through tfhe_gpu_table_lookup_dev into a sentinel-filled buffer."""
    import torch
    e = env(oracle, "uint4")
    k, Q = 12, 17
    g = rng(1217)
    table = u32rand(g, 1 << k, 2 * e.p.N)
    vals = [0x000] + [int(v) for v in g.integers(0, 1 << k, 14)] + [0xFFF, 0x5A5]
    assert len(vals) == Q and vals[0] ^ vals[15] == 0xFFF and vals[16] != vals[0] and vals[16] != vals[15]
    addr = address_rows(vals, k)
    outs = {}
    for form, name in FORMS:
        with e.ctx.options(cmux_form=form):
            outs[name] = e.ctx.table_lookup(e.set, addr, table)
            assert e.ctx.last_kernels() == expected_kernels(form, k, e.p.L)
    for q in (0, 15, 16):
        want = oracle_lookup(oracle, e, table, addr[q])
        for name, got in outs.items():
            assert np.array_equal(got[q], want), (name, q)
    for name in ("wave", "shared"):
        bad = np.flatnonzero((outs[name] != outs["auto"]).any(axis=1))
        assert bad.size == 0, (name, bad.tolist())
    SENTINEL = 0x5EA1AB1E
    t_table = to_dev(table)
    t_out = torch.full((Q, 2 * e.p.N), SENTINEL, dtype=torch.int32, device="cuda:0")
    try:
        e.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        e.ctx.table_lookup_dev(e.set, addr, t_table.data_ptr(), t_out.data_ptr())
        e.ctx.sync()
    finally:
        e.ctx.set_stream(None)
    got = from_dev(t_out)
    # every row overwritten: 2,048 uniform words equal the sentinel with probability 2^-21 per row
    assert ((got != SENTINEL).sum(axis=1) > 2000).all()
    assert np.array_equal(got, outs["auto"])


@pytest.mark.parametrize("form", [f for f, _ in FORMS], ids=[n for _, n in FORMS])
def test_table_lookup_mid_range_k(oracle, form):
    """k = 8, Q = 3 at the 128-bit set (between the k <= 5 cases and LOOKUP_MAX_K): the oracle's tree
    (255 CMUXes) on query 2, whose address 0xB6 mixes the bits."""
    e = env(oracle, "128")
    k = 8
    table = u32rand(rng(108), 1 << k, 2 * e.p.N)
    addr = address_rows([0x00, 0xFF, 0xB6], k)
    with e.ctx.options(cmux_form=form):
        got = e.ctx.table_lookup(e.set, addr, table)
        assert e.ctx.last_kernels() == expected_kernels(form, k, e.p.L)
    if "k8" not in _REF:
        _REF["k8"] = oracle_lookup(oracle, e, table, addr[2])
    assert np.array_equal(got[2], _REF["k8"])


# ---- sample extraction (trlwe.zig:146-162) ---------------------------------------
COEF = [0, 1, 7, 1023]


def test_sample_extract_matches_oracle(oracle):
    e = env(oracle, "128")
    x = u32rand(rng(41), 3, 2 * e.p.N)
    got = e.ctx.sample_extract(x, COEF)
    assert got.shape == (3, 4, e.p.N + 1)
    for b in range(3):
        for c, kk in enumerate(COEF):
            assert np.array_equal(got[b, c], oracle.sample_extract_index(x[b], kk)), (b, kk)


@pytest.fixture(scope="module")
def keyed80(oracle):
    k = get_keys(oracle, "80")
    c = tfhe_amd.Context("80", 0)
    c.load_cloud_key(k.ck.offset, k.ck.testvec, k.ck.bk, k.ck.ksk)
    yield c, k
    c.close()


def test_sample_extract_with_key_switch_matches_oracle(oracle, keyed80):
    c, k = keyed80
    x = u32rand(rng(42), 3, 2 * k.p.N)
    got = c.sample_extract(x, COEF, key_switch=True)
    assert got.shape == (3, 4, k.p.n + 1)
    for b in range(3):
        for ci, kk in enumerate(COEF):
            want = oracle.identity_key_switch(k.p, oracle.sample_extract_index(x[b], kk), k.ck.ksk)
            assert np.array_equal(got[b, ci], want), (b, kk)


# ---- end to end: lookup -> extract + key switch -> gates ---------------------------
def test_lookup_outputs_are_gate_inputs(oracle, keyed80):
    c, k = keyed80
    tp = tfhe_amd.make_params("80")
    sk = tfhe_amd.SecretKey(tp, k.k0, k.k1)
    values = np.array([0x5A, 0xC3, 0x0F, 0xF0, 0x99, 0x66, 0x01, 0xFE], np.uint64)
    table = tfhe_amd.lookup_table_pack_bits(tp, values, 8)
    queries = [6, 0, 7, 3]
    # one selector per address bit of every query, encrypted on the device
    bits = np.array([[(v >> j) & 1 for j in range(3)] for v in queries], np.uint32)
    sels = tfhe_amd.TrgswSet(c, c.trgsw_encrypt(k.k1, bits.reshape(-1), alpha=k.p.alpha_bsk, seed0=5000))
    addr = np.arange(bits.size, dtype=np.uint32).reshape(bits.shape)
    out = c.table_lookup(sels, addr, table)
    lv0 = c.sample_extract(out, np.arange(8), key_switch=True)
    for q, v in enumerate(queries):
        assert tfhe_amd.bit_utils.convert(sk.decrypt_bool(lv0[q])) == int(values[v]), q
    # the outputs are ordinary TLWELv0: AND with fresh encryptions of 1 and of 0
    fresh = sk.encrypt_bool([1, 0], seed0=77)
    gates = tfhe_amd.Gates(c)
    bit0 = bool(values[queries[0]] >> 1 & 1)  # coefficient 1 of query 0's output
    assert sk.decrypt_bool(gates.and_gate(lv0[0, 1], fresh[0]))[0] == bit0
    assert not sk.decrypt_bool(gates.and_gate(lv0[0, 1], fresh[1]))[0]
    sels.close()


def test_encrypted_sbox_example():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("encrypted_sbox", os.path.join(ROOT, "examples", "encrypted_sbox.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main(["--queries", "2"]) == 0


# ---- device-pointer forms --------------------------------------------------------
def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def from_dev(t):
    return t.cpu().numpy().view(np.uint32)


def test_dev_forms_equal_host_forms(oracle, keyed80):
    import torch
    c, k = keyed80
    e = env(oracle, "80")
    sels = tfhe_amd.TrgswSet(c, e.trgsw)
    g = rng(61)
    N2 = 2 * k.p.N
    in0, in1 = u32rand(g, 6, N2), u32rand(g, 6, N2)
    sel = np.array([2, 0, 1, 1, 0, 2], np.uint32)
    table = u32rand(g, 8, N2)
    _, addr = lookup_addresses(3, 4, g)
    want_cmux = c.cmux(sels, sel, in0, in1)
    want_lk = c.table_lookup(sels, addr, table)
    want_lv1 = c.sample_extract(want_lk, COEF)
    want_lv0 = c.sample_extract(want_lk, COEF, key_switch=True)
    t0, t1, tt = to_dev(in0), to_dev(in1), to_dev(table)
    o_cmux = torch.full((6, N2), -1, dtype=torch.int32, device="cuda:0")
    o_lk = torch.full((4, N2), -1, dtype=torch.int32, device="cuda:0")
    o_lv1 = torch.full((4 * 4, k.p.N + 1), -1, dtype=torch.int32, device="cuda:0")
    o_lv0 = torch.full((4 * 4, k.p.n + 1), -1, dtype=torch.int32, device="cuda:0")
    try:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.cmux_dev(sels, sel, t0.data_ptr(), t1.data_ptr(), o_cmux.data_ptr())
        c.table_lookup_dev(sels, addr, tt.data_ptr(), o_lk.data_ptr())
        c.sample_extract_dev(o_lk.data_ptr(), 4, COEF, o_lv1.data_ptr())
        c.sample_extract_dev(o_lk.data_ptr(), 4, COEF, o_lv0.data_ptr(), key_switch=True)
        c.sync()
    finally:
        c.set_stream(None)
    assert np.array_equal(from_dev(o_cmux), want_cmux)
    assert np.array_equal(from_dev(o_lk), want_lk)
    assert np.array_equal(from_dev(o_lv1).reshape(want_lv1.shape), want_lv1)
    assert np.array_equal(from_dev(o_lv0).reshape(want_lv0.shape), want_lv0)
    sels.close()


# ---- host staging ------------------------------------------------------------------
def test_host_staging_modes_same_words_leveled(oracle):
    """TFHE_OPT_HOST_STAGING on the leveled host entry points: pinned staging and pageable copies
    return the same words for cmux (B = 5: one full workgroup and a tail of 1), table_lookup
    (k = 3, Q = 2), rotate_by_bits (h = 2, B = 2) and sample_extract (2 coefficients of 2 TRLWEs,
    no key switch), the smallest shapes that pass through every staged input and output.  Each
    call runs twice under pinned staging, so the arena is reused from offset 0."""
    e = env(oracle, "uint4")
    g = rng(71)
    N2 = 2 * e.p.N
    in0, in1, table, x = u32rand(g, 5, N2), u32rand(g, 5, N2), u32rand(g, 8, N2), u32rand(g, 2, N2)
    sel = np.array([1, 0, 2, 1, 0], np.uint32)
    _, addr = lookup_addresses(3, 2, g)
    calls = {
        "cmux": lambda: e.ctx.cmux(e.set, sel, in0, in1),
        "table_lookup": lambda: e.ctx.table_lookup(e.set, addr, table),
        "rotate_by_bits": lambda: e.ctx.rotate_by_bits(e.set, [[1, 0], [0, 2]], [1, e.p.N + 3], x),
        "sample_extract": lambda: e.ctx.sample_extract(x, [0, e.p.N - 1]),
    }
    assert e.ctx.get_option("host_staging") == tfhe_amd.STAGING_PAGEABLE
    want = {name: f() for name, f in calls.items()}
    with e.ctx.options(host_staging=tfhe_amd.STAGING_PINNED):
        for name, f in calls.items():
            for rep in range(2):
                assert np.array_equal(f(), want[name]), (name, rep)
    assert e.ctx.get_option("host_staging") == tfhe_amd.STAGING_PAGEABLE
    for name, f in calls.items():  # and back: pageable copies after the arena was in use
        assert np.array_equal(f(), want[name]), name
    # the pageable words are the oracle's, so a staging bug cannot hide in a shared reference
    assert np.array_equal(want["cmux"][4], oracle.cmux(e.p, in0[4], in1[4], e.trgsw[sel[4]], e.off))
    assert np.array_equal(want["table_lookup"][1], oracle_lookup(oracle, e, table, addr[1]))
    assert np.array_equal(want["sample_extract"][1, 1], oracle.sample_extract_index(x[1], e.p.N - 1))


# ---- argument checks (no launch follows a refused call) -----------------------------
def test_error_returns(oracle, keyed80):
    e = env(oracle, "128")
    lib, h, s = e.ctx.lib, e.ctx.h, e.set.h
    N2 = 2 * e.p.N
    x = np.zeros((4, N2), np.uint32)
    xp = x.ctypes.data_as(u32p)
    one = np.array([0, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.uint32)
    op = one.ctypes.data_as(u32p)
    INV, NOKEY = tfhe_amd.ERR_INVALID, tfhe_amd.ERR_NO_KEY
    # null arguments
    assert lib.tfhe_gpu_cmux_batch(h, None, op, xp, xp, xp, 1) == INV
    assert lib.tfhe_gpu_cmux_batch(h, s, None, xp, xp, xp, 1) == INV
    assert lib.tfhe_gpu_cmux_batch(h, s, op, None, xp, xp, 1) == INV
    assert lib.tfhe_gpu_cmux_batch_dev(h, s, op, None, None, None, 1) == INV
    assert lib.tfhe_gpu_table_lookup_batch(h, s, op, 1, None, xp, 1) == INV
    assert lib.tfhe_gpu_table_lookup_batch(h, s, None, 1, xp, xp, 1) == INV
    assert lib.tfhe_gpu_table_lookup_dev(h, None, op, 1, None, None, 1) == INV
    assert lib.tfhe_gpu_sample_extract_batch(h, None, op, 1, 0, xp, 1) == INV
    assert lib.tfhe_gpu_sample_extract_batch(h, xp, None, 1, 0, xp, 1) == INV
    assert lib.tfhe_gpu_trlwe_encrypt_batch(h, None, None, 0.0, 1, xp, 1) == INV
    assert lib.tfhe_gpu_trlwe_decrypt_bool_batch(h, xp, None, None, 1) == INV
    assert lib.tfhe_gpu_trgsw_encrypt_batch(h, xp, None, 0.0, 1, None, 1) == INV
    out = C.c_void_p()
    assert lib.tfhe_gpu_trgsw_set_load(h, None, 1, C.byref(out)) == INV and not out.value
    assert lib.tfhe_gpu_trgsw_set_load(h, e.trgsw.ctypes.data_as(C.POINTER(C.c_double)), 0, C.byref(out)) == INV
    # selector / address index >= S (S = 3)
    bad = np.array([0, 3], np.uint32)
    assert lib.tfhe_gpu_cmux_batch(h, s, bad.ctypes.data_as(u32p), xp, xp, xp, 2) == INV
    assert lib.tfhe_gpu_table_lookup_batch(h, s, bad.ctypes.data_as(u32p), 2, xp, xp, 1) == INV
    assert b"set's size" in lib.tfhe_gpu_last_error(h)
    # k outside 1..12
    assert lib.tfhe_gpu_table_lookup_batch(h, s, op, 0, xp, xp, 1) == INV
    assert lib.tfhe_gpu_table_lookup_batch(h, s, op, 13, xp, xp, 1) == INV
    assert lib.tfhe_gpu_table_lookup_dev(h, s, op, 13, xp, xp, 1) == INV
    # coefficient index >= N
    n_bad = np.array([0, 1024], np.uint32)
    assert lib.tfhe_gpu_sample_extract_batch(h, xp, n_bad.ctypes.data_as(u32p), 2, 0, xp, 1) == INV
    # a set of another context / parameter set
    c80, _ = keyed80
    assert lib.tfhe_gpu_cmux_batch(c80.h, s, op, xp, xp, xp, 1) == INV
    assert lib.tfhe_gpu_table_lookup_batch(c80.h, s, op, 1, xp, xp, 1) == INV
    assert b"another context" in lib.tfhe_gpu_last_error(c80.h)
    # the key switch after an extraction needs a cloud key; the plain extraction does not
    assert lib.tfhe_gpu_sample_extract_batch(h, xp, op, 1, 1, xp, 1) == NOKEY
    assert lib.tfhe_gpu_sample_extract_batch(h, xp, op, 1, 0, xp, 1) == 0
    # empty batches are fine
    assert lib.tfhe_gpu_cmux_batch(h, s, None, None, None, None, 0) == 0
    assert lib.tfhe_gpu_table_lookup_batch(h, s, None, 3, xp, None, 0) == 0
    assert lib.tfhe_gpu_sample_extract_batch(h, None, op, 1, 0, None, 0) == 0
    assert lib.tfhe_gpu_trlwe_encrypt_batch(h, xp, None, 0.0, 1, None, 0) == 0
    # the form option takes 0..2
    with pytest.raises(tfhe_amd.TfheError):
        e.ctx.set_option("cmux_form", 3)
    assert e.ctx.get_option("cmux_form") == 0
