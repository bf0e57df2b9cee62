"""GPU tests of the packing key switch (TLWELv0 -> coefficient slots of a TRLWELv1): key generation against the
oracle's TRLWE encryption, the pack call word for word (np.array_equal) against the numpy restatement of its
definition (tests/test_pack_cpu.py), the device-pointer variant, chunking, the real 128-bit set through
gates -> pack -> packed lookup -> extraction -> decryption, a LUT-message slot, and the refusals."""
import numpy as np
import pytest

import tfhe_amd
from conftest import rng
from test_pack_cpu import SHAPES, edge_inputs, oracle_packing_key, oracle_params, pack_ref, random_coef, trlwe_phase, u32rand

pytestmark = pytest.mark.gpu

_ENV = {}


class Env:
    """A context without a cloud key at one of the small shapes, a secret key (seed 42) and the packing key of
    tfhe_gpu_packing_key_gen (seed0 7000, alpha_lv1): its host rows, and resident."""

    def __init__(self, shape):
        pd, self.basebit, self.t = SHAPES[shape]
        self.pd = pd
        self.ctx = tfhe_amd.Context(pd, 0)
        self.p = self.ctx.params
        self.sk = tfhe_amd.secret_key_new(self.p, 42)
        self.rows, _, _ = tfhe_amd.PackingKey.generate_rows(self.ctx, self.sk, 7000, basebit=self.basebit, t=self.t)
        self.key = tfhe_amd.PackingKey(self.ctx, self.rows, self.basebit, self.t)

    def ref(self, cts, coef):
        return pack_ref(self.p.n, self.p.N, self.rows, self.basebit, self.t, cts, coef)


def env(shape):
    if shape not in _ENV:
        _ENV[shape] = Env(shape)
    return _ENV[shape]


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def from_dev(t):
    return t.cpu().numpy().view(np.uint32)


# ---- 1. key generation ---------------------------------------------------------------------------
def test_packing_key_gen_matches_oracle(oracle):
    """n = 20, (2, 8): every k >= 1 row is oracle.trlwe_encrypt_f64 of k key_lv0[i] / 2^((j+1) basebit) at
    coefficient 0 with DefaultPrng(seed0 + idx), every k = 0 row is zero."""
    e = env("n20-2x8")
    op = oracle_params(e.pd)
    k0, k1 = oracle.secret_key(op, 42)
    assert np.array_equal(k0, e.sk.key_lv0) and np.array_equal(k1, e.sk.key_lv1)
    want = oracle_packing_key(oracle, op, k0, k1, e.basebit, e.t, 7000, op.alpha_lv1)
    assert e.rows.shape == want.shape == (20 * 8 * 4, 2048)
    assert not e.rows[0::4].any()
    assert np.array_equal(e.rows, want)


# ---- 2. pack against the restatement -------------------------------------------------------------
# n = 20 (2, 8): 3 coefficient blocks of 8, the last half padding; n = 36 (2, 7): 5 blocks, so the 3-slot LDS ring
# wraps; n = 18 (5, 3): blocks of 4, the last half padding.  2 * 300 = 600 items cross the 512-item workgroup;
# 1 * 1024 fills every slot with coef a permutation of 0 .. N - 1.
@pytest.mark.parametrize("B,C_", [(1, 1), (1, 3), (2, 300), (1, 1024)])
@pytest.mark.parametrize("shape", ["n20-2x8", "n36-2x7", "n18-5x3"])
def test_pack_matches_restatement(shape, B, C_):
    e = env(shape)
    g = rng(800 + C_)
    cts = u32rand(g, B, C_, e.p.n + 1)
    coef = random_coef(g, e.p.N, C_)
    if C_ == 1024:
        assert sorted(coef.tolist()) == list(range(1024))
    got = e.ctx.pack_tlwe(e.key, cts, coef)
    assert np.array_equal(got, e.ref(cts, coef))
    bb, tt = e.basebit, e.t
    assert e.ctx.last_kernels() == f"k_key_switch_gemm<{tt},{bb}> + k_pack_rotate_acc"


@pytest.mark.parametrize("shape", ["n20-2x8", "n36-2x7", "n18-5x3"])
def test_pack_edge_digits(shape):
    e = env(shape)
    g = rng(811)
    cts = edge_inputs(g, e.p.n, e.basebit, e.t)
    coef = np.array([e.p.N - 1, 0, 513, 7], np.uint32)
    assert np.array_equal(e.ctx.pack_tlwe(e.key, cts, coef), e.ref(cts, coef))


# ---- 3. device pointers --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["n20-2x8", "n18-5x3"])
def test_pack_dev_matches_host_call(shape):
    """tfhe_gpu_pack_tlwe_dev: the host-buffer call's words, with the input tensor of exactly B * C * (n + 1) words
    (the GEMM's whole-block reads past the last row are served from the library's own staging) and the output a
    torch tensor."""
    import torch
    e = env(shape)
    g = rng(820)
    B, C_ = 2, 77
    cts = u32rand(g, B, C_, e.p.n + 1)
    coef = random_coef(g, e.p.N, C_)
    want = e.ctx.pack_tlwe(e.key, cts, coef)
    x = to_dev(cts.reshape(-1))
    assert x.numel() == B * C_ * (e.p.n + 1)
    out = torch.full((B, 2 * e.p.N), -1, dtype=torch.int32, device="cuda:0")
    e.ctx.pack_tlwe_dev(e.key, x.data_ptr(), B, coef, out.data_ptr())
    e.ctx.sync()
    assert np.array_equal(from_dev(out), want)


# ---- 4. chunking ---------------------------------------------------------------------------------
def test_pack_in_chunks_matches_one_chunk():
    """TFHE_OPT_PACK_SCRATCH_MB = 1 leaves room for 32 items' sums (4 K splits of 8 KB each): 2 * 300 items go
    through in 19 chunks whose boundaries fall inside both output TRLWEs; same words as the unchunked call."""
    e = env("n20-2x8")
    g = rng(830)
    cts = u32rand(g, 2, 300, e.p.n + 1)
    coef = random_coef(g, e.p.N, 300)
    want = e.ctx.pack_tlwe(e.key, cts, coef)
    with e.ctx.options(pack_scratch_mb=1):
        got = e.ctx.pack_tlwe(e.key, cts, coef)
    assert e.ctx.get_option("pack_scratch_mb") == 256
    assert np.array_equal(got, want)
    assert np.array_equal(want, e.ref(cts, coef))


_BIG = {}


def big_case():
    """2 * 1,024 random inputs at n = 20 in pack_table's layout for k = 9, width 4 (stride 4, h = 8, v = 1: two
    TRLWEs of 256 entries), and the restatement's words; shared by the two tests below."""
    if not _BIG:
        e = env("n20-2x8")
        cts = u32rand(rng(860), 2048, e.p.n + 1)
        coef = (np.arange(256, dtype=np.uint32)[:, None] * 4 + np.arange(4, dtype=np.uint32)).reshape(-1)
        _BIG["case"] = (cts, coef, e.ref(cts, coef))
    return _BIG["case"]


def test_pack_ragged_last_chunk_in_another_split_regime():
    """TFHE_OPT_PACK_SCRATCH_MB = 12 with 2,048 items: a chunk of 1,536 (192 GEMM tiles: one K split on 256 CUs,
    12 MB of sums exactly) and a last chunk of 512, which on its own would take 4 splits and 16.8 MB.  The call
    keeps the first chunk's split count, so the words equal the restatement's and the unchunked call's."""
    e = env("n20-2x8")
    cts, coef, want = big_case()
    with e.ctx.options(pack_scratch_mb=12):
        got = e.ctx.pack_tlwe(e.key, cts, coef)
    assert np.array_equal(got, want)
    assert np.array_equal(e.ctx.pack_tlwe(e.key, cts, coef), want)


def test_pack_table_over_two_trlwes():
    """pack_table with v = 1 (k = 9, width 4): entry e goes to TRLWE e >> 8, slot e & 255, as
    tfhe_lookup_table_pack_slots lays a public table out."""
    e = env("n20-2x8")
    cts, coef, want = big_case()
    plan = tfhe_amd.packed_lookup_plan(e.p, 9, 4)
    assert (plan.stride, plan.h, plan.v, plan.trlwes) == (4, 8, 1, 2)
    got = e.ctx.pack_table(e.key, cts, 9, 4)
    assert got.shape == (2, 2048) and np.array_equal(got, want)
    with pytest.raises(ValueError):
        e.ctx.pack_table(e.key, cts[:-1], 9, 4)


# ---- 5. the real 128-bit set: gates -> pack -> packed lookup -> extraction -------------------------
def test_computed_table_chain_at_128(oracle, keys128):
    k = keys128
    ctx = tfhe_amd.Context("128", 0)
    ctx.load_cloud_key(k.ck.offset, k.ck.testvec, k.ck.bk, k.ck.ksk)
    p = ctx.params
    sk = tfhe_amd.SecretKey(p, k.k0, k.k1)
    # (2, 8): 700 * 8 * 3 = 16,800 TRLWE encryptions (the set's own shape, the default, is (2, 9))
    rows, basebit, t = tfhe_amd.PackingKey.generate_rows(ctx, sk, 9000, basebit=2, t=8)
    assert rows.shape == (700 * 8 * 4, 2048) and not rows[0::4].any() and rows[1::4].any(axis=1).all()
    key = tfhe_amd.PackingKey(ctx, rows, basebit, t)
    g = rng(840)
    values = g.integers(0, 16, 16)
    mask = 0b1010
    vbits = np.array([[(v >> c) & 1 for c in range(4)] for v in values], np.uint8).reshape(-1)
    mbits = np.tile(np.array([(mask >> c) & 1 for c in range(4)], np.uint8), 16)
    a, b = sk.encrypt_bool(vbits, 100), sk.encrypt_bool(mbits, 300)
    gates = ctx.gate_batch(np.full(64, tfhe_amd.XOR, np.uint8), a, b)
    want_bits = (vbits ^ mbits).astype(bool)
    assert np.array_equal(sk.decrypt_bool(gates), want_bits)

    table = ctx.pack_table(key, gates, 4, 4)
    assert ctx.last_kernels() == "k_key_switch_gemm<8,2> + k_pack_rotate_acc"
    plan = tfhe_amd.packed_lookup_plan(p, 4, 4)
    assert (plan.trlwes, plan.stride, plan.h) == (1, 4, 4) and table.shape == (1, 2048)
    coef = (np.arange(16)[:, None] * 4 + np.arange(4)).reshape(-1).astype(np.uint32)
    assert np.array_equal(table, pack_ref(p.n, p.N, rows, basebit, t, gates, coef))
    assert np.array_equal(ctx.trlwe_decrypt_bool(k.k1, table)[0, coef], want_bits)

    trgsw = np.array([oracle.trgsw_encrypt_torus_fft(k.p, mu, k.p.alpha_bsk, k.k1, 950 + mu) for mu in (0, 1)])
    sel = tfhe_amd.TrgswSet(ctx, trgsw)
    addr = np.array([[(q >> j) & 1 for j in range(4)] for q in range(16)], np.uint32)
    found = ctx.packed_lookup(sel, addr, 4, table)
    lv0 = ctx.sample_extract(found, np.arange(4), key_switch=True)
    got = sk.decrypt_bool(lv0.reshape(-1, p.n + 1)).reshape(16, 4)
    assert np.array_equal(got, want_bits.reshape(16, 4))
    assert [int(sum(int(bit) << c for c, bit in enumerate(r))) for r in got] == [int(v) ^ mask for v in values]
    sel.close()
    key.close()
    ctx.close()


# ---- 6. a LUT-message slot -------------------------------------------------------------------------
def test_pack_keeps_a_lut_message(oracle):
    """UINT4 noise at n = 18, (5, 3): 16 ciphertexts of encrypt_lwe_message (m = 16, message x / 32 on the torus)
    packed 64 coefficients apart; the phase at each slot rounds to the message."""
    e = env("n18-5x3")
    msgs = np.arange(16, dtype=np.uint32)[::-1].copy()
    cts = e.sk.encrypt_lwe_message(msgs, 16, 400)
    coef = (np.arange(16) * 64).astype(np.uint32)
    out = e.ctx.pack_tlwe(e.key, cts, coef)
    assert np.array_equal(out, e.ref(cts, coef))
    ph = trlwe_phase(oracle, e.p.N, out[0], e.sk.key_lv1)
    assert np.array_equal(np.floor(ph[coef] * 32 + 0.5).astype(np.int64) % 16, msgs)


# ---- 7. refusals, and the context works afterwards --------------------------------------------------
def test_pack_refusals_leave_the_context_usable():
    e = env("n20-2x8")
    g = rng(850)
    cts = u32rand(g, 1, 3, e.p.n + 1)
    coef = np.array([5, 0, 1023], np.uint32)
    want = e.ref(cts, coef)
    other = tfhe_amd.Context(e.pd, 0)
    multi = tfhe_amd.Context.multi(e.pd, devices=[0, 0])
    mkey = tfhe_amd.PackingKey(multi, e.rows, e.basebit, e.t)

    def refused(f):
        with pytest.raises(tfhe_amd.TfheError) as err:
            f()
        assert err.value.status == tfhe_amd.ERR_INVALID

    refused(lambda: other.pack_tlwe(e.key, cts, coef))                    # a foreign context's key
    x, out = to_dev(cts.reshape(-1)), to_dev(np.zeros(2048, np.uint32))
    refused(lambda: multi.pack_tlwe_dev(mkey, x.data_ptr(), 1, coef, out.data_ptr()))  # _dev on a multi-device context
    refused(lambda: e.ctx.pack_tlwe(e.key, cts, [5, 0, 1024]))            # coef >= N
    refused(lambda: e.ctx.pack_tlwe(e.key, cts, [5, 0, 5]))               # a duplicate
    refused(lambda: tfhe_amd.PackingKey(e.ctx, e.rows[:-1], e.basebit, e.t))  # bad len
    refused(lambda: tfhe_amd.PackingKey(e.ctx, e.rows, 4, 3))             # a shape without the GEMM form
    assert e.ctx.pack_tlwe(e.key, np.zeros((0, 3, e.p.n + 1), np.uint32), coef).shape == (0, 2048)  # B = 0
    assert np.array_equal(multi.pack_tlwe(mkey, cts, coef), want)         # host buffers: the first device
    assert np.array_equal(e.ctx.pack_tlwe(e.key, cts, coef), want)
    mkey.close()
    multi.close()
    other.close()
