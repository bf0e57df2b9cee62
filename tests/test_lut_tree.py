"""The bivariate LUT bootstrap on the device (include/tfhe_gpu.h "Bivariate LUT bootstrap") at UINT4: spread against
its host definition, bootstrap_lut_each against bootstrap_lut_batch per item and the oracle, and lut_apply2 word for
word (np.array_equal) against its four-step definition made of the existing public entries and the host definitions
(lut_apply, pack_tlwe_host, lut_spread_host, bootstrap_lut_batch), also chunked and on device buffers.  Only the
decrypt test reads messages: all 256 pairs of two 4-bit digits through the low and the high nibble of their product,
with the test vectors' measured phase error at the slot centres."""
import numpy as np
import pytest

import tfhe_amd
from conftest import rng
from test_lut_circuit import ctx_for
from test_lut_tree_cpu import ROTS, WIDTHS, words

pytestmark = pytest.mark.gpu

INV = tfhe_amd.ERR_INVALID
N = 1024
_ENV = {}


class Env:
    """The module's keys: the oracle's seeded UINT4 cloud key on the shared context (get_keys(oracle, "uint4")) and
    one packing key of the default shape (5, 3) with alpha_lv1, its host rows kept for pack_tlwe_host."""

    def __init__(self, oracle):
        self.c, self.k = ctx_for(oracle, "uint4")
        self.p = self.c.params
        self.sk = tfhe_amd.SecretKey(self.p, self.k.k0, self.k.k1)
        self.rows, self.basebit, self.t = tfhe_amd.PackingKey.generate_rows(self.c, self.sk, 7100)
        self.key = tfhe_amd.PackingKey(self.c, self.rows, self.basebit, self.t)


def env(oracle):
    if "e" not in _ENV:
        _ENV["e"] = Env(oracle)
    return _ENV["e"]


def status(call):
    with pytest.raises(tfhe_amd.TfheError) as e:
        call()
    return e.value.status


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def from_dev(t):
    return t.cpu().numpy().view(np.uint32)


def lo(m):
    return lambda x, y: (x * y) % m


def hi(m):
    return lambda x, y: (x * y) // m


def two_tables(p, m):
    """F = 2: the level-1 tables of the low and the high digit of x * y, (2m, 2N)."""
    return np.concatenate([tfhe_amd.lut_generate2(p, m, lo(m)), tfhe_amd.lut_generate2(p, m, hi(m))])


# ---- 1. spread -------------------------------------------------------------------------------------
def test_spread_matches_host_definition(oracle):
    """Every (w, rot) of the CPU test, B = 1 and 3, random words on both halves: the host definition's words; the
    kernel's two branches (i >= w, i < w) and all three signs of the rotation are in these shapes."""
    c = env(oracle).c
    for w in WIDTHS:
        for rot in ROTS:
            for B in (1, 3):
                x = words(9400 + 7 * w + rot + B, B, 2 * N)
                got = c.lut_spread(x, w, rot)
                assert np.array_equal(got, tfhe_amd.lut_spread_host(c.params, x, w, rot)), (w, rot, B)
    assert c.last_kernels().startswith("k_lut_spread")


def test_spread_dev_and_in_place(oracle):
    import torch
    c = env(oracle).c
    for w, rot in ((64, 2 * N - 32), (256, 1), (1024, N), (1, 0)):
        x = words(9500 + w, 3, 2 * N)
        want = tfhe_amd.lut_spread_host(c.params, x, w, rot)
        t_in = to_dev(x)
        t_out = torch.full((3, 2 * N), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the spread on the context's: unordered otherwise
        c.lut_spread_dev(t_in.data_ptr(), w, rot, t_out.data_ptr(), 3)
        c.lut_spread_dev(t_in.data_ptr(), w, rot, t_in.data_ptr(), 3)  # in place
        c.sync()
        assert np.array_equal(from_dev(t_out), want), (w, rot)
        assert np.array_equal(from_dev(t_in), want), (w, rot)


# ---- 2. a test vector per item ---------------------------------------------------------------------
def test_bootstrap_lut_each(oracle):
    """B = 5 (one more than a workgroup's 4 items), test vectors with random a halves: bootstrap_lut_batch called
    per item, the oracle's blind rotation, extraction and key switch for two items, and the _dev variant."""
    import torch
    e = env(oracle)
    c, k = e.c, e.k
    B = 5
    cts = e.sk.encrypt_lwe_message(np.array([0, 3, 7, 12, 15], np.uint32), 16, seed0=9600)
    tvs = np.array([tfhe_amd.lut_generate(c.params, 16, lambda x, j=j: (3 * x + j) % 16) for j in range(B)])
    tvs[:, :N] = words(9601, B, N)
    got = c.bootstrap_lut_each(cts, tvs)
    kernels = c.last_kernels()
    assert "TV" in kernels.split(" + ")[0], kernels
    for i in range(B):
        assert np.array_equal(got[i], c.bootstrap_lut_batch(cts[i:i + 1], tvs[i])[0]), i
    for i in (1, 4):
        acc = oracle.blind_rotate(k.p, cts[i], tvs[i], k.ck.bk, k.ck.offset)
        assert np.array_equal(got[i], oracle.identity_key_switch(k.p, oracle.sample_extract_index(acc, 0), k.ck.ksk)), i
    t_in, t_tv = to_dev(cts), to_dev(tvs)
    t_out = torch.full((B, c.n1), -1, dtype=torch.int32, device="cuda:0")
    c.bootstrap_lut_each_dev(t_in.data_ptr(), t_tv.data_ptr(), t_out.data_ptr(), B)
    c.sync()
    assert np.array_equal(from_dev(t_out), got)


# ---- 3. the fused node against its definition ------------------------------------------------------
def definition(e, ls, m, pool, nodes):
    """Steps 1-4 of the header out of the existing public entries and the host definitions -> (out, TV)."""
    c, w = e.c, N // m
    fn, xs, ys = nodes
    level1 = [(int(fn[b]) * m + i, [(int(ys[b]), 1)], 0) for b in range(len(fn)) for i in range(m)]
    g = c.lut_apply(ls, pool, level1).reshape(len(fn), m, c.n1)
    coef = np.arange(m, dtype=np.uint32) * w
    packed = tfhe_amd.pack_tlwe_host(c.params, e.rows, e.basebit, e.t, g, coef)
    tv = tfhe_amd.lut_spread_host(c.params, packed, w, 2 * N - N // (2 * m))
    out = np.array([c.bootstrap_lut_batch(pool[xs[b]][None], tv[b])[0] for b in range(len(fn))])
    return out, tv


@pytest.mark.parametrize("m", [16, 4])
def test_apply2_matches_its_definition(oracle, m):
    """B = 5, F = 2: the fused call's words are the definition's; again with TFHE_OPT_PACK_SCRATCH_MB = 1 (32 items'
    sums: 3 chunks of 2 nodes at m = 16), and on device buffers."""
    import torch
    e = env(oracle)
    c = e.c
    g = rng(9700 + m)
    pool = e.sk.encrypt_lwe_message(g.integers(0, m, 7).astype(np.uint32), m, seed0=9700 + 10 * m)
    nodes = (np.array([0, 1, 1, 0, 1], np.uint32), g.integers(0, 7, 5).astype(np.uint32),
             g.integers(0, 7, 5).astype(np.uint32))
    ls = tfhe_amd.LutSet(c, two_tables(c.params, m))
    try:
        want, _ = definition(e, ls, m, pool, nodes)
        got = c.lut_apply2(ls, e.key, m, pool, nodes)
        kernels = c.last_kernels()
        with c.options(pack_scratch_mb=1):
            chunked = c.lut_apply2(ls, e.key, m, pool, nodes)
        t_pool = to_dev(pool)
        t_out = torch.full((5, c.n1), -1, dtype=torch.int32, device="cuda:0")
        c.lut_apply2_dev(ls, e.key, m, t_pool.data_ptr(), 7, nodes, t_out.data_ptr())
        c.sync()
    finally:
        ls.close()
    assert "TV" in kernels.split(" + ")[0], kernels
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1)).tolist()
    assert np.array_equal(chunked, want)
    assert np.array_equal(from_dev(t_out), want)
    # the nodes as a list of triples
    assert _nodes_as_triples_agree(nodes)


def _nodes_as_triples_agree(nodes):
    a = tfhe_amd._apply2_nodes(nodes)
    b = tfhe_amd._apply2_nodes([tuple(int(col[i]) for col in nodes) for i in range(nodes[0].size)])
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 4. every pair decrypts ------------------------------------------------------------------------
def test_all_pairs_decrypt_and_the_test_vector_noise(oracle):
    """All 256 pairs (x, y) of 4-bit digits, each pair its own two fresh ciphertexts, f0 = x * y mod 16 and
    f1 = x * y >> 4: 512 nodes, every output correct.  The same test vectors rebuilt from the separate device entries
    give the fused call's words, and their phase error at the 16 slot centres (8,192 samples) has its sigma printed
    and held under 1/8 of the half-spacing 1/64 (the header's noise rule).  Measured on the MI355X with these keys
    and seeds: sigma = 7.49e-4, max = 2.42e-3."""
    e = env(oracle)
    c, m, w = e.c, 16, 64
    xv, yv = np.divmod(np.arange(256, dtype=np.uint32), 16)
    pool = np.concatenate([e.sk.encrypt_lwe_message(xv, m, seed0=9800), e.sk.encrypt_lwe_message(yv, m, seed0=10100)])
    fn = np.repeat(np.array([0, 1], np.uint32), 256)
    xs, ys = np.tile(np.arange(256, dtype=np.uint32), 2), np.tile(np.arange(256, 512, dtype=np.uint32), 2)
    ls = tfhe_amd.LutSet(c, two_tables(c.params, m))
    try:
        got = c.lut_apply2(ls, e.key, m, pool, (fn, xs, ys))
        level1 = [(int(fn[b]) * m + i, [(int(ys[b]), 1)], 0) for b in range(512) for i in range(m)]
        g = c.lut_apply(ls, pool, level1)
        tv = c.lut_spread(c.pack_tlwe(e.key, g.reshape(512, m, c.n1), np.arange(m, dtype=np.uint32) * w), w, 2 * N - 32)
        again = c.bootstrap_lut_each(pool[xs], tv)
    finally:
        ls.close()
    assert np.array_equal(again, got)
    dec = e.sk.decrypt_lwe_message(got, m)
    want = np.concatenate([(xv * yv) % 16, (xv * yv) >> 4])
    wrong = np.flatnonzero(dec != want)
    assert wrong.size == 0, [(int(xs[i]) // 16, int(xs[i]) % 16, int(fn[i])) for i in wrong[:10]]
    # phase of TV_b at the slot centres x' * w against f_fn(x', y) / 32
    a_s = c.poly_mul(tv[:, :N], np.broadcast_to(e.k.k1, (512, N)))
    ph = (tv[:, N:] - a_s).astype(np.uint32)[:, ::w].view(np.int32) / 2.0 ** 32
    xp = np.arange(16)[None, :]
    y_of = np.tile(yv, 2)[:, None].astype(np.int64)
    f_of = np.where(fn[:, None] == 0, (xp * y_of) % 16, (xp * y_of) >> 4) / 32.0
    err = (ph - f_of + 0.5) % 1.0 - 0.5
    sigma, worst = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
    print(f"test-vector phase error at the slot centres: sigma = {sigma:.3e}, max = {worst:.3e}, "
          f"half-spacing = {1 / 64:.3e}")
    assert sigma < 1.0 / (64 * 8)


# ---- 5. refusals -----------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(oracle):
    import torch
    e = env(oracle)
    c, m = e.c, 16
    pool = e.sk.encrypt_lwe_message(np.array([3, 5, 9], np.uint32), m, seed0=9900)
    tables = two_tables(c.params, m)
    ok = (np.array([0, 1], np.uint32), np.array([0, 2], np.uint32), np.array([1, 1], np.uint32))
    other = tfhe_amd.Context("uint4", 0)  # no cloud key
    multi = tfhe_amd.Context.multi("uint4", devices=[0, 0])
    ls = tfhe_amd.LutSet(c, tables)
    ls_odd = tfhe_amd.LutSet(c, tables[:24])
    try:
        ls_other, ls_multi = tfhe_amd.LutSet(other, tables), tfhe_amd.LutSet(multi, tables)
        key_other = tfhe_amd.PackingKey(other, e.rows, e.basebit, e.t)
        want = c.lut_apply2(ls, e.key, m, pool, ok)

        def call(ctx=c, s=ls, key=e.key, mm=m, nodes=ok, pl=pool):
            return ctx.lut_apply2(s, key, mm, pl, nodes)

        for bad_m in (0, 1, 3, 12, 1024, 2048):
            assert status(lambda: call(mm=bad_m)) == INV, bad_m
        assert status(lambda: call(s=ls_odd, mm=16)) == INV  # 24 tables: no multiple of 16
        assert call(s=ls_odd, mm=8, nodes=(ok[0] * 2, ok[1], ok[2])).shape == (2, c.n1)  # 3 functions at m = 8: fn 0, 2
        assert status(lambda: call(s=ls_odd, mm=8, nodes=(np.array([3, 0], np.uint32), ok[1], ok[2]))) == INV
        assert status(lambda: call(nodes=(np.array([0, 2], np.uint32), ok[1], ok[2]))) == INV  # fn * m + m > 32
        assert status(lambda: call(nodes=(ok[0], np.array([0, 3], np.uint32), ok[2]))) == INV  # x_src >= P
        assert status(lambda: call(nodes=(ok[0], ok[1], np.array([3, 1], np.uint32)))) == INV  # y_src >= P
        assert status(lambda: call(s=ls_other)) == INV
        assert status(lambda: call(key=key_other)) == INV
        lib, h = c.lib, c.h
        u32p = tfhe_amd.u32p
        pp, op = pool.ctypes.data_as(u32p), np.zeros((2, c.n1), np.uint32).ctypes.data_as(u32p)
        f, x, y = (a.ctypes.data_as(u32p) for a in ok)
        assert lib.tfhe_gpu_lut_apply2_batch(h, None, e.key.h, m, pp, 3, f, x, y, op, 2) == INV
        assert lib.tfhe_gpu_lut_apply2_batch(h, ls.h, None, m, pp, 3, f, x, y, op, 2) == INV
        assert lib.tfhe_gpu_lut_apply2_batch(h, ls.h, e.key.h, m, None, 3, f, x, y, op, 2) == INV
        assert lib.tfhe_gpu_lut_apply2_batch(h, ls.h, e.key.h, m, pp, 3, None, x, y, op, 2) == INV
        assert lib.tfhe_gpu_lut_apply2_batch(h, ls.h, e.key.h, m, pp, 3, f, None, y, op, 2) == INV
        assert lib.tfhe_gpu_lut_apply2_batch(h, ls.h, e.key.h, m, pp, 3, f, x, None, op, 2) == INV
        assert lib.tfhe_gpu_lut_apply2_batch(h, ls.h, e.key.h, m, pp, 3, f, x, y, None, 2) == INV
        assert lib.tfhe_gpu_lut_apply2_batch(h, ls.h, e.key.h, m, None, 0, None, None, None, None, 0) == 0  # B = 0
        assert lib.tfhe_gpu_bootstrap_lut_each_batch(h, None, None, None, 0) == 0
        assert lib.tfhe_gpu_lut_spread_batch(h, None, 4, 0, None, 0) == 0
        # no cloud key
        assert status(lambda: call(ctx=other, s=ls_other, key=key_other)) == tfhe_amd.ERR_NO_KEY
        assert status(lambda: other.bootstrap_lut_each(pool[:1], tables[:1])) == tfhe_amd.ERR_NO_KEY
        assert other.lut_spread(tables[:1], 64, 7).shape == (1, 2 * N)  # spread needs none
        # spread's own checks, and a null argument
        one = tables[:1]
        assert status(lambda: c.lut_spread(one, 0, 0)) == INV
        assert status(lambda: c.lut_spread(one, N + 1, 0)) == INV
        assert status(lambda: c.lut_spread(one, 64, 2 * N + 1)) == INV
        assert lib.tfhe_gpu_lut_spread_batch(h, None, 4, 0, op, 1) == INV
        assert lib.tfhe_gpu_bootstrap_lut_each_batch(h, pp, None, op, 1) == INV
        # _dev on a multi-device context
        t = torch.zeros((4, 2 * N), dtype=torch.int32, device="cuda:0")
        assert status(lambda: multi.lut_spread_dev(t.data_ptr(), 64, 0, t.data_ptr(), 1)) == INV
        assert status(lambda: multi.bootstrap_lut_each_dev(t.data_ptr(), t.data_ptr(), t.data_ptr(), 1)) == INV
        assert status(lambda: multi.lut_apply2_dev(ls_multi, e.key, m, t.data_ptr(), 3, ok, t.data_ptr())) == INV
        # and the context still works
        assert np.array_equal(call(), want)
        for x_ in (ls_other, ls_multi, key_other):
            x_.close()
    finally:
        ls.close()
        ls_odd.close()
        other.close()
        multi.close()
