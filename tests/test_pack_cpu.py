"""CPU tests of the packing key switch's host-only half: tfhe_pack_tlwe word for word against a numpy
restatement of its definition (include/tfhe_gpu.h) with random key rows (the operation is linear in them), a
real key from the oracle's TRLWE encryption whose packed slots decrypt, and the argument checks of every entry
that return before a device is touched.  pack_ref / edge_inputs / random_coef are shared with tests/test_pack.py."""
import ctypes as C

import numpy as np
import pytest

import tfhe_amd
from conftest import rng

u32p = C.POINTER(C.c_uint32)
INV = tfhe_amd.ERR_INVALID

# (parameter set, basebit, t): the four shapes of the issue
SHAPES = {
    "n20-2x8": (dict(tfhe_amd.PARAM_SETS["128"], n=20), 2, 8),
    "n36-2x7": (dict(tfhe_amd.PARAM_SETS["128"], n=36), 2, 7),
    "n18-5x3": (dict(tfhe_amd.PARAM_SETS["uint4"], n=18), 5, 3),
    "n18-5x2": (dict(tfhe_amd.PARAM_SETS["uint4"], n=18), 5, 2),
}


def u32rand(g, *shape):
    return g.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def mulxk(a, k):
    """polyMulWithXK (trgsw.zig:442-466) for k < N: res[p] = a[p - k] for p >= k, -a[p - k + N] below."""
    a = np.asarray(a, np.uint32)
    return np.concatenate([(0 - a[a.size - k:].astype(np.int64)).astype(np.uint32), a[:a.size - k]])


def pack_ref(n, N, rows, basebit, t, cts, coef):
    """The definition: per item R = (0, (b, 0, ..)) - sum_{i,j} row[base t i + base j + d_ij] with d_ij digit j of
    a_i + PREC, then out[b] = sum_c X^coef[c] R_{b,c} on each half; sums in u64, truncated to u32."""
    base = 1 << basebit
    rows = np.asarray(rows, np.uint32).reshape(n * t * base, 2 * N)
    coef = np.atleast_1d(coef)
    x = np.asarray(cts, np.uint32).reshape(-1, coef.size, n + 1)
    prec = np.uint32(1 << (32 - (1 + basebit * t)))
    i, j = np.arange(n)[:, None], np.arange(t)[None, :]
    out = np.zeros((x.shape[0], 2 * N), np.uint64)
    for b in range(x.shape[0]):
        for c, k in enumerate(coef):
            abar = (x[b, c, :n] + prec).astype(np.uint32)  # wrapping
            d = (abar[:, None] >> (32 - (j + 1) * basebit).astype(np.uint32)) & np.uint32(base - 1)
            total = rows[(base * t * i + base * j + d).reshape(-1)].astype(np.uint64).sum(axis=0)
            R = np.zeros(2 * N, np.uint64)
            R[N] = x[b, c, n]
            R = ((R - total) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            out[b, :N] += mulxk(R[:N], int(k))
            out[b, N:] += mulxk(R[N:], int(k))
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def random_coef(g, N, C):
    """C distinct coefficients, not sorted, with 0 and N - 1 among them where C allows."""
    coef = g.permutation(N)[:C].astype(np.uint32)
    if C >= 2 and 0 not in coef:
        coef[0] = 0
    if C >= 3 and N - 1 not in coef:
        coef[1] = N - 1
    if C >= 3 and np.all(np.diff(coef.astype(np.int64)) > 0):
        coef = coef[::-1].copy()
    assert len(set(coef.tolist())) == C
    return coef


def edge_inputs(g, n, basebit, t):
    """test_reencrypt_edge_digits' inputs: a words all 0, all 0xFFFFFFFF, all 0x7FFFFFFF, and exactly PREC."""
    fills = (0, 0xFFFFFFFF, 0x7FFFFFFF, 1 << (32 - (1 + basebit * t)))
    x = np.zeros((len(fills), n + 1), np.uint32)
    for r, f in enumerate(fills):
        x[r, :n] = f
    x[:, n] = u32rand(g, len(fills))
    return x


@pytest.mark.parametrize("B,C_", [(1, 1), (1, 37), (3, 5)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pack_tlwe_matches_restatement(shape, B, C_):
    pd, basebit, t = SHAPES[shape]
    p = tfhe_amd.make_params(pd)
    g = rng(700 + 10 * B + C_)
    rows = u32rand(g, p.n * t << basebit, 2 * p.N)
    cts = u32rand(g, B, C_, p.n + 1)
    coef = random_coef(g, p.N, C_)
    if C_ == 37:
        assert 0 in coef and p.N - 1 in coef and not np.all(np.diff(coef.astype(np.int64)) > 0)
    got = tfhe_amd.pack_tlwe_host(p, rows, basebit, t, cts, coef)
    assert np.array_equal(got, pack_ref(p.n, p.N, rows, basebit, t, cts, coef))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_pack_tlwe_edge_digits(shape):
    pd, basebit, t = SHAPES[shape]
    p = tfhe_amd.make_params(pd)
    g = rng(711)
    rows = u32rand(g, p.n * t << basebit, 2 * p.N)
    cts = edge_inputs(g, p.n, basebit, t)
    coef = np.array([p.N - 1, 0, 513, 7], np.uint32)
    got = tfhe_amd.pack_tlwe_host(p, rows, basebit, t, cts, coef)
    assert np.array_equal(got, pack_ref(p.n, p.N, rows, basebit, t, cts, coef))


def oracle_packing_key(oracle, op, k0, k1, basebit, t, seed0, alpha):
    """The packing key by the oracle: row idx = TRLWELv1.encryptF64 of k key_lv0[i] / 2^((j+1) basebit) at
    coefficient 0 with DefaultPrng(seed0 + idx); k = 0 rows zero."""
    base = 1 << basebit
    rows = np.zeros((op.n * t * base, 2 * op.N), np.uint32)
    mu = np.zeros(op.N)
    for i in range(op.n):
        for j in range(t):
            for k in range(1, base):
                idx = base * t * i + base * j + k
                mu[0] = float(k) * float(k0[i]) / float(1 << ((j + 1) * basebit))
                rows[idx] = oracle.trlwe_encrypt_f64(op, mu, alpha, k1, seed0 + idx)
    return rows


def oracle_params(pd):
    from oracle import OracleParams
    return OracleParams(**pd)


def trlwe_phase(oracle, N, ct, k1):
    """b - a * s as signed fractions of the torus."""
    ph = (ct[N:] - oracle.poly_mul(ct[:N], k1)).astype(np.uint32)
    return ph.view(np.int32).astype(np.float64) / 2.0 ** 32


def test_pack_with_a_real_key_decrypts(oracle):
    """n = 20, (2, 8), key rows from oracle.trlwe_encrypt_f64 (alpha_lv1, seeds seed0 + idx): 37 packed bits
    decrypt at their slots, coefficients 0 and N - 1 among them, and the unused coefficients hold noise only,
    |phase| < 2^-10.  This test's keys and seeds give 3.3e-6 (it prints the figure; DESIGN.md §4.10 quotes it);
    the check that defined the operation measured 3.9e-6 with its own."""
    pd, basebit, t = SHAPES["n20-2x8"]
    p, op = tfhe_amd.make_params(pd), oracle_params(pd)
    k0, k1 = oracle.secret_key(op, 42)
    rows = oracle_packing_key(oracle, op, k0, k1, basebit, t, 5000, op.alpha_lv1)
    g = rng(720)
    bits = g.integers(0, 2, 37)
    cts = np.array([oracle.tlwe_encrypt_bool(op.n, int(b), op.alpha_lv0, k0, 900 + i) for i, b in enumerate(bits)])
    coef = random_coef(g, p.N, 37)
    out = tfhe_amd.pack_tlwe_host(p, rows, basebit, t, cts, coef)
    assert np.array_equal(out, pack_ref(p.n, p.N, rows, basebit, t, cts, coef))
    ph = trlwe_phase(oracle, p.N, out[0], k1)
    assert np.array_equal(ph[coef] >= 0, bits.astype(bool))
    assert np.abs(np.abs(ph[coef]) - 0.125).max() < 2.0 ** -10
    unused = np.setdiff1d(np.arange(p.N), coef)
    print("largest |phase| at unused coefficients:", np.abs(ph[unused]).max())
    assert np.abs(ph[unused]).max() < 2.0 ** -10


def test_pack_tlwe_rejects_bad_arguments():
    lib = tfhe_amd.load_library()
    pd, basebit, t = SHAPES["n20-2x8"]
    p = tfhe_amd.make_params(pd)
    N = p.N
    rows = np.zeros((p.n * t << basebit, 2 * N), np.uint32)
    x = np.zeros((N + 1, p.n + 1), np.uint32)
    out = np.zeros(2 * N, np.uint32)
    rp, xp, op = (a.ctypes.data_as(u32p) for a in (rows, x, out))

    def call(coef, C_, pp=C.byref(p), r=rp, bb=basebit, tt=t, i=xp, o=op):
        coef = np.asarray(coef, np.uint32)
        return lib.tfhe_pack_tlwe(pp, r, bb, tt, i, coef.ctypes.data_as(u32p), C_, o, 1)

    assert call([3, 1], 2) == 0
    assert call([3, 1], 0) == INV
    assert call(np.arange(N + 1), N + 1) == INV
    assert call(np.arange(N), N) == 0
    assert call([3, N], 2) == INV
    assert call([3, 1, 3], 3) == INV
    assert call([3, 1], 2, bb=4, tt=3) == INV
    assert call([3, 1], 2, bb=2, tt=6) == INV
    assert call([3, 1], 2, pp=None) == INV
    assert call([3, 1], 2, r=None) == INV
    assert call([3, 1], 2, i=None) == INV
    assert call([3, 1], 2, o=None) == INV
    assert lib.tfhe_pack_tlwe(C.byref(p), rp, basebit, t, xp, None, 2, op, 1) == INV
    with pytest.raises(tfhe_amd.TfheError) as err:
        tfhe_amd.pack_tlwe_host(p, rows, basebit, t, x[:2], [5, 5])
    assert err.value.status == INV


def test_entries_refuse_a_null_context_and_are_exported():
    lib = tfhe_amd.load_library()
    x = np.zeros(2048, np.uint32)
    xp = x.ctypes.data_as(u32p)
    h = C.c_void_p()
    assert lib.tfhe_gpu_packing_key_gen(None, xp, xp, 0.0, 2, 8, 1, xp) == INV
    assert lib.tfhe_gpu_packing_key_load(None, xp, 2048, 2, 8, C.byref(h)) == INV and not h
    assert lib.tfhe_gpu_pack_tlwe_batch(None, None, xp, xp, 1, xp, 1) == INV
    assert lib.tfhe_gpu_pack_tlwe_dev(None, None, None, xp, 1, None, 1) == INV
    lib.tfhe_gpu_packing_key_destroy(None)
    for name in ("tfhe_gpu_packing_key_gen", "tfhe_gpu_packing_key_load", "tfhe_gpu_packing_key_destroy",
                 "tfhe_gpu_pack_tlwe_batch", "tfhe_gpu_pack_tlwe_dev", "tfhe_pack_tlwe"):
        assert name in tfhe_amd.EXPORTED_SYMBOLS
    assert tfhe_amd.OPTIONS["pack_scratch_mb"] == 19 and tfhe_amd.OPTION_DEFAULTS["pack_scratch_mb"] == 256


def test_default_shape_is_the_sets_own_where_the_gemm_has_it():
    shape = tfhe_amd.PackingKey.default_shape
    assert shape(tfhe_amd.make_params("128")) == (2, 9) and shape(tfhe_amd.make_params("110")) == (2, 8)
    assert shape(tfhe_amd.make_params("uint4")) == (5, 3)
    assert shape(tfhe_amd.make_params("uint2")) == (2, 8) and shape(tfhe_amd.make_params("uint3")) == (2, 8)
