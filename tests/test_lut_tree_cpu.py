"""The host-only half of the bivariate LUT bootstrap (include/tfhe_gpu.h "Bivariate LUT bootstrap"): tfhe_lut_spread
word for word against a numpy restatement of its definition, the generator's table from the trivial slot TRLWE,
lut_generate2, the argument checks that need no device, and the whole tree on the oracle at a toy n: level 1 by
blind_rotate + extract + key switch, pack_tlwe_host, lut_spread_host, and blind_rotate with the packed test
vector.  No kernel runs here.  mulxk / spread_ref are shared with tests/test_lut_tree.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import tfhe_amd
from conftest import rng
from test_pack_cpu import oracle_packing_key, oracle_params, trlwe_phase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")
u32p = C.POINTER(C.c_uint32)
INV = tfhe_amd.ERR_INVALID
UINT4 = tfhe_amd.make_params("uint4")
N = UINT4.N
WIDTHS = (1, 2, 64, 256, 1024)
ROTS = (0, 1, N, 2 * N - 32, 2 * N)


def words(seed, *shape):
    return rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def mulxk(a, k):
    """polyMulWithXK (trgsw.zig:442-466) for 0 <= k <= 2N on the last axis."""
    a = np.asarray(a, np.uint32)
    n = a.shape[-1]
    neg = (0 - a.astype(np.int64)).astype(np.uint32)
    if k < n:
        return np.concatenate([neg[..., n - k:], a[..., :n - k]], axis=-1)
    k -= n
    return np.concatenate([a[..., n - k:], neg[..., :n - k]], axis=-1)


def spread_ref(x, w, rot):
    """The definition on (B, 2N): S[h] = sum_{j<w} mulxk(in[h], j), out[h] = mulxk(S[h], rot), in wrapping u32."""
    h = np.asarray(x, np.uint32).reshape(-1, 2, N)
    S = np.zeros(h.shape, np.uint64)
    for j in range(w):
        S += mulxk(h, j)
    return mulxk((S & 0xFFFFFFFF).astype(np.uint32), rot).reshape(-1, 2 * N)


def slot_trlwe(m, f):
    """The trivial TRLWELv1 (a = 0) with Encoder.new(m).encode(f(x)) at coefficient x * N/m of b, zeros elsewhere."""
    t = np.zeros(2 * N, np.uint32)
    for x in range(m):
        t[N + x * (N // m)] = ((f(x) % m) << 32) // (2 * m)  # exact: 2m divides 2^32
    return t


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("w", WIDTHS)
def test_spread_matches_restatement(w, B):
    for rot in ROTS:
        x = words(9000 + 7 * w + rot + B, B, 2 * N)
        got = tfhe_amd.lut_spread_host(UINT4, x, w, rot)
        assert np.array_equal(got, spread_ref(x, w, rot)), (w, rot)
        if w == 1 and rot in (0, 2 * N):
            assert np.array_equal(got, x)  # the identity
        if w == 1 and rot == N:
            assert np.array_equal(got, (0 - x.astype(np.int64)).astype(np.uint32))  # X^N = -1


def test_spread_of_the_full_window_wraps_every_term():
    """w = N: S[i] = 2 E[i] - T, every term but the first i + 1 negated."""
    x = words(9100, 1, 2 * N)
    got = tfhe_amd.lut_spread_host(UINT4, x, N, 0).reshape(2, N).astype(np.uint64)
    E = np.cumsum(x.reshape(2, N).astype(np.uint64), axis=1)
    assert np.array_equal(got, (2 * E - E[:, -1:]) & 0xFFFFFFFF)


@pytest.mark.parametrize("m", [4, 16, 32])
def test_spread_of_the_slots_is_the_generators_table(m):
    f = lambda x: (5 * x + 3) % m  # noqa: E731
    got = tfhe_amd.lut_spread_host(UINT4, slot_trlwe(m, f), N // m, 2 * N - N // (2 * m))[0]
    assert np.array_equal(got, tfhe_amd.lut_generate(UINT4, m, f))


def test_lut_generate2_rows_are_the_curried_tables():
    m = 16
    f = lambda x, y: (x * y + 3 * x) % m  # noqa: E731
    t = tfhe_amd.lut_generate2(UINT4, m, f)
    assert t.shape == (m, 2 * N) and t.dtype == np.uint32
    for i in range(m):
        assert np.array_equal(t[i], tfhe_amd.lut_generate(UINT4, m, lambda y: f(i, y)))


def test_spread_rejects_bad_arguments():
    lib = tfhe_amd.load_library()
    x, out = words(9200, 2 * N), np.zeros(2 * N, np.uint32)
    xp, op, pp = x.ctypes.data_as(u32p), out.ctypes.data_as(u32p), C.byref(UINT4)
    assert lib.tfhe_lut_spread(pp, xp, 4, 7, op, 1) == 0
    assert lib.tfhe_lut_spread(pp, xp, 0, 7, op, 1) == INV
    assert lib.tfhe_lut_spread(pp, xp, N + 1, 7, op, 1) == INV
    assert lib.tfhe_lut_spread(pp, xp, N, 2 * N, op, 1) == 0
    assert lib.tfhe_lut_spread(pp, xp, 4, 2 * N + 1, op, 1) == INV
    assert lib.tfhe_lut_spread(None, xp, 4, 7, op, 1) == INV
    assert lib.tfhe_lut_spread(pp, None, 4, 7, op, 1) == INV
    assert lib.tfhe_lut_spread(pp, xp, 4, 7, None, 1) == INV
    assert lib.tfhe_lut_spread(pp, None, 4, 7, None, 0) == 0
    with pytest.raises(tfhe_amd.TfheError) as err:
        tfhe_amd.lut_spread_host(UINT4, x, 0, 0)
    assert err.value.status == INV


def test_entries_refuse_a_null_context_and_are_exported():
    lib = tfhe_amd.load_library()
    x = np.zeros(2 * N, np.uint32)
    xp = x.ctypes.data_as(u32p)
    assert lib.tfhe_gpu_lut_spread_batch(None, xp, 4, 0, xp, 1) == INV
    assert lib.tfhe_gpu_lut_spread_dev(None, None, 4, 0, None, 1) == INV
    assert lib.tfhe_gpu_bootstrap_lut_each_batch(None, xp, xp, xp, 1) == INV
    assert lib.tfhe_gpu_bootstrap_lut_each_dev(None, None, None, None, 1) == INV
    assert lib.tfhe_gpu_lut_apply2_batch(None, None, None, 16, xp, 1, xp, xp, xp, xp, 1) == INV
    assert lib.tfhe_gpu_lut_apply2_dev(None, None, None, 16, None, 1, xp, xp, xp, None, 1) == INV
    for name in ("tfhe_lut_spread", "tfhe_gpu_lut_spread_batch", "tfhe_gpu_lut_spread_dev",
                 "tfhe_gpu_bootstrap_lut_each_batch", "tfhe_gpu_bootstrap_lut_each_dev",
                 "tfhe_gpu_lut_apply2_batch", "tfhe_gpu_lut_apply2_dev"):
        assert name in tfhe_amd.EXPORTED_SYMBOLS
    assert lib.tfhe_gpu_abi_version() == 7  # additions only


def test_tree_decrypts_on_the_oracle(oracle):
    """Toy set: n = 20, otherwise UINT4's numbers; keys and the packing key ((5, 3), alpha_lv1) from the oracle.
    f(x, y) = x * y mod 16 for 4 pairs: 16 level-1 bootstraps of y with lut_generate2's tables, pack_tlwe_host into
    the slots i * 64, lut_spread_host, the oracle's blind rotation of x with that test vector, extraction and key
    switch.  The test vector's phase at the slot centres is within 1/8 of the half-spacing 1/64 of f(i, y) / 32."""
    pd = dict(tfhe_amd.PARAM_SETS["uint4"], n=20)
    p, op = tfhe_amd.make_params(pd), oracle_params(pd)
    m, basebit, t = 16, 5, 3
    w, off = N // m, N // (2 * m)
    k0, k1 = oracle.secret_key(op, 42)
    ck = oracle.cloud_key(op, 43, k0, k1)
    sk = tfhe_amd.SecretKey(p, k0, k1)
    rows = oracle_packing_key(oracle, op, k0, k1, basebit, t, 6000, op.alpha_lv1)
    f = lambda x, y: (x * y) % m  # noqa: E731
    tables = tfhe_amd.lut_generate2(p, m, f)
    coef = np.arange(m, dtype=np.uint32) * w

    def bootstrap(ct, tv):
        acc = oracle.blind_rotate(op, ct, tv, ck.bk, ck.offset)
        return oracle.identity_key_switch(op, oracle.sample_extract_index(acc, 0), ck.ksk)

    pairs = [(3, 5), (15, 15), (0, 9), (7, 2)]
    for i, (x, y) in enumerate(pairs):
        cx, cy = sk.encrypt_lwe_message(np.array([x, y], np.uint32), m, seed0=9300 + 2 * i)
        g = np.array([bootstrap(cy, tables[j]) for j in range(m)])
        packed = tfhe_amd.pack_tlwe_host(p, rows, basebit, t, g, coef)
        tv = tfhe_amd.lut_spread_host(p, packed, w, 2 * N - off)[0]
        # slot x' of the test vector is centred at x' * w (the generator's layout): it holds f(x', y) / 32
        ph = trlwe_phase(oracle, N, tv, k1)[np.arange(m) * w]
        want = np.array([f(j, y) for j in range(m)]) / (2.0 * m)
        err = (ph - want + 0.5) % 1.0 - 0.5
        assert np.abs(err).max() < 1.0 / (8 * 4 * m), np.abs(err).max()
        out = bootstrap(cx, tv)
        assert int(sk.decrypt_lwe_message(out[None], m)[0]) == f(x, y), (x, y)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_host_unit_tests_pass():
    exe = os.path.join(PKG, "lib", "test_lut_tree_cpu")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
