"""Host-only checks at the parameter sets added next to "128", "80" and "uint4" (the reference's
SECURITY_110_BIT, UINT1, UINT2, UINT3; params.zig:98-207): the oracle's own sanity at sets it is
not otherwise run at, the key-file round trip at an L = 2 BK layout and a basebit 6 KSK, and what
the C ABI's parameter check accepts and refuses.  No kernel runs here."""
import ctypes as C

import numpy as np
import pytest

import tfhe_amd
from conftest import get_keys, rng

NEW_SETS = ["110", "uint1", "uint2", "uint3"]
TRUTH = {0: lambda a, b: ~(a & b), 1: lambda a, b: a | b, 2: lambda a, b: a & b, 3: lambda a, b: a ^ b,
         4: lambda a, b: a ^ b,  # the reference's xnorGate decrypts as XOR (test_oracle.py)
         5: lambda a, b: ~(a | b), 6: lambda a, b: ~a & b, 7: lambda a, b: a & ~b, 8: lambda a, b: ~a | b,
         9: lambda a, b: a | ~b}


def test_the_two_tables_name_the_same_sets():
    from oracle import PARAM_SETS
    assert PARAM_SETS == tfhe_amd.PARAM_SETS
    # transcribed from params.zig: (n, L, bgbit, iks_t, basebit)
    shape = lambda d: (d["n"], d["L"], d["bgbit"], d["iks_t"], d["basebit"])
    assert shape(PARAM_SETS["110"]) == (630, 3, 6, 8, 2)
    assert shape(PARAM_SETS["uint1"]) == (700, 2, 10, 8, 2)
    assert shape(PARAM_SETS["uint2"]) == (687, 1, 18, 3, 4)
    assert shape(PARAM_SETS["uint3"]) == (820, 1, 23, 2, 6)


@pytest.mark.parametrize("pname", NEW_SETS)
def test_oracle_gates_decrypt(oracle, pname):
    """Every gate on both input pairs that tell it from its neighbours, 20 bootstraps."""
    k = get_keys(oracle, pname)
    p = k.p
    ops = np.repeat(np.arange(10, dtype=np.uint8), 2)
    g = rng(7)
    a, b = g.integers(0, 2, ops.size).astype(bool), g.integers(0, 2, ops.size).astype(bool)
    A = np.array([oracle.tlwe_encrypt_bool(p.n, int(x), p.alpha_lv0, k.k0, 100 + i) for i, x in enumerate(a)])
    B = np.array([oracle.tlwe_encrypt_bool(p.n, int(x), p.alpha_lv0, k.k0, 200 + i) for i, x in enumerate(b)])
    out = oracle.gate_batch(p, ops, A, B, k.ck, threads=8)
    got = np.array([oracle.tlwe_decrypt_bool(p.n, ct, k.k0) for ct in out])
    assert np.array_equal(got, np.array([TRUTH[int(o)](x, y) for o, x, y in zip(ops, a, b)]))


@pytest.mark.parametrize("pname,m", [("uint2", 4), ("uint3", 8)])
def test_oracle_lut_bootstrap_decrypts(oracle, pname, m):
    """f(x) = (3x + 1) mod m over every message, twice, with the product's table generator (equal to
    the oracle's): all decrypt to f(message)."""
    k = get_keys(oracle, pname)
    p = k.p
    f = lambda x: (3 * x + 1) % m
    tv = tfhe_amd.lut_generate(tfhe_amd.make_params(pname), m, f)
    assert np.array_equal(tv, oracle.lut_generate(p.N, m, np.array([f(x) for x in range(m)], np.uint32)))
    msgs = np.tile(np.arange(m, dtype=np.uint32), 2)
    cts = np.array([oracle.encrypt_lwe_message(p.n, int(x), m, p.alpha_lv0, k.k0, 300 + i) for i, x in enumerate(msgs)])
    out = oracle.gate_batch(p, np.full(len(cts), 255, np.uint8), cts, cts, k.ck, threads=8, testvec=tv)
    got = np.array([oracle.decrypt_lwe_message(p.n, ct, m, k.k0) for ct in out])
    assert np.array_equal(got, f(msgs))


@pytest.mark.parametrize("pname,other", [("uint1", "128"), ("uint3", "uint4")])
def test_key_file_round_trip(oracle, tmp_path, pname, other):
    """tfhe_cloud_key_write / _read of the oracle's key at UINT1 (4 BK rows per step) and UINT3 (64
    KSK candidates per level): bit-exact, and refused for another set: `other` differs from the
    file's set in L and bgbit only (UINT1 / 128-bit: same n and N) or in the key-switch shape and
    bgbit only (UINT3 / UINT4: same n, N and L)."""
    k = get_keys(oracle, pname)
    tp = tfhe_amd.make_params(pname)
    path = str(tmp_path / f"ck_{pname}.key")
    tfhe_amd.cloud_key_write(path, tp, k.ck.offset, k.ck.testvec, k.ck.bk, k.ck.ksk)
    off, tv, bk, ksk = tfhe_amd.cloud_key_read(path, tp)
    assert off == k.ck.offset and np.array_equal(tv, k.ck.testvec)
    assert bk.shape == (tp.n, 2 * tp.L, 2, tp.N) and np.array_equal(bk.view(np.uint64), k.ck.bk.view(np.uint64))
    assert np.array_equal(ksk, k.ck.ksk)
    assert tfhe_amd.make_params(other).n == tp.n
    with pytest.raises(tfhe_amd.TfheError, match="status -1"):
        tfhe_amd.cloud_key_read(path, tfhe_amd.make_params(other))
    with pytest.raises(tfhe_amd.TfheError, match="status -1"):  # the lengths of another set's key
        tfhe_amd.cloud_key_write(str(tmp_path / "x.key"), tfhe_amd.make_params(other), k.ck.offset, k.ck.testvec,
                                 k.ck.bk, k.ck.ksk)


def _params_status(d):
    """The status of a context-free C ABI call whose only reason to refuse these arguments is
    params_ok (tfhe_lookup_table_pack_bits: one entry, one bit)."""
    p = tfhe_amd.make_params(d)
    value, table = C.c_uint64(1), np.zeros(2 * p.N, np.uint32)
    return tfhe_amd.load_library().tfhe_lookup_table_pack_bits(C.byref(p), C.byref(value), 1, 1,
                                                               table.ctypes.data_as(C.POINTER(C.c_uint32)))


def test_parameter_check_accepts_the_new_sets_and_the_edges():
    """params_ok: the four sets, n = 1024 (the upper edge) with the (2, 5) key switch, L = 2 with
    bgbit 6 and (4, 3); refused: n = 1025 (the UINT5..8 sets have n > 1024), L = 4, a key switch of
    (5, 2) or (5, 4)."""
    for name in NEW_SETS:
        assert _params_status(name) == 0, name
    edge = dict(tfhe_amd.PARAM_SETS["uint4"], n=1024, iks_t=2)
    assert _params_status(edge) == 0
    assert _params_status(dict(tfhe_amd.PARAM_SETS["uint1"], n=600, bgbit=6, basebit=3, iks_t=4)) == 0
    for bad in (dict(edge, n=1025), dict(edge, L=4, bgbit=8), dict(edge, basebit=2, iks_t=5),
                dict(edge, basebit=4, iks_t=5)):
        assert _params_status(bad) == tfhe_amd.ERR_INVALID, bad
