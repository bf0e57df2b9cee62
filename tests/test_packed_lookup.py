"""GPU tests of the rotation by encrypted bits (k_rotate_chain) and the packed table lookup
built on it and the CMUX tree: every result word for word (np.array_equal) against the CPU
oracle's chain, built step by step from oracle.cmux and oracle.poly_mul_with_xk with selectors
from oracle.trgsw_encrypt_torus_fft."""
import ctypes as C

import numpy as np
import pytest

import tfhe_amd
from conftest import rng

pytestmark = pytest.mark.gpu
u32p = C.POINTER(C.c_uint32)


def u32rand(g, *shape):
    return g.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


_ENV = {}


class Env:
    """A context without a cloud key, the oracle's secret key (seed 42) and three selectors
    (encryptions of 0, 1 and 1 under it, seeds 900..902) from the oracle, resident as a TrgswSet."""

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


def oracle_chain(oracle, e, x, rot, sel_row):
    """acc <- trgsw.cmux(acc, (polyMulWithXK(acc.a, rot[j]), polyMulWithXK(acc.b, rot[j])), set[sel[j]]), in order."""
    N = e.p.N
    acc = np.array(x, np.uint32)
    for r, s in zip(rot, sel_row):
        turned = np.concatenate([oracle.poly_mul_with_xk(acc[:N], int(r)), oracle.poly_mul_with_xk(acc[N:], int(r))])
        acc = oracle.cmux(e.p, acc, turned, e.trgsw[s], e.off)
    return acc


def oracle_tree(oracle, e, table, addr_row):
    cur = [t for t in table]
    for s in addr_row:
        cur = [oracle.cmux(e.p, cur[2 * i], cur[2 * i + 1], e.trgsw[s], e.off) for i in range(len(cur) // 2)]
    assert len(cur) == 1
    return cur[0]


def oracle_packed(oracle, e, plan, table, addr_row):
    """The tree under bits h .. k-1 (level j' under bit h + j'), then the chain under bits 0 .. h-1."""
    h = plan.h
    x = oracle_tree(oracle, e, table, addr_row[h:]) if plan.v else table[0]
    return oracle_chain(oracle, e, x, list(plan.rot[:h]), addr_row[:h])


def address_rows(vals, k):
    """(Q, k) selector indices of the addresses vals: bit value 0 -> selector 0, 1 -> selector 1 or 2."""
    return np.array([[((v >> j) & 1) * (1 + (j + q) % 2) for j in range(k)] for q, v in enumerate(vals)], np.uint32)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def from_dev(t):
    return t.cpu().numpy().view(np.uint32)


_CASE = {}


def chain_case(oracle, pname):
    """Case 1, shared with the device-pointer test: B = 5 (a full workgroup of 4 waves and one live wave beside
    three that return), h = 4, random TRLWE words (a != 0), mixed selector bits."""
    if pname not in _CASE:
        e = env(oracle, pname)
        N = e.p.N
        x = u32rand(rng(301), 5, 2 * N)
        rot = np.array([2 * N - 8, N, 1, 2 * N - 1], np.uint32)
        sel = np.array([[(b + 2 * j + b * j) % 3 for j in range(4)] for b in range(5)], np.uint32)
        assert {0, 1, 2} <= set(sel.reshape(-1).tolist())
        want = np.array([oracle_chain(oracle, e, x[b], rot, sel[b]) for b in range(5)])
        _CASE[pname] = (x, rot, sel, want)
    return _CASE[pname]


def packed_v0_case(oracle):
    """Case 3, shared with the device-pointer test: set 128, k = 5, width 8: stride 8, h = 5, one TRLWE that
    all Q = 6 queries read."""
    if "v0" not in _CASE:
        e = env(oracle, "128")
        values = rng(302).integers(0, 256, 32).astype(np.uint64)
        table = tfhe_amd.lookup_table_pack_slots(e.tp, values, 8)
        vals = [0, 31, 5, 18, 9, 28]
        addr = address_rows(vals, 5)
        plan = tfhe_amd.packed_lookup_plan(e.tp, 5, 8)
        assert (plan.stride, plan.h, plan.v, plan.trlwes, plan.cmuxes) == (8, 5, 0, 1, 5) and table.shape[0] == 1
        want = np.array([oracle_packed(oracle, e, plan, table, addr[q]) for q in range(6)])
        _CASE["v0"] = (values, table, vals, addr, want)
    return _CASE["v0"]


# ---- 1. the chain against the oracle, L = 3, 2, 1 --------------------------------------
@pytest.mark.parametrize("pname", ["128", "uint1", "uint4"])
def test_rotate_chain_matches_oracle(oracle, pname):
    e = env(oracle, pname)
    x, rot, sel, want = chain_case(oracle, pname)
    got = e.ctx.rotate_by_bits(e.set, sel, rot, x)
    assert e.ctx.last_kernels() == f"k_rotate_chain<{e.p.L}>"
    for b in range(5):
        assert np.array_equal(got[b], want[b]), b
    assert not np.array_equal(got, x)


@pytest.mark.parametrize("r", [0, 2048])
@pytest.mark.parametrize("pname", ["128", "uint1", "uint4"])
def test_identity_rotation_returns_the_input(oracle, pname, r):
    """B = 1, h = 1, X^0 and X^2N: tmp is the bare decomposition offset, whose digits are all zero, so the
    external product is exactly 0 whatever the selector, and the result is the input bit for bit."""
    e = env(oracle, pname)
    assert r in (0, 2 * e.p.N)
    x = u32rand(rng(303 + r), 1, 2 * e.p.N)
    for s in (0, 1):
        got = e.ctx.rotate_by_bits(e.set, [[s]], [r], x)
        assert np.array_equal(got, x)
        assert np.array_equal(got[0], oracle_chain(oracle, e, x[0], [r], [s]))


# ---- 2. exponents on both sides of N: the negacyclic sign --------------------------------
def test_rotate_chain_sign_crossing(oracle):
    e = env(oracle, "128")
    N = e.p.N
    x = u32rand(rng(304), 4, 2 * N)
    rot = [N - 1, N + 1, 1023]
    sel = np.array([[1, 2, 1], [0, 1, 2], [2, 0, 0], [1, 1, 0]], np.uint32)
    got = e.ctx.rotate_by_bits(e.set, sel, rot, x)
    for b in range(4):
        assert np.array_equal(got[b], oracle_chain(oracle, e, x[b], rot, sel[b])), b


# ---- 3. v = 0: every query gathers table TRLWE 0 ------------------------------------------
def test_packed_lookup_one_shared_trlwe(oracle):
    e = env(oracle, "128")
    values, table, vals, addr, want = packed_v0_case(oracle)
    got = e.ctx.packed_lookup(e.set, addr, 8, table)
    assert e.ctx.last_kernels() == "k_rotate_chain<3>"
    dec = e.ctx.trlwe_decrypt_bool(e.k1, got)
    for q, v in enumerate(vals):
        assert np.array_equal(got[q], want[q]), q
        assert tfhe_amd.bit_utils.convert(dec[q][:8]) == int(values[v]), q


# ---- 4. the tree, then the chain ------------------------------------------------------------
@pytest.mark.parametrize("pname,k,width,shape,Q", [("128", 4, 200, (256, 4, 2, 2, 4, 5), 5),
                                                   ("uint4", 9, 8, (8, 128, 7, 2, 4, 10), 4)])
def test_packed_lookup_tree_then_chain(oracle, pname, k, width, shape, Q):
    e = env(oracle, pname)
    plan = tfhe_amd.packed_lookup_plan(e.tp, k, width)
    assert (plan.stride, plan.slots, plan.h, plan.v, plan.trlwes, plan.cmuxes) == shape
    g = rng(305 + k)
    table = u32rand(g, plan.trlwes, 2 * e.p.N)  # the caller's own table: any TRLWEs
    vals = [0, (1 << k) - 1] + [int(v) for v in g.integers(0, 1 << k, Q - 2)]
    addr = address_rows(vals, k)
    got = e.ctx.packed_lookup(e.set, addr, width, table)
    L = e.p.L
    assert e.ctx.last_kernels() == f"k_cmux<{L}> + k_rotate_chain<{L}>"
    for q in range(Q):
        assert np.array_equal(got[q], oracle_packed(oracle, e, plan, table, addr[q])), q


# ---- 5. device pointers on the caller's stream ---------------------------------------------
def test_dev_forms_equal_host_forms(oracle):
    import torch
    e = env(oracle, "128")
    N2 = 2 * e.p.N
    x, rot, sel, want_chain = chain_case(oracle, "128")
    _, table, _, addr, want_lk = packed_v0_case(oracle)
    t_x, t_table = to_dev(x), to_dev(table)
    o_chain = torch.full((5, N2), -1, dtype=torch.int32, device="cuda:0")
    o_lk = torch.full((6, N2), -1, dtype=torch.int32, device="cuda:0")
    try:
        e.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        e.ctx.rotate_by_bits_dev(e.set, sel, rot, t_x.data_ptr(), o_chain.data_ptr())
        e.ctx.packed_lookup_dev(e.set, addr, 8, t_table.data_ptr(), o_lk.data_ptr())
        e.ctx.sync()
    finally:
        e.ctx.set_stream(None)
    assert np.array_equal(from_dev(o_chain), want_chain)
    assert np.array_equal(from_dev(o_lk), want_lk)
    assert np.array_equal(from_dev(t_x), x) and np.array_equal(from_dev(t_table), table)


# ---- 6. the S-box end to end ------------------------------------------------------------------
def test_sbox_end_to_end():
    ctx = tfhe_amd.Context("128", 0)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    g = rng(306)
    sbox = g.permutation(256).astype(np.uint64)
    table = tfhe_amd.lookup_table_pack_slots(ctx.params, sbox, 8)
    plan = tfhe_amd.packed_lookup_plan(ctx.params, 8, 8)
    assert table.shape[0] == 2 and (plan.h, plan.v, plan.cmuxes) == (7, 1, 8)
    xs = np.array([0, 255, 0x5A, 0xA7])
    bits = ((xs[:, None] >> np.arange(8)[None, :]) & 1).astype(np.uint32)
    sels = tfhe_amd.TrgswSet(ctx, ctx.trgsw_encrypt(sk.key_lv1, bits.reshape(-1), seed0=10_000))
    addr = np.arange(4 * 8, dtype=np.uint32).reshape(4, 8)
    out = ctx.packed_lookup(sels, addr, 8, table)
    assert "k_rotate_chain<3>" in ctx.last_kernels()
    lv0 = ctx.sample_extract(out, np.arange(8), key_switch=True)
    got = [tfhe_amd.bit_utils.convert(sk.decrypt_bool(lv0[q])) for q in range(4)]
    assert got == [int(sbox[x]) for x in xs]
    sels.close()
    ctx.close()


# ---- 7. argument checks (no launch follows a refused call) ----------------------------------
def test_error_returns(oracle):
    e = env(oracle, "128")
    other = env(oracle, "uint4")
    lib, h, s = e.ctx.lib, e.ctx.h, e.set.h
    N2 = 2 * e.p.N
    x = np.zeros((4, N2), np.uint32)
    xp = x.ctypes.data_as(u32p)
    zeros = np.zeros(40, np.uint32)
    zp = zeros.ctypes.data_as(u32p)
    INV = tfhe_amd.ERR_INVALID

    def arr(*v):
        a = np.array(v, np.uint32)
        return a, a.ctypes.data_as(u32p)

    for rotate in (lib.tfhe_gpu_rotate_by_bits_batch, lib.tfhe_gpu_rotate_by_bits_dev):
        # h = 0 and h > TFHE_ROTATE_MAX_STEPS
        assert rotate(h, s, zp, zp, 0, xp, xp, 1) == INV
        assert rotate(h, s, zp, zp, 33, xp, xp, 1) == INV
        # an exponent > 2N
        _, bad_rot = arr(5, 2 * e.p.N + 1)
        assert rotate(h, s, zp, bad_rot, 2, xp, xp, 1) == INV
        assert b"2N" in lib.tfhe_gpu_last_error(h)
        # a selector index >= S (S = 3)
        _, bad_sel = arr(0, 3)
        assert rotate(h, s, bad_sel, zp, 2, xp, xp, 1) == INV
        assert b"set's size" in lib.tfhe_gpu_last_error(h)
        # a set of another context and parameter set
        assert rotate(other.ctx.h, s, zp, zp, 1, xp, xp, 1) == INV
        assert b"another context" in lib.tfhe_gpu_last_error(other.ctx.h)
        # null arguments
        assert rotate(h, None, zp, zp, 1, xp, xp, 1) == INV
        assert rotate(h, s, None, zp, 1, xp, xp, 1) == INV
        assert rotate(h, s, zp, None, 1, xp, xp, 1) == INV
        assert rotate(h, s, zp, zp, 1, None, xp, 1) == INV
        # an empty batch is fine
        assert rotate(h, s, None, zp, 1, None, None, 0) == 0
    for lookup in (lib.tfhe_gpu_packed_lookup_batch, lib.tfhe_gpu_packed_lookup_dev):
        # width = 0 and width > N
        assert lookup(h, s, zp, 3, 0, xp, xp, 1) == INV
        assert lookup(h, s, zp, 3, e.p.N + 1, xp, xp, 1) == INV
        # k = 0; v > 12 (width 8 leaves h = 7 of k = 20; width N leaves none of k = 13)
        assert lookup(h, s, zp, 0, 8, xp, xp, 1) == INV
        assert lookup(h, s, zp, 20, 8, xp, xp, 1) == INV
        assert lookup(h, s, zp, 13, e.p.N, xp, xp, 1) == INV
        # an address selector index >= S
        _, bad_sel = arr(0, 0, 3)
        assert lookup(h, s, bad_sel, 3, 8, xp, xp, 1) == INV
        assert b"set's size" in lib.tfhe_gpu_last_error(h)
        # a set of another context and parameter set
        assert lookup(other.ctx.h, s, zp, 3, 8, xp, xp, 1) == INV
        assert b"another context" in lib.tfhe_gpu_last_error(other.ctx.h)
        # null arguments
        assert lookup(h, None, zp, 3, 8, xp, xp, 1) == INV
        assert lookup(h, s, None, 3, 8, xp, xp, 1) == INV
        assert lookup(h, s, zp, 3, 8, None, xp, 1) == INV
        # no queries
        assert lookup(h, s, None, 3, 8, xp, None, 0) == 0
    # the Python surface refuses a table of the wrong size before the call
    with pytest.raises(ValueError):
        e.ctx.packed_lookup(e.set, np.zeros((1, 8), np.uint32), 8, x[:1])
