"""GPU tests of the packed scatter-add (k_rotate_chain, k_demux / k_demux_shared, k_scatter_reduce) and the table
write built on it: every result word for word (np.array_equal) against the definition built on the CPU
(tests/scatter_model.py: oracle.cmux, oracle.poly_mul_with_xk, oracle.external_product and numpy's wrapping adds)
with selectors from oracle.trgsw_encrypt_torus_fft."""
import ctypes as C

import numpy as np
import pytest

import tfhe_amd
from conftest import rng
from scatter_model import scatter_add, trlwe_phase

pytestmark = pytest.mark.gpu
u32p = C.POINTER(C.c_uint32)


def u32rand(g, *shape):
    return g.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


_ENV = {}


class Env:
    """A context without a cloud key, the oracle's secret key (seed 42) and three selectors (encryptions of 0, 1
    and 1 under it, seeds 900..902) from the oracle, resident as a TrgswSet."""

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

    def want(self, oracle, k, width, deltas, addr, table):
        plan = tfhe_amd.packed_lookup_plan(self.tp, k, width)
        return scatter_add(oracle, self.p, self.off, self.trgsw, plan, k, deltas, addr, table)


def env(oracle, pname):
    if pname not in _ENV:
        _ENV[pname] = Env(oracle, pname)
    return _ENV[pname]


def address_rows(vals, k):
    """(Q, k) selector indices of the addresses vals: bit value 0 -> selector 0, 1 -> selector 1 or 2."""
    return np.array([[((v >> j) & 1) * (1 + (j + q) % 2) for j in range(k)] for q, v in enumerate(vals)], np.uint32)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def from_dev(t):
    return t.cpu().numpy().view(np.uint32)


_CASE = {}


def tree_case(oracle):
    """Set 128, k = 4, width 256 (stride 256, h = 2, v = 2: 4 TRLWEs), Q = 37 random deltas on a random table,
    addresses 0 and 15 among them and several shared: the chunk test's case, whose first queries serve the
    composition and device-pointer tests as well.  The oracle's result is computed once."""
    if "tree" not in _CASE:
        e = env(oracle, "128")
        g = rng(411)
        N2 = 2 * e.p.N
        table, deltas = u32rand(g, 4, N2), u32rand(g, 37, N2)
        vals = [0, 15] + [int(v) for v in g.integers(0, 16, 35)]
        addr = address_rows(vals, 4)
        plan = tfhe_amd.packed_lookup_plan(e.tp, 4, 256)
        assert (plan.stride, plan.h, plan.v, plan.trlwes) == (256, 2, 2, 4)
        want5 = e.want(oracle, 4, 256, deltas[:5], addr[:5], table)
        want = e.want(oracle, 4, 256, deltas[5:], addr[5:], want5)  # wrapping adds: the sum in two parts
        _CASE["tree"] = (table, deltas, addr, want5, want)
    return _CASE["tree"]


# ---- 1. the demux tree alone (h = 0), L = 3, 2, 1 ------------------------------------------------
@pytest.mark.parametrize("k,Q", [(1, 3), (3, 2)])
@pytest.mark.parametrize("pname", ["128", "uint1", "uint4"])
def test_demux_alone_matches_oracle(oracle, pname, k, Q):
    """width = N: stride N, h = 0, a table of 2^k whole TRLWEs.  k = 1, Q = 3: one external product per query,
    three live waves beside one that returns.  k = 3, Q = 2: levels of 1, 2 and 4 parents per query, the third in
    the workgroup form (k_demux_shared) unless cmux_form = 1 forces the per-wave form; the words are the same."""
    e = env(oracle, pname)
    N, L = e.p.N, e.p.L
    plan = tfhe_amd.packed_lookup_plan(e.tp, k, N)
    assert (plan.stride, plan.h, plan.v, plan.trlwes) == (N, 0, k, 1 << k)
    g = rng(400 + 10 * k + L)
    table, deltas = u32rand(g, 1 << k, 2 * N), u32rand(g, Q, 2 * N)
    addr = address_rows([1, 1, 0] if k == 1 else [5, 6], k)
    assert {0, 1, 2} <= set(addr.reshape(-1).tolist())
    want = e.want(oracle, k, N, deltas, addr, table)
    got = e.ctx.packed_scatter_add(e.set, addr, N, deltas, table)
    assert e.ctx.last_kernels() == f"k_demux<{L}>"
    assert np.array_equal(got, want)
    assert not np.array_equal(got, table)
    with e.ctx.options(cmux_form=1):
        again = e.ctx.packed_scatter_add(e.set, addr, N, deltas, table)
        assert e.ctx.last_kernels() == f"k_demux<{L}>"
    assert np.array_equal(again, want)


# ---- 2. the rotation alone (v = 0) -----------------------------------------------------------------
def test_rotation_alone_matches_oracle(oracle):
    """Set 128, k = 5, width 8: one TRLWE of 32 slots, Q = 6 with addresses 18 twice: both deltas land."""
    e = env(oracle, "128")
    N2 = 2 * e.p.N
    plan = tfhe_amd.packed_lookup_plan(e.tp, 5, 8)
    assert (plan.stride, plan.h, plan.v, plan.trlwes) == (8, 5, 0, 1)
    g = rng(402)
    table, deltas = u32rand(g, 1, N2), u32rand(g, 6, N2)
    addr = address_rows([0, 31, 18, 9, 18, 28], 5)
    want = e.want(oracle, 5, 8, deltas, addr, table)
    got = e.ctx.packed_scatter_add(e.set, addr, 8, deltas, table)
    assert e.ctx.last_kernels() == "k_rotate_chain<3>"
    assert np.array_equal(got, want)
    # without the second write to 18 the table lacks exactly that delta's leaf: both landed
    one = e.ctx.packed_scatter_add(e.set, np.delete(addr, 4, axis=0), 8, np.delete(deltas, 4, axis=0), table)
    assert not np.array_equal(one, got)
    assert np.array_equal(e.want(oracle, 5, 8, deltas[4:5], addr[4:5], one), got)


# ---- 3. both, with meaning -------------------------------------------------------------------------
def test_writes_change_the_addressed_entries(oracle):
    """Set 128, k = 9, width 8 (h = 7, v = 2): a table of 512 bytes, 5 of them replaced by deltas that encrypt
    new - old per bit (0 or +-1/4 at alpha_lv1); the words equal the oracle's, and a packed lookup of the written
    and of 3 unwritten addresses decrypts to the model.  (The oracle alone, at this shape: phase error at most
    0.0020 after one write and 0.0071 after eight, against a margin of 0.125.)"""
    e = env(oracle, "128")
    N = e.p.N
    plan = tfhe_amd.packed_lookup_plan(e.tp, 9, 8)
    assert (plan.stride, plan.h, plan.v, plan.trlwes) == (8, 7, 2, 4)
    g = rng(403)
    model = g.integers(0, 256, 512).astype(np.uint64)
    table = tfhe_amd.lookup_table_pack_slots(e.tp, model, 8)
    written = [0, 511, 0b101100101, 130, 257]
    new = [0xFF, 0x00, 0x5A, int(model[130]) ^ 0x81, 0xC3]
    deltas = []
    for q, (a, v) in enumerate(zip(written, new)):
        mu = np.zeros(N)
        for c in range(8):
            mu[c] = 0.25 * (((v >> c) & 1) - ((int(model[a]) >> c) & 1))
        deltas.append(oracle.trlwe_encrypt_f64(e.p, mu, e.p.alpha_lv1, e.k1, 980 + q))
        model[a] = v
    deltas = np.array(deltas)
    addr = address_rows(written, 9)
    got = e.ctx.packed_scatter_add(e.set, addr, 8, deltas, table)
    assert e.ctx.last_kernels() == "k_rotate_chain<3> + k_demux<3>"
    assert np.array_equal(got, e.want(oracle, 9, 8, deltas, addr, table))
    reads = written + [1, 258, 384]
    out = e.ctx.packed_lookup(e.set, address_rows(reads, 9), 8, got)
    dec = e.ctx.trlwe_decrypt_bool(e.k1, out)
    for q, a in enumerate(reads):
        assert tfhe_amd.bit_utils.convert(dec[q][:8]) == int(model[a]), (q, a)


# ---- 4. a zero delta --------------------------------------------------------------------------------
def test_zero_delta_leaves_the_table_unchanged(oracle):
    """An all-zero TRLWE: tmp is the bare decomposition offset, whose digits are all zero, so every external
    product of the chain and of the tree is exactly 0 and the table comes back bit for bit."""
    e = env(oracle, "128")
    table = u32rand(rng(404), 4, 2 * e.p.N)
    addr = address_rows([0b101100101, 511], 9)
    got = e.ctx.packed_scatter_add(e.set, addr, 8, np.zeros((2, 2 * e.p.N), np.uint32), table)
    assert e.ctx.last_kernels() == "k_rotate_chain<3> + k_demux<3>"
    assert np.array_equal(got, table)


# ---- 5. chunks ----------------------------------------------------------------------------------------
def test_chunked_scatter_is_the_same_sum(oracle):
    """scatter_scratch_mb = 1 leaves room for 1 MB / (4 x 8 KB) = 32 queries' leaves: Q = 37 runs as 32 + 5 and
    gives the words of the oracle and of the same call in one chunk."""
    e = env(oracle, "128")
    table, deltas, addr, _, want = tree_case(oracle)
    with e.ctx.options(scatter_scratch_mb=1):
        assert e.ctx.get_option("scatter_scratch_mb") == 1
        got = e.ctx.packed_scatter_add(e.set, addr, 256, deltas, table)
    assert e.ctx.get_option("scatter_scratch_mb") == 256
    assert np.array_equal(got, want)
    assert np.array_equal(e.ctx.packed_scatter_add(e.set, addr, 256, deltas, table), want)


# ---- 6. against the entry points the scatter is made of, without the oracle -----------------------
def test_scatter_equals_its_composition(oracle):
    """rotate_by_bits with rot[j] = stride << j, cmux with an all-zero in0 (ExtProd(sel, in1 - 0) + 0 = hi), and
    numpy for lo = x - hi and the sum: the same words at v = 2."""
    e = env(oracle, "128")
    table, deltas, addr, _, _ = tree_case(oracle)
    deltas, addr = deltas[:5], addr[:5]
    zero = np.zeros((1, 2 * e.p.N), np.uint32)
    d = e.ctx.rotate_by_bits(e.set, addr[:, :2], [256, 512], deltas)
    want = table.copy()
    for q in range(5):
        nodes = [d[q]]
        for level in range(2):
            nxt = []
            for x in nodes:
                hi = e.ctx.cmux(e.set, [addr[q, 3 - level]], zero, x[None, :])[0]
                nxt += [x - hi, hi]
            nodes = nxt
        for i in range(4):
            want[i] += nodes[i]
    assert np.array_equal(e.ctx.packed_scatter_add(e.set, addr, 256, deltas, table), want)


# ---- 7. device pointers, in place, on the caller's stream ------------------------------------------
def test_dev_form_equals_host_form_in_place(oracle):
    import torch
    e = env(oracle, "128")
    table, deltas, addr, want5, _ = tree_case(oracle)
    t_table, t_delta, t_sixth = to_dev(table), to_dev(deltas[:5]), to_dev(deltas[5:6])
    try:
        e.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        e.ctx.packed_scatter_add_dev(e.set, addr[:5], 256, t_delta.data_ptr(), t_table.data_ptr())
        e.ctx.sync()
        assert np.array_equal(from_dev(t_table), want5)
        assert np.array_equal(from_dev(t_delta), deltas[:5])
        # tensors in place of the addresses: the table's size is checked before the call
        with pytest.raises(ValueError):
            e.ctx.packed_scatter_add_dev(e.set, addr[:5], 8, t_delta, t_table)
        e.ctx.packed_scatter_add_dev(e.set, addr[5:6], 256, t_sixth, t_table)
        e.ctx.sync()
    finally:
        e.ctx.set_stream(None)
    assert np.array_equal(from_dev(t_table), e.ctx.packed_scatter_add(e.set, addr[5:6], 256, deltas[5:6], want5))


def test_dev_form_refuses_a_multi_device_context(oracle):
    e = env(oracle, "128")
    multi = tfhe_amd.Context.multi("128", devices=[0, 0])
    with pytest.raises(tfhe_amd.TfheError) as err:
        multi.packed_scatter_add_dev(e.set, np.zeros((1, 4), np.uint32), 256, 64, 64)  # never dereferenced
    assert err.value.status == tfhe_amd.ERR_INVALID and "single-device" in str(err.value)
    multi.close()


# ---- 8. refusals (no upload or launch follows a refused call) --------------------------------------
def test_refusals_leave_the_context_usable(oracle):
    e = env(oracle, "128")
    other = env(oracle, "uint4")
    lib, h, s = e.ctx.lib, e.ctx.h, e.set.h
    N2 = 2 * e.p.N
    x = u32rand(rng(405), 8, N2)
    keep = x.copy()
    xp = x.ctypes.data_as(u32p)
    d = np.zeros((1, N2), np.uint32)
    dp = d.ctypes.data_as(u32p)
    zeros = np.zeros(40, np.uint32)
    zp = zeros.ctypes.data_as(u32p)
    bad = np.array([0, 0, 3], np.uint32)
    INV = tfhe_amd.ERR_INVALID
    for scatter in (lib.tfhe_gpu_packed_scatter_add_batch, lib.tfhe_gpu_packed_scatter_add_dev):
        # k = 0; width = 0 and width > N
        assert scatter(h, s, zp, 0, 8, dp, xp, 1) == INV
        assert scatter(h, s, zp, 3, 0, dp, xp, 1) == INV
        assert scatter(h, s, zp, 3, e.p.N + 1, dp, xp, 1) == INV
        # v > 12 (width 8 leaves h = 7 of k = 20; width N leaves none of k = 13)
        assert scatter(h, s, zp, 20, 8, dp, xp, 1) == INV
        assert scatter(h, s, zp, 13, e.p.N, dp, xp, 1) == INV
        # an address selector index >= S (S = 3)
        assert scatter(h, s, bad.ctypes.data_as(u32p), 3, 8, dp, xp, 1) == INV
        assert b"set's size" in lib.tfhe_gpu_last_error(h)
        # a set of another context and parameter set
        assert scatter(other.ctx.h, s, zp, 3, 8, dp, xp, 1) == INV
        assert b"another context" in lib.tfhe_gpu_last_error(other.ctx.h)
        # null arguments
        assert scatter(None, s, zp, 3, 8, dp, xp, 1) == INV
        assert scatter(h, None, zp, 3, 8, dp, xp, 1) == INV
        assert scatter(h, s, None, 3, 8, dp, xp, 1) == INV
        assert scatter(h, s, zp, 3, 8, None, xp, 1) == INV
        assert scatter(h, s, zp, 3, 8, dp, None, 1) == INV
        # no queries: TFHE_OK, and the table is not touched
        assert scatter(h, s, None, 3, 8, None, xp, 0) == 0
    assert np.array_equal(x, keep)
    # a valid call succeeds afterwards
    table, deltas, addr, want5, _ = tree_case(oracle)
    assert np.array_equal(e.ctx.packed_scatter_add(e.set, addr[:5], 256, deltas[:5], table), want5)
    # the Python surface refuses a table of the wrong size before the call
    with pytest.raises(ValueError):
        e.ctx.packed_scatter_add(e.set, np.zeros((1, 8), np.uint32), 8, d, x[:1])


# ---- 9. the real 128-bit set: set semantics through lookup, bootstrap, pack and scatter-add ---------
def test_packed_write_chain_at_128(oracle, keys128):
    """A 16-entry table of 4-bit words in one TRLWE (k = 4, width 4), 3 distinct addresses written in one call
    with new values from sk.encrypt_bool; all 16 entries read back decrypt to the model.  The largest
    |phase - ideal| over the table's 64 coefficients after the write is printed (DESIGN.md §4.8c states it:
    0.0214 on a written entry, 0.0056 on the others, against the margin of 0.125)."""
    k = keys128
    ctx = tfhe_amd.Context("128", 0)
    ctx.load_cloud_key(k.ck.offset, k.ck.testvec, k.ck.bk, k.ck.ksk)
    p = ctx.params
    sk = tfhe_amd.SecretKey(p, k.k0, k.k1)
    rows, basebit, t = tfhe_amd.PackingKey.generate_rows(ctx, sk, 9000, basebit=2, t=8)
    key = tfhe_amd.PackingKey(ctx, rows, basebit, t)
    g = rng(860)
    model = g.integers(0, 16, 16).astype(np.uint64)
    table = tfhe_amd.lookup_table_pack_slots(p, model, 4)
    assert table.shape == (1, 2048)
    trgsw = np.array([oracle.trgsw_encrypt_torus_fft(k.p, mu, k.p.alpha_bsk, k.k1, 950 + mu) for mu in (0, 1)])
    sel = tfhe_amd.TrgswSet(ctx, trgsw)
    where, what = [3, 12, 6], [int(model[3]) ^ 0xF, 0x0, 0x9]
    addr = np.array([[(a >> j) & 1 for j in range(4)] for a in where], np.uint32)
    bits = np.array([[(v >> c) & 1 for c in range(4)] for v in what], np.uint8).reshape(-1)
    new = sk.encrypt_bool(bits, 500).reshape(3, 4, p.n + 1)
    for a, v in zip(where, what):
        model[a] = v
    table = ctx.packed_write(sel, key, addr, 4, new, table)
    assert ctx.last_kernels() == "k_rotate_chain<3>"
    want_bits = np.array([[(int(v) >> c) & 1 for c in range(4)] for v in model], bool)
    ph = trlwe_phase(oracle, p.N, table[0], k.k1)[:64].reshape(16, 4)
    err = np.abs(ph - np.where(want_bits, 0.125, -0.125))
    print(f"packed_write at 128, k = 4, width 4, 3 writes: max |phase - ideal| = {err.max():.5f} "
          f"(written entries {err[where].max():.5f}, others {np.delete(err, where, axis=0).max():.5f})")
    every = np.array([[(q >> j) & 1 for j in range(4)] for q in range(16)], np.uint32)
    found = ctx.packed_lookup(sel, every, 4, table)
    lv0 = ctx.sample_extract(found, np.arange(4), key_switch=True)
    got = sk.decrypt_bool(lv0.reshape(-1, p.n + 1)).reshape(16, 4)
    assert np.array_equal(got, want_bits)
    sel.close()
    key.close()
    ctx.close()
