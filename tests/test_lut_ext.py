"""The extended LUT bootstrap on the device (include/tfhe_gpu.h "Extended LUT bootstrap"): the blind
rotation in Z[X]/(X^(N E) + 1) on E = 2^eta accumulator components (k_blind_rotate_ext<L, E>), which
gives the UINT4 key 5- and 6-bit digits.  Parity is word for word against the definition composed
from oracle.cmux and oracle.poly_mul_with_xk in reference-tree mode; there is no tolerance anywhere.
The decryption tests first prove from the key that every input survives the mod switch, so a wrong
digit blames the kernel."""
import numpy as np
import pytest

import tfhe_amd
from conftest import rng
from test_lut_circuit import combine, ctx_for

pytestmark = pytest.mark.gpu

N = 1024
_NOISE = dict(alpha_lv0=2.0e-5, alpha_lv1=2.0e-8, alpha_ksk=2.0e-5, alpha_bsk=2.0e-8)
# Synthetic small-n sets with the fields of uint4 (L = 1), 128 (L = 3) and l2small (L = 2), made the way
# tests/test_param_sets.py makes its synthetic sets.  n = 8: keygen and the key load pass there, and the
# definition costs 8 E oracle CMUXes per item.
SMALL = {
    "uint4": dict(n=8, N=1024, nbit=10, L=1, bgbit=22, basebit=5, iks_t=3, **_NOISE),
    "128": dict(n=8, N=1024, nbit=10, L=3, bgbit=6, basebit=2, iks_t=9, **_NOISE),
    "l2small": dict(n=8, N=1024, nbit=10, L=2, bgbit=6, basebit=3, iks_t=4, **_NOISE),
}
_SMALL, _CACHE = {}, {}


def small_ctx(oracle, name):
    """(context, oracle params, cloud key arrays) of a synthetic set, its seeded key loaded; cached."""
    if name not in _SMALL:
        from oracle import OracleParams
        p = OracleParams(**SMALL[name])
        k0, k1 = oracle.secret_key(p, 42)
        ck = oracle.cloud_key(p, 43, k0, k1)
        c = tfhe_amd.Context(tfhe_amd.make_params(SMALL[name]), 0)
        c.load_cloud_key(ck.offset, ck.testvec, ck.bk, ck.ksk)
        _SMALL[name] = (c, p, ck)
    return _SMALL[name]


def words(seed, *shape):
    return rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def mod_switch(w, eta):
    sh = 21 - eta
    return (int(w) + (1 << (sh - 1))) >> sh


def ext_rotate(oracle, comps, a, eta):
    """ext_rotate of the definition: output k = mulxk(c_{(k - r) mod E}, q + [k < r]), a = q E + r."""
    E = 1 << eta
    q, r = a >> eta, a & (E - 1)
    out = np.zeros_like(comps)
    for k in range(E):
        c, ex = comps[(k - r) % E], (q + (k < r)) % (2 * N)
        out[k, :N], out[k, N:] = oracle.poly_mul_with_xk(c[:N], ex), oracle.poly_mul_with_xk(c[N:], ex)
    return out


def blind_rotate_ext_ref(oracle, p, ck, x, tv, eta):
    """The definition: acc = ext_rotate(tv, b~), then n steps of cmux(BK_i; in0 = acc_k, in1 = rot_k)."""
    E = 1 << eta
    acc = ext_rotate(oracle, np.asarray(tv, np.uint32).reshape(E, 2 * N), 2 * N * E - mod_switch(x[p.n], eta), eta)
    for i in range(p.n):
        rot = ext_rotate(oracle, acc, mod_switch(x[i], eta), eta)
        acc = np.array([oracle.cmux(p, acc[k], rot[k], ck.bk[i], ck.offset) for k in range(E)])
    return acc


def crafted_inputs(n, eta, seed):
    """B = 5 TLWELv0 of n = 8 mask words: random ones, and the words at which the component permutation, the
    carry to the exponent 2N and the two barriers can go wrong."""
    E, sh, top = 1 << eta, 21 - eta, 2 * N << eta
    x = words(seed, 5, n + 1)
    at = lambda pos: (pos << sh) & 0xFFFFFFFF  # a word the mod switch sends to position pos
    x[1, 0], x[1, 1], x[1, n] = 0, 0xFFFFFFFF, 0  # a mask word 0; one that rounds to 2N E; b~ = 2N E
    for r in range(E):  # every residue r at q = 2N - 1: the k < r carry to 2N
        x[2, r] = at((2 * N - 1) * E + r)
    x[2, n] = at(5)  # b~ = 2N E - 5: r = 1 (E = 2), 3 (E = 4)
    for r in range(E):  # every residue at q = 0: the pure component permutation
        x[3, r] = at(r)
    x[3, n] = 0xFFFFFFFF  # rounds to 2N E: b~ = 0
    x[4, n] = at(top - 1)  # b~ = 1
    assert mod_switch(x[1, 1], eta) == top and mod_switch(x[3, n], eta) == top
    assert [mod_switch(x[2, r], eta) for r in range(E)] == [(2 * N - 1) * E + r for r in range(E)]
    assert (top - mod_switch(x[2, n], eta)) % E != 0 and top - mod_switch(x[4, n], eta) == 1
    return x


@pytest.mark.parametrize("eta", [1, 2])
@pytest.mark.parametrize("name", ["uint4", "128", "l2small"])
def test_blind_rotate_ext_is_the_definition(oracle, name, eta):
    """(a) All E accumulators of B = 5 items, word for word, at L = 1, 3 and 2."""
    oracle.set_fused(0)  # the reference's expression trees
    c, p, ck = small_ctx(oracle, name)
    E = 1 << eta
    tv = words(200 + eta, E, 2 * N)  # any a: both halves random
    x = crafted_inputs(p.n, eta, 210 + eta)
    got = c.blind_rotate_ext(eta, x, tv)
    assert got.shape == (5, E, 2 * N)
    assert c.last_kernels() == f"k_blind_rotate_ext<{p.L},{E}>", c.last_kernels()
    for i in range(5):
        want = blind_rotate_ext_ref(oracle, p, ck, x[i], tv, eta)
        bad = [k for k in range(E) if not np.array_equal(got[i, k], want[k])]
        assert not bad, (name, eta, i, bad)


def test_blind_rotate_ext_eta_zero_is_the_ordinary_entry(oracle):
    c, p, ck = small_ctx(oracle, "uint4")
    tv, x = words(220, 2 * N), words(221, 3, p.n + 1)
    assert np.array_equal(c.blind_rotate_ext(0, x, tv)[:, 0], c.blind_rotate_batch(x, tv))


@pytest.mark.parametrize("pname", ["uint4", "128"])
def test_eta_zero_is_lut_apply(oracle, pname):
    """(b) B = 7 nodes with combinations: a call with eta = 0 returns the words of lut_apply and runs its kernels."""
    c, k = ctx_for(oracle, pname)
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    g, m = rng(230), 16 if pname == "uint4" else 4
    pool = sk.encrypt_lwe_message(g.integers(0, m // 4, 5).astype(np.uint32), m, seed0=2310)
    nodes = [(i % 3, [(int(g.integers(0, 5)), int(g.integers(-2, 4))) for _ in range(i % 3)], (i % 2) << 28)
             for i in range(7)]
    tables = np.array([tfhe_amd.lut_generate(c.params, m, lambda x, j=j: ((j + 1) * x + j) % m) for j in range(3)])
    ls = tfhe_amd.LutSet(c, tables)
    try:
        want = c.lut_apply(ls, pool, nodes)
        kernels = c.last_kernels()
        assert np.array_equal(c.lut_apply_ext(ls, 0, pool, nodes), want)
        assert c.last_kernels() == kernels and "ext" not in kernels
    finally:
        ls.close()


def uint4_case(oracle):
    """B = 6 nodes at the real UINT4 set over two extended tables (eta = 2, m = 64): fresh 6-bit encryptions,
    one or two terms each, a constant on two of them."""
    if "c" not in _CACHE:
        c, k = ctx_for(oracle, "uint4")
        sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
        g = rng(240)
        pool = sk.encrypt_lwe_message(g.integers(0, 16, 5).astype(np.uint32), 64, seed0=2410)
        nodes = [((i * 3 + 1) % 2, [(int(g.integers(0, 5)), 1)] + ([(int(g.integers(0, 5)), 2)] if i % 2 else []),
                  (3 << 25) if i in (1, 4) else 0) for i in range(6)]
        tables = np.concatenate([tfhe_amd.lut_generate_ext(c.params, 2, 64, lambda x: (5 * x + 1) % 64),
                                 tfhe_amd.lut_generate_ext(c.params, 2, 64, lambda x: (x * x) % 16)])
        _CACHE["c"] = (pool, nodes, tables)
    return _CACHE["c"]


def test_full_path_at_uint4(oracle):
    """(c) n = 820, eta = 2, per-item tables: the host-buffer and the device-buffer forms both equal
    sample_extract(acc_0, 0, key_switch) of blind_rotate_ext over the host-combined x_i; one item's four
    accumulators also equal the definition on the oracle (820 steps)."""
    import torch
    oracle.set_fused(0)
    c, k = ctx_for(oracle, "uint4")
    pool, nodes, tables = uint4_case(oracle)
    assert tables.shape == (8, 2 * N) and {n[0] for n in nodes} == {0, 1}
    x = combine(pool, nodes)
    acc = np.zeros((6, 4, 2 * N), np.uint32)
    for t in (0, 1):
        sel = [i for i, n in enumerate(nodes) if n[0] == t]
        acc[sel] = c.blind_rotate_ext(2, x[sel], tables[4 * t:4 * t + 4])
    assert c.last_kernels() == "k_blind_rotate_ext<1,4>"
    want = c.sample_extract(acc[:, 0], [0], key_switch=True).reshape(6, c.n1)
    ls = tfhe_amd.LutSet(c, tables)
    try:
        got = c.lut_apply_ext(ls, 2, pool, nodes)
        assert c.last_kernels().startswith("k_blind_rotate_ext<1,4> + k_key_switch"), c.last_kernels()
        assert np.array_equal(got, want)
        t_pool = torch.from_numpy(np.ascontiguousarray(pool).view(np.int32)).to("cuda:0")
        t_out = torch.zeros((6, c.n1), dtype=torch.int32, device="cuda:0")
        try:
            c.set_stream(torch.cuda.current_stream().cuda_stream)
            c.lut_apply_ext_dev(ls, 2, t_pool.data_ptr(), pool.shape[0], nodes, t_out.data_ptr())
            c.sync()
        finally:
            c.set_stream(None)
        assert np.array_equal(t_out.cpu().numpy().view(np.uint32), want)
    finally:
        ls.close()
    ref = blind_rotate_ext_ref(oracle, k.p, k.ck, x[1], tables[4 * nodes[1][0]:4 * nodes[1][0] + 4], 2)
    assert np.array_equal(acc[1], ref)


def phases(cts, key):
    """b - sum a_i s_i of every ciphertext, as a fraction of the torus in [0, 1)."""
    s = key.astype(np.uint64)
    return ((cts[:, -1].astype(np.uint64) - cts[:, :-1].astype(np.uint64) @ s) & 0xFFFFFFFF) / 2.0 ** 32


def rounded_phases(cts, key, eta):
    """The phase the blind rotation sees: (b~ - sum a~_i s_i) / (2N E) mod 1, from the key."""
    sh = 21 - eta
    r = (cts.astype(np.uint64) + (1 << (sh - 1))) >> sh
    return (((r[:, -1] - r[:, :-1] @ key.astype(np.uint64)) << sh) & 0xFFFFFFFF) / 2.0 ** 32


def centred(d):
    return (d + 0.5) % 1.0 - 0.5


def check_inputs_survive(cts, msgs, m, key, eta):
    err = centred(rounded_phases(cts, key, eta) - msgs / (2.0 * m))
    assert np.abs(err).max() < 1.0 / (4 * m), ("an input leaves its block in the mod switch: choose another seed",
                                               float(np.abs(err).max()))
    return err


@pytest.mark.parametrize("m,eta", [(64, 2), (32, 1)])
def test_six_and_five_bit_digits_decrypt(oracle, m, eta):
    """(d) Every message x 4 encryptions through f = identity and f = (7x + 3) mod m, at the real UINT4 key:
    all decrypt to f(x).  The inputs' rounded phases are first checked against the half-spacing 1/(4m) from the
    key.  Measured on the MI355X (this test prints it): the outputs' phase error has sigma 7.5e-4 / 7.6e-4 of the
    torus and max 2.4e-3 over the 256 outputs at m = 64, eta = 2 (half-spacing 3.9e-3), and sigma 7.1e-4 / 7.5e-4,
    max 2.1e-3 at m = 32, eta = 1 (half-spacing 7.8e-3)."""
    c, k = ctx_for(oracle, "uint4")
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    E = 1 << eta
    fs = [lambda x: x, lambda x: (7 * x + 3) % m]
    tables = np.concatenate([tfhe_amd.lut_generate_ext(c.params, eta, m, f) for f in fs])
    msgs = np.repeat(np.arange(m, dtype=np.uint32), 4)
    cts = sk.encrypt_lwe_message(msgs, m, seed0=2500 + m)
    check_inputs_survive(cts, msgs, m, k.k0, eta)
    ls = tfhe_amd.LutSet(c, tables)
    try:
        for j, f in enumerate(fs):
            out = c.lut_apply_ext(ls, eta, cts, [(j, [(i, 1)], 0) for i in range(len(msgs))])
            assert c.last_kernels().startswith(f"k_blind_rotate_ext<1,{E}>")
            want = np.array([f(int(x)) for x in msgs], np.uint32)
            err = centred(phases(out, k.k0) - want / (2.0 * m))
            print(f"m = {m}, eta = {eta}, f{j}: output phase error sigma {err.std():.3e}, max {np.abs(err).max():.3e} "
                  f"of the torus; half-spacing {1 / (4 * m):.3e}")
            wrong = np.flatnonzero(sk.decrypt_lwe_message(out, m) != want)
            assert wrong.size == 0, (j, msgs[wrong].tolist())
    finally:
        ls.close()


def test_chain_of_two_bootstraps(oracle):
    """(d) m = 32, eta = 2: the output of one extended bootstrap is the input of the next; every message
    decrypts to f2(f1(x)).  The second stage's inputs are checked from the key like the first's."""
    c, k = ctx_for(oracle, "uint4")
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    m, eta = 32, 2
    f1, f2 = (lambda x: (5 * x + 2) % m), (lambda x: (x * x + 1) % m)
    tables = np.concatenate([tfhe_amd.lut_generate_ext(c.params, eta, m, f) for f in (f1, f2)])
    msgs = np.arange(m, dtype=np.uint32)
    cts = sk.encrypt_lwe_message(msgs, m, seed0=2600)
    check_inputs_survive(cts, msgs, m, k.k0, eta)
    nodes = lambda t: [(t, [(i, 1)], 0) for i in range(m)]
    ls = tfhe_amd.LutSet(c, tables)
    try:
        mid = c.lut_apply_ext(ls, eta, cts, nodes(0))
        mid_want = np.array([f1(int(x)) for x in msgs], np.uint32)
        check_inputs_survive(mid, mid_want, m, k.k0, eta)
        out = c.lut_apply_ext(ls, eta, mid, nodes(1))
    finally:
        ls.close()
    assert sk.decrypt_lwe_message(mid, m).tolist() == mid_want.tolist()
    assert sk.decrypt_lwe_message(out, m).tolist() == [f2(f1(int(x))) for x in msgs]


def test_refusals_and_empty_calls(oracle):
    """(e) Every refusal returns its status before any launch, B = 0 is OK, and the context still works."""
    import torch
    c, k = ctx_for(oracle, "uint4")
    pool, nodes, tables = uint4_case(oracle)
    P = len(pool)
    ls = tfhe_amd.LutSet(c, tables)  # 8 entries: two extended tables at eta = 2, four at eta = 1
    other = tfhe_amd.Context("uint4", 0)  # no key, and a set of its own
    multi = tfhe_amd.Context.multi("uint4", devices=[0, 0])
    try:
        ls_other, ls_multi = tfhe_amd.LutSet(other, tables), tfhe_amd.LutSet(multi, tables)

        def status(call):
            with pytest.raises(tfhe_amd.TfheError) as e:
                call()
            return e.value.status

        INVALID = tfhe_amd.ERR_INVALID
        t = torch.zeros((len(nodes), c.n1), dtype=torch.int32, device="cuda:0")
        assert status(lambda: c.lut_apply_ext(ls, 3, pool, nodes)) == INVALID  # eta > 2
        assert status(lambda: c.lut_apply_ext_dev(ls, 3, t.data_ptr(), P, nodes, t.data_ptr())) == INVALID
        assert status(lambda: c.blind_rotate_ext(3, pool, np.zeros((8, 2 * N), np.uint32))) == INVALID
        beyond = nodes[:3] + [(2, nodes[3][1], 0)] + nodes[4:]  # lut * E + E = 12 > 8
        assert status(lambda: c.lut_apply_ext(ls, 2, pool, beyond)) == INVALID
        edge = nodes[:3] + [(3, nodes[3][1], 0)] + nodes[4:]  # eta = 1: table 3 is entries 6, 7, the last
        assert c.lut_apply_ext(ls, 1, pool, edge).shape == (6, c.n1)
        assert status(lambda: c.lut_apply_ext(ls, 1, pool, nodes[:3] + [(4, nodes[3][1], 0)])) == INVALID
        bad_src = nodes[:2] + [(0, [(P, 1)], 0)]
        assert status(lambda: c.lut_apply_ext(ls, 2, pool, bad_src)) == INVALID
        assert status(lambda: c.lut_apply_ext(ls_other, 2, pool, nodes)) == INVALID  # another context's set
        assert status(lambda: other.lut_apply_ext(ls_other, 2, pool, nodes)) == tfhe_amd.ERR_NO_KEY
        assert status(lambda: other.blind_rotate_ext(2, pool, tables[:4])) == tfhe_amd.ERR_NO_KEY
        assert status(lambda: multi.lut_apply_ext_dev(ls_multi, 2, t.data_ptr(), P, nodes, t.data_ptr())) == INVALID
        # empty calls are no-ops, without a key too
        assert c.lut_apply_ext(ls, 2, pool, []).shape == (0, c.n1)
        assert other.lut_apply_ext(ls_other, 2, pool, []).shape == (0, c.n1)
        assert c.blind_rotate_ext(2, np.zeros((0, c.n1), np.uint32), tables[:4]).shape == (0, 4, 2 * N)
        # and the context still works
        got = c.lut_apply_ext(ls, 2, pool, nodes)
        assert c.last_kernels().startswith("k_blind_rotate_ext<1,4>")
        acc = c.blind_rotate_ext(2, combine(pool, nodes)[:1], tables[4 * nodes[0][0]:4 * nodes[0][0] + 4])
        assert np.array_equal(got[0], c.sample_extract(acc[:, 0], [0], key_switch=True).reshape(-1))
    finally:
        ls.close()
        other.close()
        multi.close()
