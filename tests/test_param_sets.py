"""GPU parity at the parameter sets params_ok accepts beyond "128", "80" and "uint4": the
reference's SECURITY_110_BIT, UINT1 (L = 2), UINT2 and UINT3, and three synthetic sets that reach
the instantiations no reference set reaches (the fused L = 2 kernels, the (4,3), (4,4) and (2,5)
key-switch shapes, n = 1024).  Every comparison is np.array_equal against the oracle's restatement
of the reference on the same seeded inputs; there is no tolerance anywhere.  Where the kernel
choice is the point, last_kernels() is asserted (DESIGN.md §6.3 lists instantiation -> test).

The oracle costs tens of milliseconds per blind rotation, so every case compares at most ~16
items with it, and keys, contexts and references are computed once per module."""
import numpy as np
import pytest

import tfhe_amd
from conftest import crafted_near_tie_case, get_keys, rng
from test_leveled import FORMS, env, expected_kernels, lookup_addresses, oracle_lookup
from test_lut_circuit import combine, oracle_nodes

pytestmark = pytest.mark.gpu

REFERENCE_SETS = ["110", "uint1", "uint2", "uint3"]
# Test-only sets (plain dicts: not in the libraries' tables).  Messages do not survive l2small's 12
# gadget bits: nothing is decrypted at these sets, bit-exactness only.
_NOISE = dict(alpha_lv0=2.0e-5, alpha_lv1=2.0e-8, alpha_ksk=2.0e-5, alpha_bsk=2.0e-8)
SYNTHETIC = {
    # small_products() holds at L = 2 only with bgbit 6: the fused <2,true,true> kernels, the SMALL
    # reference trees <2,true,false> and the margin guard's recompute at L = 2
    "l2small": dict(n=600, N=1024, nbit=10, L=2, bgbit=6, basebit=3, iks_t=4, **_NOISE),
    "ks44": dict(n=500, N=1024, nbit=10, L=1, bgbit=22, basebit=4, iks_t=4, **_NOISE),
    # the accepted upper edge of n
    "ks25_nmax": dict(n=1024, N=1024, nbit=10, L=1, bgbit=22, basebit=5, iks_t=2, **_NOISE),
}
COPY = 255
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
TRUTH = {0: lambda a, b: ~(a & b), 1: lambda a, b: a | b, 2: lambda a, b: a & b, 3: lambda a, b: a ^ b,
         4: lambda a, b: a ^ b,  # the reference's xnorGate decrypts as XOR (test_oracle.py)
         5: lambda a, b: ~(a | b), 6: lambda a, b: ~a & b, 7: lambda a, b: a & ~b, 8: lambda a, b: ~a | b,
         9: lambda a, b: a | ~b, COPY: lambda a, b: a}


def u32rand(g, *shape):
    return g.integers(0, 1 << 32, shape, dtype=np.uint32)


class SyntheticKeys:
    """What conftest.Keys holds, for a set given as a dict.  keygen = False (ks44, a pure key-switch
    set): a KSK of uniform random words, as good as a generated one under wrapping integer
    arithmetic, and a zero BK that no test here rotates with."""

    def __init__(self, oracle, name, keygen):
        from oracle import CloudKeyArrays, OracleParams
        self.name, self.p = name, OracleParams(**SYNTHETIC[name])
        p = self.p
        self.k0, self.k1 = oracle.secret_key(p, 42)
        if keygen:
            self.ck = oracle.cloud_key(p, 43, self.k0, self.k1)
        else:
            ksk = u32rand(rng(4300 + p.n), p.N * p.iks_t * (1 << p.basebit), p.n + 1)
            self.ck = CloudKeyArrays(oracle.decomposition_offset(p), oracle.testvec(p), ksk,
                                     np.zeros((p.n, 2 * p.L, 2, p.N)))


_CTX, _CACHE = {}, {}


def ctx_for(oracle, name):
    """(context with the set's seeded cloud key loaded, its keys), cached for the module."""
    if name not in _CTX:
        if name in SYNTHETIC:
            k = SyntheticKeys(oracle, name, keygen=name != "ks44")
            c = tfhe_amd.Context(tfhe_amd.make_params(SYNTHETIC[name]), 0)
        else:
            k = get_keys(oracle, name)
            c = tfhe_amd.Context(name, 0)
        c.load_cloud_key(k.ck.offset, k.ck.testvec, k.ck.bk, k.ck.ksk)
        _CTX[name] = (c, k)
    return _CTX[name]


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def test_params_ok_accepts_every_set_used_here():
    """The sets are the C ABI's to accept: a context exists for each (tfhe_gpu_create runs
    params_ok), and the two Python tables name the same numbers."""
    from oracle import PARAM_SETS
    for name in REFERENCE_SETS:
        assert PARAM_SETS[name] == tfhe_amd.PARAM_SETS[name], name
    for name in REFERENCE_SETS + list(SYNTHETIC):
        c = tfhe_amd.Context(tfhe_amd.make_params(SYNTHETIC.get(name, name)), 0)
        c.close()


# ---- external product (trgsw.zig) ---------------------------------------------
@pytest.mark.parametrize("pname", ["uint1", "l2small", "110"])
def test_external_product_vs_oracle(oracle, pname):
    """k_external_product<2> (uint1: Bg = 2^10, l2small: Bg = 2^6) and <3> at n = 630: 8 items against
    a fresh TRGSW and against a row of the resident key."""
    c, k = ctx_for(oracle, pname)
    p = k.p
    x = u32rand(rng(4), 8, 2048)
    trgsw = oracle.trgsw_encrypt_torus_fft(p, 1, p.alpha_bsk, k.k1, 17)
    want = np.array([oracle.external_product(p, trgsw, t, k.ck.offset) for t in x])
    assert np.array_equal(c.external_product(x, trgsw_fft=trgsw), want)
    want = np.array([oracle.external_product(p, k.ck.bk[p.n - 1], t, k.ck.offset) for t in x])
    assert np.array_equal(c.external_product(x, bk_index=p.n - 1), want)


# ---- key switch: every form that exists for the shape -------------------------
KS_BIG = 1027  # three 512-item GEMM workgroup rows, the last with 3 items


def ks_case(oracle, pname, B):
    """(inputs, oracle outputs) of a key-switch batch; for B = KS_BIG the oracle on four probe items."""
    def make():
        _, k = ctx_for(oracle, pname)
        lv1 = u32rand(rng(500 + B), B, 1025)
        probe = [0, 511, 512, B - 1] if B == KS_BIG else range(B)
        return lv1, {i: oracle.identity_key_switch(k.p, lv1[i], k.ck.ksk) for i in probe}
    return cached(("ks", pname, B), make)


def check_ks(c, case, opts, name):
    lv1, want = case
    with c.options(**opts):
        got = c.key_switch(lv1)
        assert name in c.last_kernels(), (name, c.last_kernels())
    for i, w in want.items():
        assert np.array_equal(got[i], w), i
    return got


SEL_FORMS = {"lanes": (dict(ks_form=0), "k_key_switch_lanes<8,2,"),
             "lanes-narrow": (dict(ks_form=0, ks_narrow=1), "k_key_switch_lanes<8,2,32,4,1>"),
             "sel": (dict(ks_form=1), "k_key_switch_sel"),
             "gemm": (dict(ks_form=2), "k_key_switch_gemm<8,2>")}


@pytest.mark.parametrize("form", list(SEL_FORMS))
@pytest.mark.parametrize("pname,B", [("110", 1), ("110", 130), ("uint1", 1), ("uint1", 67)])
def test_key_switch_8_2(oracle, pname, B, form):
    """(t, basebit) = (8, 2) at n = 630 and n = 700: the lane form in wide / narrow blocks, the
    select form and the one-hot GEMM (8 levels per coefficient block, 20 / 22 output tiles)."""
    c, _ = ctx_for(oracle, pname)
    opts, name = SEL_FORMS[form]
    check_ks(c, ks_case(oracle, pname, B), opts, name)


GATHER_SHAPES = {"uint2": (3, 4), "l2small": (4, 3), "ks44": (4, 4)}


@pytest.mark.parametrize("form", ["lanes", "gather"])
@pytest.mark.parametrize("B", [1, 77])
@pytest.mark.parametrize("pname", list(GATHER_SHAPES))
def test_key_switch_gather_shapes(oracle, pname, B, form):
    """(3,4) at UINT2, (4,3) and (4,4): the lane form's instantiation of the shape and the gather
    form (ks_form = 1)."""
    c, _ = ctx_for(oracle, pname)
    t, bb = GATHER_SHAPES[pname]
    opts, name = {"lanes": (dict(ks_form=0), f"k_key_switch_lanes<{t},{bb},32,4,1>"),
                  "gather": (dict(ks_form=1), "k_key_switch_gather")}[form]
    check_ks(c, ks_case(oracle, pname, B), opts, name)
    if form == "lanes":  # auto has no GEMM at these shapes: the same lane kernel
        check_ks(c, ks_case(oracle, pname, B), dict(ks_form=3), name)


NMAX_FORMS = {"lanes": (dict(ks_form=0, ks_item_groups=1), "k_key_switch_lanes<2,5,32,4,1>"),
              "ring": (dict(ks_form=0, ks_item_groups=0), "k_key_switch_ring<2,5,32,4,4>"),
              "groups2": (dict(ks_form=0, ks_item_groups=2), "k_key_switch_lanes<2,5,32,4,2>"),
              "groups4": (dict(ks_form=0, ks_item_groups=4), "k_key_switch_lanes<2,5,32,4,4>"),
              "gather": (dict(ks_form=1), "k_key_switch_gather"),
              "gemm": (dict(ks_form=2), "k_key_switch_gemm<2,5>"),
              "auto": (dict(), "k_key_switch_gemm<2,5>")}


@pytest.mark.parametrize("form", list(NMAX_FORMS))
@pytest.mark.parametrize("B", [1, 200])
def test_key_switch_2_5_at_n_1024(oracle, B, form):
    """(2, 5) at the accepted upper edge n = 1024 (1,025 output words: 33 chunks / tiles, the last
    one holding the b word alone; 1,028-word KSK rows): the lane form, the ring form and the lane
    form with 2 and 4 item groups (above 64 items; a single item runs the plain lane kernel),
    gather, and the GEMM."""
    c, _ = ctx_for(oracle, "ks25_nmax")
    opts, name = NMAX_FORMS[form]
    if B <= 64 and form in ("ring", "groups2", "groups4"):
        name = "k_key_switch_lanes<2,5,32,4,1>"
    check_ks(c, ks_case(oracle, "ks25_nmax", B), opts, name)


@pytest.mark.parametrize("pname,name", [("110", "k_key_switch_gemm<8,2>"), ("uint1", "k_key_switch_gemm<8,2>"),
                                        ("ks25_nmax", "k_key_switch_gemm<2,5>")])
def test_key_switch_gemm_full_batches(oracle, pname, name):
    """The GEMM shapes at 1,027 items (three 512-item workgroup rows, the last ragged): the oracle on
    four probe items, the lane form on all of them."""
    c, _ = ctx_for(oracle, pname)
    case = ks_case(oracle, pname, KS_BIG)
    lanes = check_ks(c, case, dict(ks_form=0), "k_key_switch_")
    got = check_ks(c, case, dict(ks_form=2), name)
    assert np.array_equal(got, lanes)


@pytest.mark.parametrize("ks_form", [0, 1, 2, 3])
@pytest.mark.parametrize("B", [1, 70])
def test_key_switch_basebit_6_is_the_gather_form(oracle, B, ks_form):
    """UINT3's (2, 6) has no lane or GEMM instantiation.  include/tfhe_gpu.h documents
    TFHE_OPT_KS_FORM 2 and 3 as falling back where the GEMM does not apply, and 0 as a choice
    among the forms the shape has: every value ends in k_key_switch_gather<2> (KS_ANY_BASEBIT)
    with the oracle's words and no error status."""
    c, _ = ctx_for(oracle, "uint3")
    check_ks(c, ks_case(oracle, "uint3", B), dict(ks_form=ks_form), "k_key_switch_gather")
    assert "lanes" not in c.last_kernels() and "gemm" not in c.last_kernels()


# ---- blind rotation -------------------------------------------------------------
def br_case(oracle, pname):
    """8 uniform TLWEs (bit-exactness only) and the oracle's rotations of them."""
    def make():
        _, k = ctx_for(oracle, pname)
        cts = u32rand(rng(600), 8, k.p.n + 1)
        return cts, np.array([oracle.blind_rotate(k.p, t, k.ck.testvec, k.ck.bk, k.ck.offset) for t in cts])
    return cached(("br", pname), make)


BR_NAMES = {
    # (whole, whole-reference, wide, wide-reference)
    "uint1": ("k_blind_rotate<2,false,false> (whole form)", "k_blind_rotate<2,false,false> (whole form)",
              "k_blind_rotate_wide<2,false,false> (latency form)", "k_blind_rotate_wide<2,false,false> (latency form)"),
    "l2small": ("k_blind_rotate<2,true,true> (whole form, fused)", "k_blind_rotate<2,true,false> (whole form)",
                "k_blind_rotate_wide<2,true,true> (latency form, fused)",
                "k_blind_rotate_wide<2,true,false> (latency form)"),
    "110": ("k_blind_rotate_assist<true> (whole form, loader waves own polynomial b, fused)",
            "k_blind_rotate<3,true,false> (whole form)", "k_blind_rotate_wide<3,true,true> (latency form, fused)",
            "k_blind_rotate_wide<3,true,false> (latency form)"),
    "uint2": ("k_blind_rotate<1,false,false> (whole form)", "k_blind_rotate<1,false,false> (whole form)",
              "k_blind_rotate_wide<1,false,false> (latency form)", "k_blind_rotate_wide<1,false,false> (latency form)"),
}
BR_NAMES["uint3"] = BR_NAMES["uint2"]
BR_FORMS = ["whole", "whole-reference", "wide", "wide-reference", "octo", "octo-reference"]


@pytest.mark.parametrize("form", BR_FORMS)
@pytest.mark.parametrize("pname", list(BR_NAMES))
def test_blind_rotate_vs_oracle(oracle, pname, form):
    """Every product form x {default arithmetic, arith = reference} at B = 3 and B = 5 (idle item
    slots in the whole and octo forms).  UINT1 (Bg = 2^10) is outside the exact-integer regime and
    never fuses; l2small (Bg = 2^6) runs the fused L = 2 kernels under an admitted keygen'd key;
    the 110-bit set is the assist form at n = 630; the octo form exists at L = 1 only."""
    c, k = ctx_for(oracle, pname)
    kind, ref = form.split("-")[0], form.endswith("reference")
    if kind == "octo" and k.p.L != 1:
        with pytest.raises(tfhe_amd.TfheError, match="L = 1 only"):
            c.set_option("br_form", "octo")
        assert c.get_option("br_form") == 0
        return
    cts, want = br_case(oracle, pname)
    if pname in ("l2small", "110"):
        assert c.get_option("fused_admitted") == 1
    if kind == "octo":
        name = "k_blind_rotate_octo<1,false,false> (octo form)"
    else:
        name = BR_NAMES[pname][2 * (kind == "wide") + ref]
    with c.options(br_form=kind, arith=int(ref)):
        for lo, hi in ((0, 3), (3, 8)):
            assert np.array_equal(c.blind_rotate_batch(cts[lo:hi]), want[lo:hi]), (lo, hi)
            assert c.last_kernels().split(" + ")[0] == name
    if pname == "uint1":
        assert "fused)" not in name


@pytest.mark.parametrize("pname", ["uint1", "l2small"])
def test_whole_form_every_idle_slot_count_at_l2(oracle, pname):
    """The L = 2 whole form at B = 1..8: 3, 2, 1 or 0 idle gate slots in the last workgroup."""
    c, _ = ctx_for(oracle, pname)
    cts, want = br_case(oracle, pname)
    with c.options(br_form="whole"):
        for B in range(1, 9):
            assert np.array_equal(c.blind_rotate_batch(cts[:B]), want[:B]), B
        assert c.last_kernels().startswith("k_blind_rotate<2,")


@pytest.mark.parametrize("pname,form", [("110", "whole"), ("110", "wide"), ("uint2", "whole"), ("uint2", "octo")])
def test_bootstrap_without_key_switch(oracle, pname, form):
    """The hybrid sampleExtractIndex2's n - j indexing at n = 630 and n = 687 (neither a multiple
    of 64; the assist form writes word n from its loader wave)."""
    c, k = ctx_for(oracle, pname)
    cts = br_case(oracle, pname)[0][:3]
    want = cached(("bwks", pname), lambda: np.array([oracle.bootstrap_without_key_switch(k.p, t, k.ck) for t in cts]))
    with c.options(br_form=form):
        assert np.array_equal(c.bootstrap_without_key_switch_batch(cts), want)


def test_bootstraps_at_n_1024(oracle):
    """The accepted upper edge n = 1024 through the blind rotation (1,024 CMUX steps: every entry of
    the a~ table in LDS is used), the hybrid sampleExtractIndex2 (j < n: -acc[n - j] reaches acc[1]
    .. acc[1023]; word n = acc[N]) in the three forms, the full bootstrap, and a two-level LUT circuit
    whose combination and output gather move 1,025 words per wire."""
    c, k = ctx_for(oracle, "ks25_nmax")
    p = k.p
    cts = u32rand(rng(1024), 5, p.n + 1)
    want = np.array([oracle.bootstrap_without_key_switch(p, t, k.ck) for t in cts])
    for form in ("whole", "wide", "octo"):
        with c.options(br_form=form):
            assert np.array_equal(c.bootstrap_without_key_switch_batch(cts), want), form
    assert np.array_equal(c.bootstrap_batch(cts[:3]), np.array([oracle.bootstrap(p, t, k.ck) for t in cts[:3]]))
    assert c.last_kernels() == "k_blind_rotate_wide<1,false,false> (latency form) + k_key_switch_gemm<2,5> + k_ks_gemm_reduce"
    tables = np.array([tfhe_amd.lut_generate(c.params, 16, lambda x, j=j: ((j + 1) * x + j) % 16) for j in range(2)])
    circ = tfhe_amd.LutCircuit()
    a, b = circ.input(), circ.input()
    n0 = circ.node(0, [(a, 1), (b, -1)], const=1 << 27)
    circ.node(1, [(n0, I32_MAX), (a, I32_MIN), (b, 3)])
    circ.output(3, 0, 2)
    wires = np.zeros((4, c.n1), np.uint32)
    wires[:2] = cts[:2]
    for i in (0, 1):
        wires[2 + i] = oracle_nodes(oracle, p, k.ck, wires, [circ.nodes[i]], tables)[0]
    ls = tfhe_amd.LutSet(c, tables)
    try:
        got, ran = circ.run(c, ls, cts[:2])
    finally:
        ls.close()
    assert ran == 2 and np.array_equal(got, wires[[3, 0, 2]])


@pytest.mark.parametrize("form", ["auto", "whole"])
def test_margin_guard_recomputes_near_ties_at_l2(oracle, form):
    """test_margin_guard_recomputes_near_ties at L = 2 (l2small, zero KSK): under the crafted key the
    oracle's fused mode parts from its reference mode.  The key admission refuses
    this key the fused arithmetic by default (its BK spectrum is 2^41.3 > 2^39), so the default runs
    the reference's trees and recomputes nothing; forced fused arithmetic flags the items, the
    recompute launch br_kernel('w', 2, true, false) redoes them (near_tie_items rises) and every
    output equals the oracle's reference-mode words."""
    from oracle import OracleParams
    p = OracleParams(**SYNTHETIC["l2small"])
    tv, bk, ct = crafted_near_tie_case(oracle, p)
    off = oracle.decomposition_offset(p)
    cts = np.concatenate([u32rand(rng(4242), 2, p.n + 1), ct[None], u32rand(rng(4243), 3, p.n + 1)])

    def modes():
        out = []
        try:
            for mode in (0, 1):
                oracle.set_fused(mode)
                out.append(np.array([oracle.blind_rotate(p, x, tv, bk, off) for x in cts]))
        finally:
            oracle.set_fused(0)
        return out
    want, fused = cached("near_tie_l2", modes)
    parted = int((fused != want).any(axis=1).sum())
    assert not np.array_equal(fused[2], want[2]) and parted >= 1
    ksk = np.zeros((p.N * p.iks_t * (1 << p.basebit), p.n + 1), np.uint32)
    c = tfhe_amd.Context(tfhe_amd.make_params(SYNTHETIC["l2small"]), 0)
    try:
        c.load_cloud_key(off, tv, bk, ksk)
        assert c.get_option("fused_admitted") == 0
        before = c.near_tie_items()
        with c.options(br_form=form):
            assert np.array_equal(c.blind_rotate_batch(cts, tv), want)
            assert not c.last_kernels().split(" + ")[0].endswith("fused)")
        assert c.near_tie_items() == before
        with c.options(br_form=form, arith=tfhe_amd.ARITH_FUSED_FORCED):
            got = c.blind_rotate_batch(cts, tv)
            fused_name = {"auto": "k_blind_rotate_wide<2,true,true> (latency form, fused)",
                          "whole": "k_blind_rotate<2,true,true> (whole form, fused)"}[form]
            assert c.last_kernels().split(" + ")[0] == fused_name
        assert parted <= c.near_tie_items() - before <= len(cts)
        assert np.array_equal(got, want)
    finally:
        c.close()


# ---- gates and bootstraps end to end ------------------------------------------------
@pytest.mark.parametrize("pname", REFERENCE_SETS)
def test_all_ops_bit_exact(oracle, pname):
    """13 items: the ten gates, COPY, and muxNaive's two ANDs (a AND b, NOT a AND c), then its OR
    over the device's own outputs.  Bit-exact at every reference set; at the 110-bit and UINT1 sets
    (the boolean ones) every output decrypts to its truth table too."""
    c, k = ctx_for(oracle, pname)
    p = k.p
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    g = rng(7)
    ops = np.array(list(range(10)) + [COPY, tfhe_amd.AND, tfhe_amd.AND], np.uint8)
    a_bits, b_bits = g.integers(0, 2, 13).astype(bool), g.integers(0, 2, 13).astype(bool)
    A = sk.encrypt_bool(a_bits.astype(np.uint8), seed0=100)
    B = sk.encrypt_bool(b_bits.astype(np.uint8), seed0=200)
    A[12], a_bits[12] = tfhe_amd.Gates.not_gate(A[11]), ~a_bits[11]  # muxNaive's NOT a
    got = c.gate_batch(ops, A, B)
    assert np.array_equal(got, oracle.gate_batch(p, ops, A, B, k.ck, threads=8))
    mux = c.gate_batch(np.array([tfhe_amd.OR], np.uint8), got[11:12], got[12:13])
    assert np.array_equal(mux, oracle.gate_batch(p, np.array([tfhe_amd.OR], np.uint8), got[11:12], got[12:13], k.ck))
    if pname in ("110", "uint1"):
        want = np.array([TRUTH[int(o)](x, y) for o, x, y in zip(ops, a_bits, b_bits)], bool)
        assert np.array_equal(sk.decrypt_bool(got), want)
        assert sk.decrypt_bool(mux)[0] == (b_bits[11] if a_bits[11] else b_bits[12])


@pytest.mark.parametrize("pname,m", [("uint2", 4), ("uint3", 8), ("uint1", 2)])
def test_lut_pbs(oracle, pname, m):
    """f(x) = (x + 1) mod m over every message, twice: bit-exact on all 2m items, and every one
    decrypts to f(message)."""
    c, k = ctx_for(oracle, pname)
    tv = tfhe_amd.lut_generate(c.params, m, lambda x: (x + 1) % m)
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    msgs = np.tile(np.arange(m, dtype=np.uint32), 2)
    cts = sk.encrypt_lwe_message(msgs, m, seed0=77)
    out = c.bootstrap_lut_batch(cts, tv)
    want = oracle.gate_batch(k.p, np.full(len(cts), COPY, np.uint8), cts, cts, k.ck, threads=8, testvec=tv)
    assert np.array_equal(out, want)
    assert np.array_equal(sk.decrypt_lwe_message(out, m), (msgs + 1) % m)


def test_auto_plan_tail_split_at_l2(oracle):
    """UINT1, B = 4 x CUs + 3 gates: blind_rotate_plan's PLAN_WHOLE_TAIL, the full rounds in
    k_blind_rotate<2,false,false> and the 3-item tail in the latency form.  The oracle on the items
    around the split and on the last one; the whole batch equals the same call forced to the whole
    form; every gate decrypts."""
    import torch
    c, k = ctx_for(oracle, "uint1")
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    full, B = 4 * cus, 4 * cus + 3
    g = rng(1303)
    ops = g.integers(0, 10, B).astype(np.uint8)
    a_bits, b_bits = g.integers(0, 2, B).astype(bool), g.integers(0, 2, B).astype(bool)
    A = sk.encrypt_bool(a_bits.astype(np.uint8), seed0=30_000)
    Bc = sk.encrypt_bool(b_bits.astype(np.uint8), seed0=40_000)
    got = c.gate_batch(ops, A, Bc)
    assert c.last_kernels() == "k_blind_rotate<2,false,false> (whole form) + k_key_switch_gemm<8,2> + k_ks_gemm_reduce"
    with c.options(br_form="whole"):
        whole = c.gate_batch(ops, A, Bc)
    bad = np.flatnonzero((got != whole).any(axis=1))
    assert bad.size == 0, bad[:10].tolist()
    probe = np.array([0, full - 1, full, full + 1, B - 1])
    assert np.array_equal(got[probe], oracle.gate_batch(k.p, ops[probe], A[probe], Bc[probe], k.ck, threads=5))
    want = np.zeros(B, bool)
    for o in range(10):
        m = ops == o
        want[m] = TRUTH[o](a_bits[m], b_bits[m])
    assert np.array_equal(sk.decrypt_bool(got), want)


# ---- LUT circuits ----------------------------------------------------------------------


def lut_case(oracle, pname, m):
    """9 nodes over 5 fresh encryptions and 3 tables of modulus m: 0-4 terms, constants on three
    nodes, and on nodes 3 and 7 coefficients at the int32 edges (-2^31, 2^31 - 1, -1), so the
    wrapping multiply is exercised beyond small integers.  k_lut_combine runs at n + 1 words."""
    def make():
        c, k = ctx_for(oracle, pname)
        sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
        g = rng(1310)
        pool = sk.encrypt_lwe_message(g.integers(0, m, 5).astype(np.uint32), m, seed0=2300)
        nodes = []
        for i in range(9):
            nt = [1, 2, 0, 4, 3, 1, 2, 4, 3][i]
            terms = [(int(g.integers(0, 5)), int(g.integers(-2, 5))) for _ in range(nt)]
            if i == 3:
                terms = [(0, I32_MIN), (1, I32_MAX), (2, -1), (3, 3)]
            if i == 7:
                terms = [(4, I32_MAX), (4, I32_MIN), (0, -1), (2, I32_MAX)]
            nodes.append(((2 * i + 1) % 3, terms, (3 << 28) if i in (2, 5) else 0xFFFFFFFF if i == 8 else 0))
        x = combine(pool, nodes)
        for i in (3, 7, 8):  # combine() itself, against Python integers, on the first a word and the b word
            for j in (0, c.n1 - 1):
                v = sum(co * int(pool[s][j]) for s, co in nodes[i][1]) + (nodes[i][2] if j == c.n1 - 1 else 0)
                assert int(x[i][j]) == v % (1 << 32), (i, j)
        tables = np.array([tfhe_amd.lut_generate(c.params, m, lambda x, j=j: ((j + 1) * x + j) % m) for j in range(3)])
        return pool, nodes, tables, oracle_nodes(oracle, k.p, k.ck, pool, nodes, tables)
    return cached(("lut", pname), make)


@pytest.mark.parametrize("pname,m,forms", [
    ("uint1", 2, {"auto": "k_blind_rotate_wide<2,false,false,TV>", "whole": "k_blind_rotate<2,false,false,TV>"}),
    ("uint2", 4, {"auto": "k_blind_rotate_wide<1,false,false,TV>", "whole": "k_blind_rotate<1,false,false,TV>",
                  "octo": "k_blind_rotate_octo<1,false,false,TV>"})])
def test_lut_apply_per_item_tables(oracle, pname, m, forms):
    """tfhe_gpu_lut_apply_batch at L = 2 (the <2,...,TV> kernels of both forms) and at UINT2: all 9
    nodes equal the oracle in every form."""
    c, _ = ctx_for(oracle, pname)
    pool, nodes, tables, want = lut_case(oracle, pname, m)
    assert {len(n[1]) for n in nodes} == {0, 1, 2, 3, 4} and sum(1 for n in nodes if n[2]) >= 3
    assert sum(1 for n in nodes if len(n[1]) >= 4 and {I32_MIN, I32_MAX, -1} <= {co for _, co in n[1]}) >= 2
    ls = tfhe_amd.LutSet(c, tables)
    try:
        for form, name in forms.items():
            with c.options(br_form=form):
                got = c.lut_apply(ls, pool, nodes)
                assert c.last_kernels().startswith(name), (form, c.last_kernels())
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (form, bad.tolist())
    finally:
        ls.close()


def test_lut_circuit_at_uint2(oracle):
    """A LutCircuit of 8 nodes and depth 4 at UINT2 (n + 1 = 688 words per wire) against the oracle's
    composition level by level; two nodes carry int32-edge coefficients and four terms."""
    c, k = ctx_for(oracle, "uint2")
    sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
    circ = tfhe_amd.LutCircuit()
    a, b, d = circ.input(), circ.input(), circ.input()
    n0 = circ.node(0, [(a, 1), (b, 1)])
    n1 = circ.node(1, [(b, 2), (d, -1)], const=1 << 29)
    n2 = circ.node(2, [(a, I32_MIN), (b, I32_MAX), (d, -1), (a, 3)])
    n3 = circ.node(0, [(n0, 1), (n1, 1), (d, 1)])
    n4 = circ.node(1, [(n2, -1), (n0, 2)])
    n5 = circ.node(2, [], const=3 << 29)
    n6 = circ.node(0, [(n3, I32_MAX), (n4, I32_MIN), (n5, -1), (n1, 1)], const=0xFFFFFFFF)
    circ.node(1, [(n3, 1), (n4, 1), (n6, 1)])
    circ.output(*range(3 + len(circ.nodes)))
    levels, depth = circ.schedule()
    assert depth == 4 and levels.tolist() == [1, 1, 1, 2, 2, 1, 3, 4]
    inputs = sk.encrypt_lwe_message(np.array([1, 2, 3], np.uint32), 4, seed0=6300)
    tables = lut_case(oracle, "uint2", 4)[2]
    wires = np.zeros((3 + len(circ.nodes), c.n1), np.uint32)
    wires[:3] = inputs
    for lv in range(1, depth + 1):
        idx = np.flatnonzero(levels == lv)
        wires[3 + idx] = oracle_nodes(oracle, k.p, k.ck, wires, [circ.nodes[i] for i in idx], tables)
    ls = tfhe_amd.LutSet(c, tables)
    try:
        got, ran = circ.run(c, ls, inputs)
    finally:
        ls.close()
    assert ran == depth
    bad = np.flatnonzero((got != wires).any(axis=1))
    assert bad.size == 0, bad.tolist()


# ---- leveled operations at L = 2 (UINT1, a context without a cloud key) ---------------
def test_leveled_encryptions_at_l2(oracle):
    e = env(oracle, "uint1")
    bits = rng(11).integers(0, 2, (3, e.p.N)).astype(bool)
    mu = np.where(bits, 0.125, -0.125)
    got = e.ctx.trlwe_encrypt(e.k1, mu, alpha=e.p.alpha_lv1, seed0=700)
    want = np.array([oracle.trlwe_encrypt_f64(e.p, mu[i], e.p.alpha_lv1, e.k1, 700 + i) for i in range(3)])
    assert np.array_equal(got, want)
    assert np.array_equal(e.ctx.trlwe_decrypt_bool(e.k1, got), bits)
    tg = e.ctx.trgsw_encrypt(e.k1, [0, 1], alpha=e.p.alpha_bsk, seed0=900)
    assert tg.shape == (2, 4, 2, e.p.N)
    assert np.array_equal(tg, e.trgsw[:2])


@pytest.mark.parametrize("B", [1, 5, 9])
def test_cmux_at_l2(oracle, B):
    e = env(oracle, "uint1")
    g = rng(20 + B)
    in0, in1 = u32rand(g, B, 2 * e.p.N), u32rand(g, B, 2 * e.p.N)
    sel = np.array([(2 * i + 1) % 3 for i in range(B)], np.uint32)
    got = e.ctx.cmux(e.set, sel, in0, in1)
    assert e.ctx.last_kernels() == "k_cmux<2>"
    for i in range(B):
        assert np.array_equal(got[i], oracle.cmux(e.p, in0[i], in1[i], e.trgsw[sel[i]], e.off)), i


@pytest.mark.parametrize("form", [f for f, _ in FORMS], ids=[n for _, n in FORMS])
@pytest.mark.parametrize("k,Q", [(3, 5), (5, 2)])
def test_table_lookup_at_l2(oracle, k, Q, form):
    e = env(oracle, "uint1")
    g = rng(100 + k)
    table = u32rand(g, 1 << k, 2 * e.p.N)
    _, addr = lookup_addresses(k, Q, g)
    with e.ctx.options(cmux_form=form):
        got = e.ctx.table_lookup(e.set, addr, table)
        assert e.ctx.last_kernels() == expected_kernels(form, k, 2)
        if form != tfhe_amd.CMUX_PER_WAVE:
            assert e.ctx.last_kernels() == "k_cmux_shared<2> + k_cmux<2>"
    want = cached(("lookup_l2", k), lambda: [oracle_lookup(oracle, e, table, addr[q]) for q in range(Q)])
    for q in range(Q):
        assert np.array_equal(got[q], want[q]), q


def test_table_lookup_returns_the_addressed_entry_at_l2(oracle):
    e = env(oracle, "uint1")
    values = np.array([0xA5, 0x3C, 0xFF, 0x00, 0x81, 0x7E, 0x12, 0xC9], np.uint64)
    table = tfhe_amd.lookup_table_pack_bits(e.tp, values, 8)
    addr = np.array([[((v >> j) & 1) * (1 + j % 2) for j in range(3)] for v in range(8)], np.uint32)
    dec = e.ctx.trlwe_decrypt_bool(e.k1, e.ctx.table_lookup(e.set, addr, table))
    for v in range(8):
        assert tfhe_amd.bit_utils.convert(dec[v][:8]) == int(values[v]), v


# ---- key generation ---------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["uint1", "uint3"])
def test_keygen_matches_oracle(oracle, pname):
    """tfhe_gpu_keygen == the oracle's CloudKey.new at an L = 2 BK layout and at a basebit 6 KSK."""
    k = get_keys(oracle, pname)
    c = tfhe_amd.Context(pname, 0)
    try:
        sk, (bk, ksk) = c.keygen(42, 43, want_host_copy=True)
        assert np.array_equal(sk.key_lv0, k.k0) and np.array_equal(sk.key_lv1, k.k1)
        assert np.array_equal(ksk, k.ck.ksk)
        assert np.array_equal(bk, k.ck.bk)
    finally:
        c.close()
