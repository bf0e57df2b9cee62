"""GPU parity over the gadget grid (gadget_grid_cases.py; DESIGN.md §6.3 maps instantiation -> test): every
blind-rotation instantiation br_kernel() can reach from an accepted (L, bgbit), its per-item-table twin, the
leveled kernels at the extreme gadgets, the margin guard's recompute at L = 1, and the select / gather key switch
at 16 and 32 items per block.  Every comparison is np.array_equal against the oracle in reference-tree mode;
there is no tolerance anywhere, and last_kernels() is asserted wherever the instantiation is the point.

n = 8 at every grid set: an oracle rotation is 8 CMUXes and a GPU launch takes milliseconds.  Keys, contexts and
oracle outputs are computed once per module."""
import types

import numpy as np
import pytest

import tfhe_amd
from conftest import rng
from gadget_grid_cases import (EXTREMES, GRID, L2SMALL, N, grid_keys, grid_set, lut_nodes_case, near_tie_batch,
                               rotate_modes, rotation_inputs, small_products, whole_form_packs, words)
from test_leveled import expected_kernels, lookup_addresses, oracle_lookup
from test_lut_circuit import ctx_for as ctx_128, oracle_nodes
from test_lut_ext import blind_rotate_ext_ref
from test_param_sets import ctx_for as ctx_named

pytestmark = pytest.mark.gpu

_CTX, _CACHE = {}, {}


def ctx_for(oracle, L, bgbit):
    """(context with the set's seeded cloud key loaded, its GridKeys), cached for the module."""
    if (L, bgbit) not in _CTX:
        k = grid_keys(oracle, L, bgbit)
        c = tfhe_amd.Context(tfhe_amd.make_params(k.d), 0)
        c.load_cloud_key(k.ck.offset, k.ck.testvec, k.ck.bk, k.ck.ksk)
        _CTX[L, bgbit] = (c, k)
    return _CTX[L, bgbit]


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def br_name(form, L, bgbit, fused, tv=False):
    """The name br_kernel() gives the instantiation (tfhe_kernels.hip, tfhe_kernels_whole.hip)."""
    s, f = str(small_products(L, bgbit)).lower(), str(fused).lower()
    targs = f"{L},{s},{f}" + (",TV" if tv else "")
    per = "per-item tables; " if tv else ""
    tail = ", fused)" if fused else ")"
    if form == "whole" and fused and L == 3:
        return f"k_blind_rotate_assist<true{',TV' if tv else ''}> ({per}whole form, loader waves own polynomial b, fused)"
    kernel, what = {"whole": ("k_blind_rotate", "whole form"), "wide": ("k_blind_rotate_wide", "latency form"),
                    "octo": ("k_blind_rotate_octo", "octo form")}[form]
    return f"{kernel}<{targs}> ({per}{what}{tail}"


ARITH = {"default": tfhe_amd.ARITH_AUTO, "reference": tfhe_amd.ARITH_REFERENCE, "forced": tfhe_amd.ARITH_FUSED_FORCED}


def br_cases(sets):
    """(L, bgbit, form, arith): whole and wide (octo at L = 1 too) x default and reference arithmetic, and the
    forced fused arithmetic where the set has small products."""
    out = []
    for L, bgbit in sets:
        for form in ["whole", "wide"] + (["octo"] if L == 1 else []):
            for arith in ["default", "reference"] + (["forced"] if small_products(L, bgbit) else []):
                out.append(pytest.param(L, bgbit, form, arith, id=f"{L}-{bgbit}-{form}-{arith}"))
    return out


def ks_kernels(c):
    """The key-switch part of last_kernels() after a bare key switch: what precedes the first separator is the
    context's last blind rotation, of an earlier call or none (tests/golden/last_kernels.json records that)."""
    return c.last_kernels().split(" + ", 1)[1]


def is_fused(c, L, bgbit, arith):
    return small_products(L, bgbit) and (arith == "forced" or (arith == "default" and c.get_option("fused_admitted") == 1))


def assert_whole_form_refused(c):
    """(3,9) and (3,10): TFHE_OPT_BR_FORM 1 is refused with the reason, and the option keeps its value."""
    with pytest.raises(tfhe_amd.TfheError, match="whole form.*4\\*bgbit > 32") as e:
        c.set_option("br_form", "whole")
    assert e.value.status == tfhe_amd.ERR_INVALID and c.get_option("br_form") == 0


# ---- blind rotation: every form x arithmetic ----------------------------------------------
def br_case(oracle, L, bgbit):
    def make():
        _, k = ctx_for(oracle, L, bgbit)
        cts = rotation_inputs(k.p.n)
        return cts, np.array([oracle.blind_rotate(k.p, t, k.ck.testvec, k.ck.bk, k.ck.offset) for t in cts])
    return cached(("br", L, bgbit), make)


@pytest.mark.parametrize("L,bgbit,form,arith", br_cases(GRID))
def test_blind_rotate_vs_oracle(oracle, L, bgbit, form, arith):
    """B = 3 and B = 5 (idle item slots in the whole and octo forms; B = 5 spans two whole-form workgroups) of
    uniform words with an a~ = 0 and an a~ = 2N row.  The first kernel is the instantiation br_kernel() names for
    (form, L, small_products, fused), and it ends in 'fused)' exactly when the set has small products and the key
    was admitted (default) or the fused arithmetic forced; every word equals the oracle's reference trees either
    way (the margin guard recomputes what the fused arithmetic rounds near a tie).  Among these:
    k_blind_rotate<1,true,*>, _wide<1,true,*>, _octo<1,true,*> at (1,1) and (1,7), <3,false,false> of both forms at
    (3,7) and (3,8), and the assist form at Bg = 2.  At (3,9) and (3,10), where tmp_a's level-2 field does not fit
    under tmp_b's in one word, the whole form is refused and the default dispatch is the latency form."""
    c, k = ctx_for(oracle, L, bgbit)
    cts, want = br_case(oracle, L, bgbit)
    fused = is_fused(c, L, bgbit, arith)
    if form == "whole" and not whole_form_packs(L, bgbit):
        assert_whole_form_refused(c)
        form, opts = "wide", dict(br_form="auto")  # what every plan runs there
    else:
        opts = dict(br_form=form)
    name = br_name(form, L, bgbit, fused)
    assert name.endswith("fused)") == fused
    with c.options(arith=ARITH[arith], **opts):
        for lo, hi in ((0, 3), (3, 8)):
            got = c.blind_rotate_batch(cts[lo:hi])
            assert c.last_kernels().split(" + ")[0] == name, c.last_kernels()
            bad = np.flatnonzero((got != want[lo:hi]).any(axis=1))
            assert bad.size == 0, ((lo, hi), bad.tolist(), int((got != want[lo:hi]).sum()))


# ---- per-item tables: the TV twin of every instantiation -----------------------------------
def lut_case(oracle, L, bgbit):
    def make():
        _, k = ctx_for(oracle, L, bgbit)
        pool, nodes, tables, _ = lut_nodes_case(k.p.n)
        return pool, nodes, tables, oracle_nodes(oracle, k.p, k.ck, pool, nodes, tables)
    return cached(("lut", L, bgbit), make)


@pytest.mark.parametrize("L,bgbit,form,arith", br_cases(GRID + [(2, 6)]))
def test_lut_apply_per_item_tables(oracle, L, bgbit, form, arith):
    """tfhe_gpu_lut_apply_batch on 5 nodes over 4 inputs and 3 uniform tables, each form forced: the <...,TV>
    twin of every instantiation above, and <2,true,*,TV> of both forms at l2small with n = 8.  The outputs pass
    the key switch at n = 8 (9 output words: one tile of the GEMM, 9 of its 32 columns; the lane form at l2small's
    (4,3)) and equal oracle.gate_batch(COPY, x_i, testvec = the node's table) word for word."""
    c, k = ctx_for(oracle, L, bgbit)
    pool, nodes, tables, want = lut_case(oracle, L, bgbit)
    fused = is_fused(c, L, bgbit, arith)
    if form == "whole" and not whole_form_packs(L, bgbit):
        assert_whole_form_refused(c)
        form, opts = "wide", dict(br_form="auto")
    else:
        opts = dict(br_form=form)
    ls = tfhe_amd.LutSet(c, tables)
    try:
        with c.options(arith=ARITH[arith], **opts):
            got = c.lut_apply(ls, pool, nodes)
            kernels = c.last_kernels().split(" + ")
    finally:
        ls.close()
    assert kernels[0] == br_name(form, L, bgbit, fused, tv=True), kernels
    assert kernels[1:] == (["k_key_switch_lanes<4,3,32,4,1>"] if (L, bgbit) == (2, 6) else
                           ["k_key_switch_gemm<3,5>", "k_ks_gemm_reduce"]), kernels
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, bad.tolist()


def test_key_switch_at_n_8(oracle):
    """The first key switch at n = 8 on its own: 9 output words, so one 32-word chunk of the lane form, one
    256-thread block of the gather form, most of whose lanes have no word, and one 32-column GEMM tile with 9
    columns in use; 1 and 5 items."""
    c, k = ctx_for(oracle, 1, 8)
    lv1 = words(7900, 5, N + 1)
    want = np.array([oracle.identity_key_switch(k.p, x, k.ck.ksk) for x in lv1])
    for opts, name in ((dict(ks_form=0), "k_key_switch_lanes<3,5,32,4,1>"), (dict(ks_form=1), "k_key_switch_gather"),
                       (dict(ks_form=1, ks_sel_items=32), "k_key_switch_gather<3,32>"),
                       (dict(ks_form=2), "k_key_switch_gemm<3,5> + k_ks_gemm_reduce"),
                       (dict(), "k_key_switch_gemm<3,5> + k_ks_gemm_reduce")):
        with c.options(**opts):
            for B in (1, 5):
                assert np.array_equal(c.key_switch(lv1[:B]), want[:B]), (opts, B)
                assert ks_kernels(c) == name


# ---- external product and the leveled kernels at the extreme gadgets ------------------------
def leveled_env(oracle, L, bgbit):
    """Three selectors (encryptions of 0, 1, 1) resident on the set's context: what test_leveled.Env holds."""
    def make():
        c, k = ctx_for(oracle, L, bgbit)
        trgsw = np.array([oracle.trgsw_encrypt_torus_fft(k.p, mu, k.p.alpha_bsk, k.k1, 900 + s)
                          for s, mu in enumerate([0, 1, 1])])
        return types.SimpleNamespace(ctx=c, p=k.p, k=k, off=k.ck.offset, trgsw=trgsw, set=tfhe_amd.TrgswSet(c, trgsw))
    return cached(("env", L, bgbit), make)


@pytest.mark.parametrize("L,bgbit", EXTREMES)
def test_external_product_at_the_extremes(oracle, L, bgbit):
    """k_external_product<L> on 4 items against a fresh TRGSW and against a row of the resident key, at Bg = 2,
    at L bgbit = 32 (the last field starts at bit 0), and at the L = 3 gadgets around 4 bgbit = 32."""
    e = leveled_env(oracle, L, bgbit)
    x = words(8000 + bgbit, 4, 2 * N)
    want = np.array([oracle.external_product(e.p, e.trgsw[1], t, e.off) for t in x])
    assert np.array_equal(e.ctx.external_product(x, trgsw_fft=e.trgsw[1]), want)
    row = e.p.n - 1
    want = np.array([oracle.external_product(e.p, e.k.ck.bk[row], t, e.off) for t in x])
    assert np.array_equal(e.ctx.external_product(x, bk_index=row), want)


@pytest.mark.parametrize("L,bgbit", EXTREMES)
def test_cmux_at_the_extremes(oracle, L, bgbit):
    """k_cmux<L>, B = 5: two workgroups, the second with one item."""
    e = leveled_env(oracle, L, bgbit)
    g = rng(8100 + bgbit)
    in0, in1 = words(8100 + bgbit, 5, 2 * N), words(8200 + bgbit, 5, 2 * N)
    sel = np.array([(2 * i + 1) % 3 for i in range(5)], np.uint32)
    got = e.ctx.cmux(e.set, sel, in0, in1)
    assert e.ctx.last_kernels() == f"k_cmux<{L}>"
    for i in range(5):
        assert np.array_equal(got[i], oracle.cmux(e.p, in0[i], in1[i], e.trgsw[sel[i]], e.off)), i


@pytest.mark.parametrize("form", [tfhe_amd.CMUX_PER_WAVE, tfhe_amd.CMUX_SHARED], ids=["wave", "shared"])
@pytest.mark.parametrize("L,bgbit", EXTREMES)
def test_table_lookup_at_the_extremes(oracle, L, bgbit, form):
    """k = 3, Q = 2: the per-wave form, and the workgroup form (k_cmux_shared<L> on the first level, whose 4 pairs
    per query share a selector) followed by k_cmux<L>; the CMUX tree level by level on the oracle."""
    e = leveled_env(oracle, L, bgbit)
    g = rng(8300 + bgbit)
    table = words(8300 + bgbit, 8, 2 * N)
    _, addr = lookup_addresses(3, 2, g)
    with e.ctx.options(cmux_form=form):
        got = e.ctx.table_lookup(e.set, addr, table)
        assert e.ctx.last_kernels() == expected_kernels(form, 3, L)
    want = cached(("lookup", L, bgbit), lambda: [oracle_lookup(oracle, e, table, addr[q]) for q in range(2)])
    for q in range(2):
        assert np.array_equal(got[q], want[q]), q


@pytest.mark.parametrize("L,bgbit", EXTREMES)
def test_blind_rotate_ext_at_the_extremes(oracle, L, bgbit):
    """k_blind_rotate_ext<L,2> (eta = 1), B = 3: both accumulators of every item, word for word, against the
    definition composed from oracle.cmux and oracle.poly_mul_with_xk."""
    oracle.set_fused(0)
    c, k = ctx_for(oracle, L, bgbit)
    tv, x = words(8400 + bgbit, 2, 2 * N), words(8500 + bgbit, 3, k.p.n + 1)
    got = c.blind_rotate_ext(1, x, tv)
    assert got.shape == (3, 2, 2 * N) and c.last_kernels() == f"k_blind_rotate_ext<{L},2>", c.last_kernels()
    for i in range(3):
        assert np.array_equal(got[i], blind_rotate_ext_ref(oracle, k.p, k.ck, x[i], tv, 1)), i


# ---- the margin guard at L = 1 ---------------------------------------------------------------
@pytest.mark.parametrize("form", ["auto", "whole", "octo"])
def test_margin_guard_recomputes_near_ties_at_l1(oracle, form):
    """test_param_sets.test_margin_guard_recomputes_near_ties_at_l2 at L = 1, (1,7), zero KSK.  Under the crafted
    key the oracle's fused mode parts from its reference mode (test_gadget_grid_cpu proves it for the crafted
    item).  By default the rotation returns the reference-mode words, whichever arithmetic the key admission
    chose; forced fused arithmetic runs <1,true,true> of the form, flags the items, the recompute launch
    br_kernel('w', 1, true, false) = k_blind_rotate<1,true,false> redoes them (near_tie_items rises by at least
    the number of parted items) and every output equals the reference-mode words.  An honest batch under the
    set's own keygen'd key, forced fused, recomputes at most what it flags and equals the oracle too
    (test_blind_rotate_vs_oracle's 'forced' cases)."""
    k = grid_keys(oracle, 1, 7)
    p = k.p
    tv, bk, cts = near_tie_batch(oracle, p)
    off = k.ck.offset
    want, fused = cached("near_tie_l1", lambda: rotate_modes(oracle, p, cts, tv, bk, off))
    parted = int((fused != want).any(axis=1).sum())
    assert not np.array_equal(fused[2], want[2]) and parted >= 1
    ksk = np.zeros((p.N * p.iks_t * (1 << p.basebit), p.n + 1), np.uint32)
    c = tfhe_amd.Context(tfhe_amd.make_params(k.d), 0)
    try:
        c.load_cloud_key(off, tv, bk, ksk)
        admitted = c.get_option("fused_admitted") == 1
        before = c.near_tie_items()
        with c.options(br_form=form):
            assert np.array_equal(c.blind_rotate_batch(cts, tv), want)
            assert c.last_kernels().split(" + ")[0].endswith("fused)") == admitted
        if not admitted:
            assert c.near_tie_items() == before
        before = c.near_tie_items()
        with c.options(br_form=form, arith=tfhe_amd.ARITH_FUSED_FORCED):
            got = c.blind_rotate_batch(cts, tv)
            assert c.last_kernels().split(" + ")[0] == br_name({"auto": "wide"}.get(form, form), 1, 7, True)
        assert parted <= c.near_tie_items() - before <= len(cts)
        assert np.array_equal(got, want)
    finally:
        c.close()


# ---- TFHE_OPT_KS_SEL_ITEMS ---------------------------------------------------------------------
KS_SETS = {"128": (lambda o: ctx_128(o, "128"), "k_key_switch_sel", 9),
           "uint2": (lambda o: ctx_named(o, "uint2"), "k_key_switch_gather", 3)}


def ks_case(oracle, pname):
    def make():
        _, k = KS_SETS[pname][0](oracle)
        lv1 = words(8600, 33, N + 1)
        return lv1, np.array([oracle.identity_key_switch(k.p, x, k.ck.ksk) for x in lv1])
    return cached(("ks", pname), make)


@pytest.mark.parametrize("items", [8, 16, 32])
@pytest.mark.parametrize("B", [1, 17, 33])
@pytest.mark.parametrize("pname", list(KS_SETS))
def test_key_switch_items_per_block(oracle, pname, B, items):
    """ks_form = 1 with 8, 16 and 32 items per block at the 128-bit set (k_key_switch_sel<9,G>, n + 1 = 701
    words: three blocks across, the last ragged) and at UINT2 (k_key_switch_gather<3,G>, (3,4)): one item, 17 (a
    ragged second block at 16) and 33 (a ragged second block at 32, a fifth at 8).  Every item against the
    oracle.  The default keeps its bare name; 16 and 32 name their instantiation."""
    c, _ = KS_SETS[pname][0](oracle)
    lv1, want = ks_case(oracle, pname)
    kernel, t = KS_SETS[pname][1:]
    with c.options(ks_form=1, ks_sel_items=items):
        got = c.key_switch(lv1[:B])
        assert ks_kernels(c) == (kernel if items == 8 else f"{kernel}<{t},{items}>")
    bad = np.flatnonzero((got != want[:B]).any(axis=1))
    assert bad.size == 0, bad.tolist()


@pytest.mark.parametrize("value", [0, 1, 4, 12, 24, 64, -8])
def test_key_switch_items_per_block_refuses_other_values(oracle, value):
    """include/tfhe_gpu.h: TFHE_OPT_KS_SEL_ITEMS takes 8, 16 or 32; anything else is TFHE_ERR_INVALID and the
    option keeps its value (so the next key switch still runs what was chosen)."""
    c, _ = KS_SETS["uint2"][0](oracle)
    with c.options(ks_form=1, ks_sel_items=16):
        with pytest.raises(tfhe_amd.TfheError) as e:
            c.set_option("ks_sel_items", value)
        assert e.value.status == tfhe_amd.ERR_INVALID
        assert c.get_option("ks_sel_items") == 16
        lv1, want = ks_case(oracle, "uint2")
        assert np.array_equal(c.key_switch(lv1[:3]), want[:3]) and ks_kernels(c) == "k_key_switch_gather<3,16>"
    assert c.get_option("ks_sel_items") == 8
