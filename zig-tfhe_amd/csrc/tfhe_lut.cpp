// tfhe_lut.cpp — LUT circuits of the C ABI (include/tfhe_gpu.h): resident sets of test vectors, batches of
// "linear combination, then programmable bootstrap with the node's own table", and the level-scheduled evaluator
// for DAGs of such nodes.  Host code: the kernels are in tfhe_kernels_lut.hip and tfhe_kernels_lut_ext.hip, the
// bootstrap is run_bootstrap_dev with a per-item table selector (KParams::tv_sel), the planner is in tfhe_cpu.cpp.
//
// Every node is bootstrapped by lut_level_step, which runs one level (LutLevel) over device memory: the select
// nodes' test vectors (select_testvecs: stage, pack, spread), the multi-output nodes in a launch of their own
// (lut_multi_launch: rounded x, the accumulator, the fan-out extraction, one key switch), one combination launch
// over the rest, and their bootstraps grouped by eta (bootstrap_by_eta: run_bootstrap_dev for eta = 0, one
// k_blind_rotate_ext launch per eta > 0, then one extraction and one key switch over the extended items).  An
// item's test vector is a table of the set, or LUT_TV_EACH | k: test vector k of the level's own.
// What feeds it:
//   lut_circuit_on   one LutLevel per level of the plan: wires is the wire table, out the level's run of slots.
//   lut_batch_on     the flat node batches (lut_apply, _multi, _ext, lut_select, _ext) as one level: wires is the
//                    caller's pool, out the caller's out, every node in the one eta group; select nodes have no set.
//   lut_each_on      bootstrap_lut_each[_ext] has no nodes: bootstrap_by_eta on the caller's inputs and test vectors.
//   lut_apply2_on    the bivariate node is not a level (per chunk: level 1, pack, spread, level 2); it shares the
//                    helpers.
// batch_entry checks the arguments of every flat entry.  Everything here runs on the context's first device.
#include "tfhe_gpu.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "tfhe_ctx.hpp"

using namespace tfhe;

// T test vectors (TRLWELv1, 2N words each) resident on one device.
struct tfhe_gpu_lut_set {
    const tfhe_gpu_ctx *ctx = nullptr;  // the context that loaded it (identity only, never dereferenced)
    tfhe_params P{};
    size_t T = 0;
    DevPtr<uint32_t> tables;  // T * 2N words
};

namespace tfhe {

// The multi-output form of a launch of B nodes with M >= B outputs: x (rounded per node by shift[])
// -> one accumulator per node -> the M extractions fan[] names -> one key switch into out
// (M TLWELv0).  desc pointers are device copies.  x, the accumulators and the extractions are the launch's own.
static int lut_multi_launch(Device &d, const uint32_t *tables, const uint32_t *pool, const uint32_t *off,
                            const uint32_t *src, const int32_t *coef, const uint32_t *konst, const uint32_t *lut,
                            const uint32_t *shift, const uint32_t *fan, uint32_t *out, size_t B, size_t M) {
    Frame f(d);
    uint32_t *x = f.take<uint32_t>(B * tlwe0_words(d.P)), *acc = f.take<uint32_t>(B * 2 * (size_t)d.P.N);
    uint32_t *lv1 = f.ks_input<uint32_t>(M * 1025);
    int rc = f.rc();
    if (rc) return rc;
    HIPCHK(d, launch_lut_combine_round(d.K, pool, off, src, coef, konst, shift, x, B, d.stream));
    const size_t ev_at = d.ev_used;
    if ((rc = run_bootstrap_dev(d, nullptr, x, nullptr, tables, acc, B, RUN_TRLWE, nullptr, lut))) return rc;
    const char *fan_name = "";
    HIPCHK(d, launch_lut_fanout_extract(acc, fan, lv1, M, d.stream, &fan_name));
    KsGemm G;
    if ((rc = ks_gemm_args(f, M, G))) return rc;
    HIPCHK(d, launch_key_switch(d.K, lv1, d.d_ksk, out, M, d.stream, d.opts, &d.last_ks, &G));
    // last_kernels: the blind rotation, then the fan-out extraction and the key switch
    d.lut_multi_ks = std::string(fan_name) + " + " + d.last_ks;
    d.last_ks = d.lut_multi_ks.c_str();
    // profiling: the launch's third event moves behind the epilogue, so (ev1, ev2) times extract + key switch
    if (d.ev_used == ev_at + 3) HIPCHK(d, hipEventRecord(d.events[ev_at + 2], d.stream));
    return TFHE_OK;
}

// round_theta's shift per node and the (node, coefficient) pair per output, for the nodes theta[0 .. B)
static void multi_descriptors(const tfhe_params &P, const uint32_t *theta, size_t B, std::vector<uint32_t> &shift,
                              std::vector<uint32_t> &fan) {
    for (size_t i = 0; i < B; i++) {
        shift.push_back(lut_round_shift(P, theta[i]));
        for (uint32_t j = 0; j < (1u << theta[i]); j++) fan.push_back((uint32_t)i), fan.push_back(j);
    }
}

static_assert(LUT_TV_EACH == TV_SEL_EACH, "the planner's selector bit is the kernels'");

// The selector of a bootstrap whose item g reads test vector g of the call's own (tv_each + g * 2N):
// LUT_TV_EACH | 0 .. B-1, appended to a call's descriptors.
static size_t add_iota(DescBlob &blob, size_t B) {
    const size_t at = blob.words.size();
    for (size_t i = 0; i < B; i++) blob.words.push_back((uint32_t)i | LUT_TV_EACH);
    return at;
}

// The extended blind rotation over device buffers, async: all E accumulators of each item (all) or acc_0.
// tv_each: the base of the entries of tv_sel with TV_SEL_EACH set (select nodes), or NULL.
static int blind_rotate_ext_launch(Device &d, uint32_t eta, const uint32_t *x, const uint32_t *testvec,
                                   const uint32_t *tv_sel, uint32_t *acc, bool all, size_t B,
                                   const uint32_t *tv_each = nullptr) {
    BrExtBatch b;
    b.eta = eta;
    b.in = x;
    b.testvec = testvec;
    b.tv_sel = tv_sel;
    b.tv_each = tv_each;
    b.bk = d.d_bk;
    b.out = acc;
    b.all = all;
    b.B = B;
    d.last_ks = "";
    HIPCHK(d, launch_blind_rotate_ext(d.K, tables(d), b, d.stream, &d.last_br));
    d.bootstraps += B;
    return TFHE_OK;
}

// The end of an extended bootstrap over B accumulators acc_0 (2N words each): sampleExtractIndex(., 0) into lv1
// (f.ks_input of B * 1025 words) and one key switch into out.  zero: a device word 0, the extraction's coefficient.
static int ext_extract_ks(Device &d, Frame &f, const uint32_t *acc, const uint32_t *zero, uint32_t *lv1, uint32_t *out,
                          size_t B) {
    HIPCHK(d, launch_sample_extract(acc, zero, 1, lv1, B, d.stream));
    KsGemm G;
    if (const int rc = ks_gemm_args(f, B, G)) return rc;
    HIPCHK(d, launch_key_switch(d.K, lv1, d.d_ksk, out, B, d.stream, d.opts, &d.last_ks, &G));
    return TFHE_OK;
}

// The bootstraps of a run of items x grouped by eta, n[0] | n[1] | n[2] of them, into the same run of out: item g
// starts from the test vector tv_sel[g] names, a table of `tables` (the extended table for eta > 0; NULL where no
// item names one) or, with LUT_TV_EACH set, one of tv_each in every component.  The eta = 0 group is one
// run_bootstrap_dev; each eta > 0 group is one k_blind_rotate_ext launch (acc_0 of each item), and one extraction and
// one key switch follow over both groups.  Their accumulators come from f; zero: a device word 0 (n[1] + n[2] > 0).
static int bootstrap_by_eta(Device &d, Frame &f, const uint32_t *x, const uint32_t *tables, const uint32_t *tv_sel,
                            const uint32_t *tv_each, const size_t n[3], const uint32_t *zero, uint32_t *out) {
    const size_t w = tlwe0_words(d.P), TRLWE = 2 * (size_t)d.P.N, next = n[1] + n[2];
    int rc;
    if (n[0]) {
        rc = run_bootstrap_dev(d, nullptr, x, nullptr, tables, out, n[0], RUN_BOOTSTRAP, nullptr, tv_sel, tv_each);
        if (rc) return rc;
    }
    if (!next) return TFHE_OK;
    uint32_t *acc = f.take<uint32_t>(next * TRLWE), *lv1 = f.ks_input<uint32_t>(next * 1025);
    if ((rc = f.rc())) return rc;
    for (size_t e = 1, done = 0; e <= 2; done += n[e], e++) {
        if (!n[e]) continue;
        rc = blind_rotate_ext_launch(d, (uint32_t)e, x + (n[0] + done) * w, tables, tv_sel + n[0] + done,
                                     acc + done * TRLWE, /*all*/ false, n[e], tv_each);
        if (rc) return rc;
    }
    return ext_extract_ks(d, f, acc, zero, lv1, out + n[0] * w, next);
}

// The test vectors of ns select nodes (include/tfhe_gpu.h "Select nodes") into tv (ns TRLWELv1): per chunk of
// nodes the m entries of each are staged in pack order (the combine kernel with at most one term: a wire is
// copied, a constant becomes a trivial ciphertext) and packed into the slots i*w; then one spread in place over
// all of them.  The chunk is the pack's own (pack_chunk_items) in whole nodes, as in lut_apply2_on, and every
// step is per item, so chunking changes no word.  e_off / e_konst start at the first node's first entry, e_src and
// ones (a 1 per wire entry) are whole arrays the offsets index, coef_dev holds the m slot coefficients; all device.
static int select_testvecs(Device &d, const tfhe_gpu_packing_key &pk, uint32_t m, const uint32_t *pool,
                           const uint32_t *e_off, const uint32_t *e_src, const int32_t *ones, const uint32_t *e_konst,
                           const uint32_t *coef_dev, uint32_t *tv, size_t ns) {
    const size_t w = tlwe0_words(d.P), N = d.P.N;
    const size_t nodes = std::min(ns, std::max<size_t>(1, pack_chunk_items(d, ns * m, (int)pk.basebit) / m));
    Frame f(d);
    uint32_t *g = f.ks_input<uint32_t>(nodes * m * w, /*pack*/ true);
    int rc = f.rc();
    if (rc) return rc;
    for (size_t b0 = 0; b0 < ns; b0 += nodes) {
        const size_t nb = std::min(nodes, ns - b0);
        HIPCHK(d, launch_lut_combine(d.K, pool, e_off + b0 * m, e_src, ones, e_konst + b0 * m, g, nb * m, d.stream));
        if ((rc = pack_launch(d, pk, g, coef_dev, m, tv + b0 * 2 * N, nb))) return rc;
    }
    HIPCHK(d, launch_lut_spread(tv, (uint32_t)(N / m), (uint32_t)(2 * N - N / (2 * m)), tv, ns, d.stream));
    return TFHE_OK;
}

// The pack's slot coefficients i * N/m of a select node, appended to a call's descriptors.
static size_t add_slot_coefs(DescBlob &blob, uint32_t N, uint32_t m) {
    const size_t at = blob.reserve(m);
    for (uint32_t i = 0; i < m; i++) blob.words[at + i] = i * (N / m);
    return at;
}

// One level of nodes over device memory (every pointer is a device pointer).  The nodes come in the plan's order
// (tfhe_cpu.hpp, LutCircuitPlan): grouped by eta, eta = 0 first, and inside each group the ordinary nodes, then
// the select nodes; the outputs follow that order.  A multi-output node (theta > 0) has eta 0, an extended node
// one output.
struct LutLevel {
    const uint32_t *wires;   // the source ciphertexts (TLWELv0): what the terms and the select entries name
    const uint32_t *tables;  // the set's test vectors; NULL where every node is a select node (the flat select entries)
    // the nodes: nb + 1 CSR offsets into the whole arrays src / coef, and per node the constant and where its test
    // vector comes from: a table, or LUT_TV_EACH | k for the level's k-th select node
    const uint32_t *off, *src;
    const int32_t *coef;
    const uint32_t *konst, *tv_sel;
    // read where no != nb only: round_theta's shift per node, the (node, coefficient) pair per output
    const uint32_t *shift, *fan;
    size_t nb, no;                  // nodes, outputs
    uint32_t neta[3], nsel_eta[3];  // the nodes / the select nodes of each eta group
    size_t nsel;                    // select nodes in all
    // select nodes: their entries' CSR from the level's first entry on (m per node in pack order, at most one term
    // each, into the whole arrays e_src / ones), the entries' constants, the m slot coefficients, the packing key
    const uint32_t *e_off, *e_src;
    const int32_t *ones;
    const uint32_t *e_konst, *slot_coef;
    const tfhe_gpu_packing_key *pk;
    uint32_t m;
    const uint32_t *zero;  // a word 0, the extended nodes' extraction coefficient
    uint32_t *out;         // no TLWELv0
};

// Runs a level: the select nodes' test vectors first; with a theta > 0 the ordinary eta = 0 nodes in one multi-output
// launch; one combination launch over the rest, whose items are bootstrapped group by group.  The level's
// temporaries go with its frame.
static int lut_level_step(Device &d, const LutLevel &L) {
    const size_t w = tlwe0_words(d.P);
    const size_t next = (size_t)L.neta[1] + L.neta[2], nb0 = L.nb - next, no0 = L.no - next;  // an extended node has one output
    const size_t nord = nb0 - L.nsel_eta[0];
    int rc;
    Frame level(d);
    uint32_t *tv = nullptr;
    if (L.nsel) {  // the test vectors of all of the level's select nodes, whatever their eta
        tv = level.take<uint32_t>(L.nsel * 2 * (size_t)d.P.N);
        if ((rc = level.rc())) return rc;
        rc = select_testvecs(d, *L.pk, L.m, L.wires, L.e_off, L.e_src, L.ones, L.e_konst, L.slot_coef, tv, L.nsel);
        if (rc) return rc;
    }
    // a theta > 0 in this level: the ordinary nodes in the multi-output launch, the select nodes with the rest
    const bool split = no0 != nb0;
    if (split) {
        rc = lut_multi_launch(d, L.tables, L.wires, L.off, L.src, L.coef, L.konst, L.tv_sel, L.shift, L.fan, L.out, nord,
                              no0 - L.nsel_eta[0]);
        if (rc) return rc;
    }
    // one combination launch over the rest: the eta = 0 items of the bootstrap launch, then the extended groups,
    // into the slots behind the multi-output launch's
    const size_t skip = split ? nord : 0, items = L.nb - skip;
    if (!items) return TFHE_OK;
    uint32_t *x = level.take<uint32_t>(items * w);
    if ((rc = level.rc())) return rc;
    HIPCHK(d, launch_lut_combine(d.K, L.wires, L.off + skip, L.src, L.coef, L.konst + skip, x, items, d.stream));
    const size_t n[3] = {nb0 - skip, L.neta[1], L.neta[2]};
    return bootstrap_by_eta(d, level, x, L.tables, L.tv_sel + skip, tv, n, L.zero, L.out + (no0 - n[0]) * w);
}

// A whole LUT circuit: the plan's descriptors in one upload, one level step per level into the wire table (in the
// plan's slot order, so a level's outputs are one run of slots above everything it reads), the outputs gathered at
// the end.  pk, m: the select nodes'.
static int lut_circuit_on(Device &d, const tfhe_gpu_lut_set &set, size_t n_inputs, const uint32_t *inputs, size_t n_nodes,
                          const LutCircuitPlan &pl, size_t n_outputs, uint32_t *outputs, bool dev,
                          const tfhe_gpu_packing_key *pk = nullptr, uint32_t m = 0) {
    if (n_nodes && !d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t w = tlwe0_words(d.P), W = pl.slot.size();  // inputs + every node's outputs
    // multi-output nodes anywhere: round_theta's shift per node (evaluation order) and the plan's fan-out pairs
    const bool multi = std::any_of(pl.theta.begin(), pl.theta.end(), [](uint32_t t) { return t != 0; });
    const bool select = pl.depth && pl.sfirst[pl.depth] != 0;
    const bool ext = std::any_of(pl.eta.begin(), pl.eta.end(), [](uint32_t e) { return e != 0; });
    std::vector<uint32_t> shift;
    if (multi)
        for (uint32_t t : pl.theta) shift.push_back(lut_round_shift(d.P, t));
    const std::vector<uint32_t> ones(pl.e_src.size(), 1u);
    DescBlob blob;
    // tv_sel is lut on every ordinary node, so it serves the multi-output launches as their table indices too
    const size_t off_at = blob.add(pl.off.data(), pl.off.size()), src_at = blob.add(pl.src.data(), pl.src.size()),
                 coef_at = blob.add(pl.coef.data(), pl.coef.size()), konst_at = blob.add(pl.konst.data(), n_nodes),
                 lut_at = blob.add(pl.tv_sel.data(), n_nodes), out_at = blob.add(pl.out_slots.data(), n_outputs),
                 shift_at = blob.add(shift.data(), shift.size()),
                 fan_at = multi ? blob.add(pl.fan.data(), pl.fan.size()) : 0,
                 eoff_at = select ? blob.add(pl.e_off.data(), pl.e_off.size()) : 0,
                 esrc_at = select ? blob.add(pl.e_src.data(), pl.e_src.size()) : 0,
                 one_at = select ? blob.add(ones.data(), ones.size()) : 0,
                 ekonst_at = select ? blob.add(pl.e_konst.data(), pl.e_konst.size()) : 0,
                 pcoef_at = select ? add_slot_coefs(blob, d.P.N, m) : 0,
                 zero_at = ext ? blob.reserve(1) : 0;  // the extraction's coefficient 0
    Frame f(d);
    Io io{f, dev};
    uint32_t *wires = f.take<uint32_t>(W * w);
    const uint32_t *desc = blob.upload(f);
    int rc = n_outputs ? io.out(outputs, n_outputs * w * 4) : f.rc();
    if (rc) return rc;
    if (n_inputs)
        HIPCHK(d, hipMemcpyAsync(wires, inputs, n_inputs * w * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                 d.stream));
    LutLevel L{};  // what every level shares; a level reads slots below its first and writes its own run
    L.wires = wires, L.tables = set.tables, L.src = desc + src_at;
    L.coef = reinterpret_cast<const int32_t *>(desc + coef_at);
    L.e_src = desc + esrc_at, L.ones = reinterpret_cast<const int32_t *>(desc + one_at);
    L.slot_coef = desc + pcoef_at, L.pk = pk, L.m = m, L.zero = desc + zero_at;
    for (uint32_t lv = 1; lv <= pl.depth; lv++) {
        // sfirst has depth + 1 entries in every plan (all 0 without select nodes), so e0 is read for every level
        const size_t at = pl.first[lv - 1], oat = pl.ofirst[lv - 1], e0 = (size_t)pl.sfirst[lv - 1] * m;
        L.off = desc + off_at + at + (lv - 1);
        L.konst = desc + konst_at + at, L.tv_sel = desc + lut_at + at;
        L.shift = desc + shift_at + at, L.fan = desc + fan_at + 2 * oat;
        L.nb = pl.first[lv] - at, L.no = pl.ofirst[lv] - oat, L.nsel = pl.nsel[lv - 1];
        std::copy_n(pl.neta.data() + 3 * (size_t)(lv - 1), 3, L.neta);
        std::copy_n(pl.nsel_eta.data() + 3 * (size_t)(lv - 1), 3, L.nsel_eta);
        L.e_off = desc + eoff_at + e0, L.e_konst = desc + ekonst_at + e0;
        L.out = wires + (n_inputs + oat) * w;
        if ((rc = lut_level_step(d, L))) return rc;
    }
    if (n_outputs) HIPCHK(d, launch_tlwe_gather(d.K, wires, desc + out_at, outputs, n_outputs, false, d.stream));
    return io.finish();
}

// What a flat entry was called with, as the C ABI names it.  BY_TABLE: nodes that read a table of the set (theta:
// NULL for the single-output entries).  BY_SELECT: select nodes, m entries each.  EACH: no nodes; pool is the B
// ciphertexts to bootstrap, tv their B test vectors.
struct LutBatch {
    const char *name;  // what the refusals call the entry
    enum Kind { BY_TABLE, BY_SELECT, EACH } kind;
    const tfhe_gpu_lut_set *set;
    const tfhe_gpu_packing_key *pk;
    uint32_t m, eta;
    const uint32_t *pool;
    size_t P;
    const uint32_t *term_off, *term_src;
    const int32_t *term_coef;
    const uint32_t *konst, *lut, *theta, *sel_src, *sel_konst, *tv;
    uint32_t *out;
    size_t B;
    bool dev;  // pool, tv and out are device pointers, and the call returns without waiting
};

// B nodes over a pool of P ciphertexts (checked arguments) as one level: its descriptors, every node in the
// group of the call's eta, the pool for the wires and out for the outputs.  multi: some theta is not 0.
static int lut_batch_on(Device &d, const LutBatch &a, bool multi) {
    if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const bool sel = a.kind == LutBatch::BY_SELECT;
    const size_t w = tlwe0_words(d.P), B = a.B, terms = a.term_off[B];
    std::vector<uint32_t> shift, fan, e_off(1, 0u), e_src, e_konst;
    if (multi) multi_descriptors(d.P, a.theta, B, shift, fan);
    const size_t M = multi ? fan.size() / 2 : B;
    for (size_t j = 0; sel && j < B * a.m; j++) {  // the entries as the combine kernel takes them
        const bool c = a.sel_src[j] == TFHE_LUT_ENTRY_CONST;
        if (!c) e_src.push_back(a.sel_src[j]);
        e_konst.push_back(c ? a.sel_konst[j] : 0u);
        e_off.push_back((uint32_t)e_src.size());
    }
    const std::vector<uint32_t> ones(e_src.size(), 1u);
    DescBlob blob;
    const size_t off_at = blob.add(a.term_off, B + 1), src_at = blob.add(a.term_src, terms),
                 coef_at = blob.add(a.term_coef, terms), konst_at = blob.add(a.konst, B),
                 tv_at = sel ? add_iota(blob, B) : blob.add(a.lut, B),  // select node b reads test vector b
                 shift_at = blob.add(shift.data(), shift.size()), fan_at = blob.add(fan.data(), fan.size()),
                 eoff_at = blob.add(e_off.data(), e_off.size()), esrc_at = blob.add(e_src.data(), e_src.size()),
                 one_at = blob.add(ones.data(), ones.size()), ekonst_at = blob.add(e_konst.data(), e_konst.size()),
                 pcoef_at = add_slot_coefs(blob, d.P.N, sel ? a.m : 0), zero_at = blob.reserve(1);
    Frame f(d);
    Io io{f, a.dev};
    const uint32_t *desc = blob.upload(f), *pool = a.pool;
    uint32_t *out = a.out;
    if (terms || !e_src.empty()) io.in(pool, a.P * w * 4);  // neither: the pool (may be NULL) is never read
    int rc = io.out(out, M * w * 4);
    if (rc) return rc;
    LutLevel L{};
    L.wires = pool, L.off = desc + off_at, L.src = desc + src_at;
    if (!sel) L.tables = a.set->tables;
    L.coef = reinterpret_cast<const int32_t *>(desc + coef_at);
    L.konst = desc + konst_at, L.tv_sel = desc + tv_at, L.shift = desc + shift_at, L.fan = desc + fan_at;
    L.nb = B, L.no = M, L.neta[a.eta] = (uint32_t)B;
    if (sel) L.nsel_eta[a.eta] = (uint32_t)B, L.nsel = B;
    L.e_off = desc + eoff_at, L.e_src = desc + esrc_at, L.ones = reinterpret_cast<const int32_t *>(desc + one_at);
    L.e_konst = desc + ekonst_at, L.slot_coef = desc + pcoef_at, L.pk = a.pk, L.m = a.m;
    L.zero = desc + zero_at, L.out = out;
    rc = lut_level_step(d, L);
    return rc ? rc : io.finish();
}

// B bootstraps with a test vector per item (checked arguments): the caller's inputs are x, item g reads tv + g * 2N.
static int lut_each_on(Device &d, const LutBatch &a) {
    if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t w = tlwe0_words(d.P), B = a.B;
    DescBlob blob;
    const size_t iota_at = add_iota(blob, B), zero_at = blob.reserve(1);
    Frame f(d);
    Io io{f, a.dev};
    const uint32_t *desc = blob.upload(f), *in = a.pool, *tv = a.tv;
    uint32_t *out = a.out;
    io.in(in, B * w * 4);
    io.in(tv, B * 2 * (size_t)d.P.N * sizeof(uint32_t));
    int rc = io.out(out, B * w * 4);
    if (rc) return rc;
    size_t n[3] = {0, 0, 0};
    n[a.eta] = B;
    rc = bootstrap_by_eta(d, f, in, nullptr, desc + iota_at, tv, n, desc + zero_at, out);
    return rc ? rc : io.finish();
}

// "", or what is wrong with packing m slots on this context's parameters, as `who` says it
static std::string select_m_bad(const tfhe_gpu_ctx *c, uint32_t m, const char *who = "select nodes") {
    const bool bad = m < 2 || (m & (m - 1)) || 2 * (uint64_t)m > c->P.N;
    return bad ? std::string(who) + ": m must be a power of two with 2 <= m and 2m <= N" : std::string();
}

// Every flat entry: the refusals, in one order (eta's range, null arguments, the context, the set or the key, m,
// then with B > 0 the sizes and the descriptors), and the run.  An eta of 0 is the entry without eta, limits and
// messages included.
static int batch_entry(tfhe_gpu_ctx *c, const LutBatch &a) {
    const bool tab = a.kind == LutBatch::BY_TABLE, sel = a.kind == LutBatch::BY_SELECT, nodes = tab || sel;
    const size_t B = a.B;
    const std::string name = a.name;
    if (a.eta > TFHE_LUT_EXT_MAX_LOG) return fail(c, TFHE_ERR_INVALID, name + ": eta > TFHE_LUT_EXT_MAX_LOG");
    const bool missing = nodes ? !a.term_off || !a.konst || (tab && !a.lut) || (sel && (!a.sel_src || !a.sel_konst))
                               : !a.pool || !a.tv;
    if (!c || (tab && !a.set) || (sel && !a.pk) || (B && (missing || !a.out)))
        return fail(c, TFHE_ERR_INVALID, "null argument");
    if (a.dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (tab)
        if (const int rc = set_mismatch(c, a.set, "LUT set")) return rc;
    if (sel) {
        if (const int rc = set_mismatch(c, a.pk, "packing key")) return rc;
        const std::string why = select_m_bad(c, a.m);
        if (!why.empty()) return fail(c, TFHE_ERR_INVALID, why);
    }
    if (B == 0) return TFHE_OK;
    // 2^32 - 1 items for the plain batches, 2^31 - 1 with an eta or entries; in nodes, entries or test vector words
    const uint64_t cap = (a.eta || sel ? 0x7FFFFFFFull : 0xFFFFFFFFull) / (sel ? a.m : nodes ? 1 : 2048);
    if (B > cap || a.P > 0xFFFFFFFFull)
        return fail(c, TFHE_ERR_INVALID, name + (nodes ? ": too many nodes or ciphertexts" : ": too many items"));
    bool multi = false;
    if (nodes) {
        if (a.term_off[B] && (!a.term_src || !a.term_coef || !a.pool)) return fail(c, TFHE_ERR_INVALID, "null argument");
        // the extended table t is the entries t E .. t E + E - 1: t < floor(T / E)
        if (const char *why = check_lut_nodes(B, a.P, tab ? a.set->T >> a.eta : 0, a.term_off, a.term_src, a.lut))
            return fail(c, TFHE_ERR_INVALID, (tab && a.eta ? "extended " : "") + name + ": " + why);
    }
    for (size_t i = 0; a.theta && i < B; i++) {
        if (a.theta[i] > TFHE_LUT_MULTI_MAX_LOG) return fail(c, TFHE_ERR_INVALID, name + ": theta > TFHE_LUT_MULTI_MAX_LOG");
        multi |= a.theta[i] != 0;
    }
    if (multi && B > 0xFFFFFFFFull >> TFHE_LUT_MULTI_MAX_LOG) return fail(c, TFHE_ERR_INVALID, name + ": too many outputs");
    for (size_t j = 0; sel && j < B * a.m; j++)
        if (a.sel_src[j] != TFHE_LUT_ENTRY_CONST && (a.sel_src[j] >= a.P || !a.pool))
            return fail(c, TFHE_ERR_INVALID, name + ": an entry is not a ciphertext of the pool");
    return on_device0(c, [&](Device &d) { return nodes ? lut_batch_on(d, a, multi) : lut_each_on(d, a); });
}

// A flat entry's arguments with the fields every kind has; the others stay NULL / 0 for the entry to set.
static LutBatch flat_batch(const char *name, LutBatch::Kind kind, uint32_t eta, const uint32_t *pool, uint32_t *out,
                           size_t B, bool dev) {
    LutBatch a{};
    a.name = name, a.kind = kind, a.eta = eta, a.pool = pool, a.out = out, a.B = B, a.dev = dev;
    return a;
}

// theta: NULL for the single-output entries; eta: 0 for the entries without one
static int apply_entry(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, uint32_t eta, const uint32_t *pool, size_t P,
                       const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef, const uint32_t *konst,
                       const uint32_t *lut, const uint32_t *theta, uint32_t *out, size_t B, bool dev) {
    LutBatch a = flat_batch("LUT batch", LutBatch::BY_TABLE, eta, pool, out, B, dev);
    a.set = set, a.P = P, a.term_off = term_off, a.term_src = term_src, a.term_coef = term_coef, a.konst = konst;
    a.lut = lut, a.theta = theta;
    return batch_entry(c, a);
}

static int select_entry(tfhe_gpu_ctx *c, const tfhe_gpu_packing_key *pk, uint32_t m, uint32_t eta, const uint32_t *pool,
                        size_t P, const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                        const uint32_t *konst, const uint32_t *sel_src, const uint32_t *sel_konst, uint32_t *out, size_t B,
                        bool dev) {
    LutBatch a = flat_batch("lut_select", LutBatch::BY_SELECT, eta, pool, out, B, dev);
    a.pk = pk, a.m = m, a.P = P, a.term_off = term_off, a.term_src = term_src, a.term_coef = term_coef, a.konst = konst;
    a.sel_src = sel_src, a.sel_konst = sel_konst;
    return batch_entry(c, a);
}

static int each_entry(tfhe_gpu_ctx *c, uint32_t eta, const uint32_t *in, const uint32_t *testvecs, uint32_t *out, size_t B,
                      bool dev) {
    LutBatch a = flat_batch("bootstrap_lut_each", LutBatch::EACH, eta, in, out, B, dev);
    a.tv = testvecs;
    return batch_entry(c, a);
}

static int circuit_entry(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, size_t n_inputs, const uint32_t *inputs,
                         size_t n_nodes, const uint32_t *term_off, const uint32_t *term_wire, const int32_t *term_coef,
                         const uint32_t *konst, const uint32_t *lut, const uint32_t *theta, size_t n_outputs,
                         const uint32_t *out_wires, uint32_t *outputs, uint32_t *levels, bool dev,
                         const tfhe_gpu_packing_key *pk = nullptr, const LutSelect *sel = nullptr,
                         const uint32_t *eta = nullptr) {
    if (!c || !set || (n_inputs && !inputs) || (n_nodes && (!term_off || !konst || !lut)) ||
        (n_outputs && (!out_wires || !outputs)) || (sel && !pk))
        return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (const int rc = set_mismatch(c, set, "LUT set")) return rc;
    if (sel) {
        if (const int rc = set_mismatch(c, pk, "packing key")) return rc;
        const std::string why = select_m_bad(c, sel->m);
        if (!why.empty()) return fail(c, TFHE_ERR_INVALID, why);
        if (n_nodes && sel->off[n_nodes] && (!sel->wire || !sel->konst)) return fail(c, TFHE_ERR_INVALID, "null argument");
    }
    if (n_nodes && term_off[n_nodes] && (!term_wire || !term_coef)) return fail(c, TFHE_ERR_INVALID, "null argument");
    LutCircuitPlan pl;
    if (const char *why = plan_lut_circuit(n_inputs, n_nodes, term_off, term_wire, term_coef, konst, lut, set->T,
                                           n_outputs, out_wires, pl, theta, sel, eta))
        return fail(c, TFHE_ERR_INVALID, std::string("LUT circuit: ") + why);
    const int rc = on_device0(c, [&](Device &d) {
        return lut_circuit_on(d, *set, n_inputs, inputs, n_nodes, pl, n_outputs, outputs, dev, pk, sel ? sel->m : 0);
    });
    if (!rc && levels) *levels = pl.depth;
    return rc;
}

// ---- Bivariate LUT bootstrap (include/tfhe_gpu.h): spread, the fused node ----

static int spread_entry(tfhe_gpu_ctx *c, const uint32_t *in, uint32_t w, uint32_t rot, uint32_t *out, size_t B, bool dev) {
    if (!c || (B && (!in || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (w == 0 || w > c->P.N || rot > 2 * c->P.N) return fail(c, TFHE_ERR_INVALID, "spread: w outside 1..N or rot > 2N");
    if (B > 0x7FFFFFFFull) return fail(c, TFHE_ERR_INVALID, "spread: too many items");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) -> int {
        const size_t bytes = B * 2 * (size_t)d.P.N * sizeof(uint32_t);
        Frame f(d);
        Io io{f, dev};
        int rc = io.in(in, bytes);
        if (!rc) rc = io.out(out, bytes);
        if (rc) return rc;
        d.last_br = d.last_ks = "";
        HIPCHK(d, launch_lut_spread(in, w, rot, out, B, d.stream, &d.last_br));
        return io.finish();
    });
}

// B bivariate nodes (checked arguments): per chunk of nodes, level 1 (m one-term nodes each, table fn*m + i),
// the pack into slots i*w, the spread in place, and level 2 with the chunk's test vectors.  The chunk is the
// pack's own (pack_chunk_items) in whole nodes, so the intermediates (m TLWELv0 in and out of level 1 per node,
// less than the sums of m items) stay within the same bound; every step is per item, so chunking changes no word.
static int lut_apply2_on(Device &d, const tfhe_gpu_lut_set &set, const tfhe_gpu_packing_key &pk, uint32_t m,
                         const uint32_t *pool, size_t P, const uint32_t *fn, const uint32_t *x_src, const uint32_t *y_src,
                         uint32_t *out, size_t B, bool dev) {
    if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t w = tlwe0_words(d.P), N = d.P.N, items = B * m;
    const uint32_t slot = (uint32_t)(N / m), rot = (uint32_t)(2 * N - N / (2 * m));
    const size_t nodes = std::min(B, std::max<size_t>(1, pack_chunk_items(d, items, (int)pk.basebit) / m));
    // descriptors: level 1 has one term per item (term k of item k: pool[y_src[b]], coefficient 1), level 2
    // one per node; off / ones / zeros serve both (level 1 is the longer)
    std::vector<uint32_t> off(items + 1), src1(items), lut1(items), ones(items, 1u), zeros(items, 0u);
    std::iota(off.begin(), off.end(), 0u);
    for (size_t b = 0; b < B; b++)
        for (uint32_t i = 0; i < m; i++) src1[b * m + i] = y_src[b], lut1[b * m + i] = fn[b] * m + i;
    DescBlob blob;
    const size_t off_at = blob.add(off.data(), items + 1), src1_at = blob.add(src1.data(), items),
                 lut1_at = blob.add(lut1.data(), items), one_at = blob.add(ones.data(), items),
                 zero_at = blob.add(zeros.data(), items), src2_at = blob.add(x_src, B),
                 coef_at = add_slot_coefs(blob, d.P.N, m), each_at = add_iota(blob, nodes);
    Frame f(d);
    Io io{f, dev};
    const uint32_t *desc = blob.upload(f);
    io.in(pool, P * w * 4);
    int rc = io.out(out, B * w * 4);
    // a chunk's combined ciphertexts, level 1's outputs (the pack's inputs) and test vectors: every chunk's alike
    uint32_t *x = f.take<uint32_t>(nodes * m * w), *g = f.ks_input<uint32_t>(nodes * m * w, /*pack*/ true);
    uint32_t *tv = f.take<uint32_t>(nodes * 2 * N);
    if ((rc = f.rc())) return rc;
    const uint32_t *off_d = desc + off_at, *zeros_d = desc + zero_at;
    const int32_t *ones_d = reinterpret_cast<const int32_t *>(desc + one_at);
    for (size_t b0 = 0; b0 < B; b0 += nodes) {
        const size_t nb = std::min(nodes, B - b0), ni = nb * m, n2[3] = {nb, 0, 0};
        // term_off = 0, 1, 2, .. with src advanced to the chunk: item k of the chunk has the one term k
        HIPCHK(d, launch_lut_combine(d.K, pool, off_d, desc + src1_at + b0 * m, ones_d, zeros_d, x, ni, d.stream));
        if ((rc = run_bootstrap_dev(d, nullptr, x, nullptr, set.tables, g, ni, RUN_BOOTSTRAP, nullptr,
                                    desc + lut1_at + b0 * m)))
            return rc;
        if ((rc = pack_launch(d, pk, g, desc + coef_at, m, tv, nb))) return rc;
        HIPCHK(d, launch_lut_spread(tv, slot, rot, tv, nb, d.stream));
        HIPCHK(d, launch_lut_combine(d.K, pool, off_d, desc + src2_at + b0, ones_d, zeros_d, x, nb, d.stream));
        // node k of the chunk reads the chunk's test vector k
        if ((rc = bootstrap_by_eta(d, f, x, nullptr, desc + each_at, tv, n2, nullptr, out + b0 * w))) return rc;
    }
    return io.finish();
}

static int apply2_entry(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk, uint32_t m,
                        const uint32_t *pool, size_t P, const uint32_t *fn, const uint32_t *x_src, const uint32_t *y_src,
                        uint32_t *out, size_t B, bool dev) {
    if (!c || !set || !pk || (B && (!pool || !fn || !x_src || !y_src || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (const int rc = set_mismatch(c, set, "LUT set")) return rc;
    if (const int rc = set_mismatch(c, pk, "packing key")) return rc;
    const std::string why = select_m_bad(c, m, "lut_apply2");
    if (!why.empty()) return fail(c, TFHE_ERR_INVALID, why);
    if (set->T % m) return fail(c, TFHE_ERR_INVALID, "lut_apply2: the set's size is not a multiple of m");
    if (B == 0) return TFHE_OK;
    if (B > 0xFFFFFFFFull / m - 1 || P > 0xFFFFFFFFull) return fail(c, TFHE_ERR_INVALID, "lut_apply2: too many nodes or ciphertexts");
    for (size_t b = 0; b < B; b++) {
        if (fn[b] >= set->T / m) return fail(c, TFHE_ERR_INVALID, "lut_apply2: fn * m + m exceeds the set");
        if (x_src[b] >= P || y_src[b] >= P) return fail(c, TFHE_ERR_INVALID, "lut_apply2: a source is not in the pool");
    }
    return on_device0(c, [&](Device &d) { return lut_apply2_on(d, *set, *pk, m, pool, P, fn, x_src, y_src, out, B, dev); });
}

// ---- Extended LUT bootstrap (include/tfhe_gpu.h): E = 2^eta accumulator components per item, eta = 1 or 2 ----

static int blind_rotate_ext_entry(tfhe_gpu_ctx *c, uint32_t eta, const uint32_t *in, const uint32_t *testvecs,
                                  uint32_t *out, size_t B) {
    if (!c || (B && (!in || !testvecs || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (eta > TFHE_LUT_EXT_MAX_LOG) return fail(c, TFHE_ERR_INVALID, "blind_rotate_ext: eta > TFHE_LUT_EXT_MAX_LOG");
    if (eta == 0) return tfhe_gpu_blind_rotate_batch(c, in, testvecs, out, B);
    if (B > 0x7FFFFFFFull >> eta) return fail(c, TFHE_ERR_INVALID, "blind_rotate_ext: too many items");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) -> int {
        if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
        const size_t w = tlwe0_words(d.P), E = (size_t)1 << eta, TRLWE_BYTES = 2 * (size_t)d.P.N * sizeof(uint32_t);
        Frame f(d);
        Io io{f, false};
        io.in(in, B * w * 4);
        io.in(testvecs, E * TRLWE_BYTES);
        int rc = io.out(out, B * E * TRLWE_BYTES);
        if (rc) return rc;
        if ((rc = blind_rotate_ext_launch(d, eta, in, testvecs, nullptr, out, /*all*/ true, B))) return rc;
        return io.finish();
    });
}

}  // namespace tfhe

extern "C" {

int tfhe_gpu_blind_rotate_ext_batch(tfhe_gpu_ctx *c, uint32_t eta, const uint32_t *in, const uint32_t *testvecs,
                                    uint32_t *out, size_t B) {
    return blind_rotate_ext_entry(c, eta, in, testvecs, out, B);
}

int tfhe_gpu_lut_apply_ext_batch(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, uint32_t eta, const uint32_t *pool,
                                 size_t P, const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                                 const uint32_t *konst, const uint32_t *lut, uint32_t *out, size_t B) {
    return apply_entry(c, set, eta, pool, P, term_off, term_src, term_coef, konst, lut, nullptr, out, B, false);
}

int tfhe_gpu_lut_apply_ext_dev(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, uint32_t eta, const uint32_t *pool_dev,
                               size_t P, const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                               const uint32_t *konst, const uint32_t *lut, uint32_t *out_dev, size_t B) {
    return apply_entry(c, set, eta, pool_dev, P, term_off, term_src, term_coef, konst, lut, nullptr, out_dev, B, true);
}

int tfhe_gpu_bootstrap_lut_each_ext_batch(tfhe_gpu_ctx *c, uint32_t eta, const uint32_t *in, const uint32_t *testvecs,
                                          uint32_t *out, size_t B) {
    return each_entry(c, eta, in, testvecs, out, B, false);
}

int tfhe_gpu_bootstrap_lut_each_ext_dev(tfhe_gpu_ctx *c, uint32_t eta, const uint32_t *in_dev,
                                        const uint32_t *testvecs_dev, uint32_t *out_dev, size_t B) {
    return each_entry(c, eta, in_dev, testvecs_dev, out_dev, B, true);
}

int tfhe_gpu_lut_spread_batch(tfhe_gpu_ctx *c, const uint32_t *in, uint32_t w, uint32_t rot, uint32_t *out, size_t B) {
    return spread_entry(c, in, w, rot, out, B, false);
}

int tfhe_gpu_lut_spread_dev(tfhe_gpu_ctx *c, const uint32_t *in_dev, uint32_t w, uint32_t rot, uint32_t *out_dev, size_t B) {
    return spread_entry(c, in_dev, w, rot, out_dev, B, true);
}

int tfhe_gpu_bootstrap_lut_each_batch(tfhe_gpu_ctx *c, const uint32_t *in, const uint32_t *testvecs, uint32_t *out,
                                      size_t B) {
    return each_entry(c, 0, in, testvecs, out, B, false);
}

int tfhe_gpu_bootstrap_lut_each_dev(tfhe_gpu_ctx *c, const uint32_t *in_dev, const uint32_t *testvecs_dev,
                                    uint32_t *out_dev, size_t B) {
    return each_entry(c, 0, in_dev, testvecs_dev, out_dev, B, true);
}

int tfhe_gpu_lut_apply2_batch(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk, uint32_t m,
                              const uint32_t *pool, size_t P, const uint32_t *fn, const uint32_t *x_src,
                              const uint32_t *y_src, uint32_t *out, size_t B) {
    return apply2_entry(c, set, pk, m, pool, P, fn, x_src, y_src, out, B, false);
}

int tfhe_gpu_lut_apply2_dev(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk, uint32_t m,
                            const uint32_t *pool_dev, size_t P, const uint32_t *fn, const uint32_t *x_src,
                            const uint32_t *y_src, uint32_t *out_dev, size_t B) {
    return apply2_entry(c, set, pk, m, pool_dev, P, fn, x_src, y_src, out_dev, B, true);
}

int tfhe_gpu_lut_set_load(tfhe_gpu_ctx *c, const uint32_t *testvecs, size_t T, tfhe_gpu_lut_set **out) {
    if (out) *out = nullptr;
    if (!c || !testvecs || !out || T == 0 || T > 0xFFFFFFFFull / 2048) return fail(c, TFHE_ERR_INVALID, "null argument or empty set");
    std::unique_ptr<tfhe_gpu_lut_set> set(new tfhe_gpu_lut_set);
    set->ctx = c;
    set->P = c->P;
    set->T = T;
    const int rc = on_device0(c, [&](Device &d) -> int {
        const size_t bytes = T * 2 * d.P.N * sizeof(uint32_t);
        if (hipMalloc((void **)set->tables.make(d.device), bytes) != hipSuccess)
            return fail(d, TFHE_ERR_OOM, "hipMalloc(LUT set)");
        HIPCHK(d, hipMemcpyAsync(set->tables, testvecs, bytes, hipMemcpyHostToDevice, d.stream));
        HIPCHK(d, hipStreamSynchronize(d.stream));
        return TFHE_OK;
    });
    if (rc) return rc;
    *out = set.release();
    return TFHE_OK;
}

void tfhe_gpu_lut_set_destroy(tfhe_gpu_lut_set *set) { delete set; }

int tfhe_gpu_lut_apply_batch(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const uint32_t *pool, size_t P,
                             const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                             const uint32_t *konst, const uint32_t *lut, uint32_t *out, size_t B) {
    return apply_entry(c, set, 0, pool, P, term_off, term_src, term_coef, konst, lut, nullptr, out, B, false);
}

int tfhe_gpu_lut_apply_dev(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const uint32_t *pool_dev, size_t P,
                           const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                           const uint32_t *konst, const uint32_t *lut, uint32_t *out_dev, size_t B) {
    return apply_entry(c, set, 0, pool_dev, P, term_off, term_src, term_coef, konst, lut, nullptr, out_dev, B, true);
}

int tfhe_gpu_lut_apply_multi_batch(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const uint32_t *pool, size_t P,
                                   const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                                   const uint32_t *konst, const uint32_t *lut, const uint32_t *theta, uint32_t *out,
                                   size_t B) {
    return apply_entry(c, set, 0, pool, P, term_off, term_src, term_coef, konst, lut, theta, out, B, false);
}

int tfhe_gpu_lut_apply_multi_dev(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const uint32_t *pool_dev, size_t P,
                                 const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                                 const uint32_t *konst, const uint32_t *lut, const uint32_t *theta, uint32_t *out_dev,
                                 size_t B) {
    return apply_entry(c, set, 0, pool_dev, P, term_off, term_src, term_coef, konst, lut, theta, out_dev, B, true);
}

int tfhe_gpu_lut_circuit_eval(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, size_t n_inputs, const uint32_t *inputs,
                              size_t n_nodes, const uint32_t *term_off, const uint32_t *term_wire,
                              const int32_t *term_coef, const uint32_t *konst, const uint32_t *lut, size_t n_outputs,
                              const uint32_t *out_wires, uint32_t *outputs, uint32_t *levels) {
    return circuit_entry(c, set, n_inputs, inputs, n_nodes, term_off, term_wire, term_coef, konst, lut, nullptr,
                         n_outputs, out_wires, outputs, levels, false);
}

int tfhe_gpu_lut_circuit_eval_dev(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, size_t n_inputs,
                                  const uint32_t *inputs_dev, size_t n_nodes, const uint32_t *term_off,
                                  const uint32_t *term_wire, const int32_t *term_coef, const uint32_t *konst,
                                  const uint32_t *lut, size_t n_outputs, const uint32_t *out_wires,
                                  uint32_t *outputs_dev, uint32_t *levels) {
    return circuit_entry(c, set, n_inputs, inputs_dev, n_nodes, term_off, term_wire, term_coef, konst, lut, nullptr,
                         n_outputs, out_wires, outputs_dev, levels, true);
}

int tfhe_gpu_lut_circuit_eval_multi(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, size_t n_inputs,
                                    const uint32_t *inputs, size_t n_nodes, const uint32_t *term_off,
                                    const uint32_t *term_wire, const int32_t *term_coef, const uint32_t *konst,
                                    const uint32_t *lut, const uint32_t *theta, size_t n_outputs,
                                    const uint32_t *out_wires, uint32_t *outputs, uint32_t *levels) {
    return circuit_entry(c, set, n_inputs, inputs, n_nodes, term_off, term_wire, term_coef, konst, lut, theta, n_outputs,
                         out_wires, outputs, levels, false);
}

int tfhe_gpu_lut_circuit_eval_multi_dev(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, size_t n_inputs,
                                        const uint32_t *inputs_dev, size_t n_nodes, const uint32_t *term_off,
                                        const uint32_t *term_wire, const int32_t *term_coef, const uint32_t *konst,
                                        const uint32_t *lut, const uint32_t *theta, size_t n_outputs,
                                        const uint32_t *out_wires, uint32_t *outputs_dev, uint32_t *levels) {
    return circuit_entry(c, set, n_inputs, inputs_dev, n_nodes, term_off, term_wire, term_coef, konst, lut, theta,
                         n_outputs, out_wires, outputs_dev, levels, true);
}

// sel_off == NULL: the _multi entry (pk and m are not looked at)
int tfhe_gpu_lut_circuit_eval_select(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk,
                                     uint32_t m, size_t n_inputs, const uint32_t *inputs, size_t n_nodes,
                                     const uint32_t *term_off, const uint32_t *term_wire, const int32_t *term_coef,
                                     const uint32_t *konst, const uint32_t *lut, const uint32_t *theta,
                                     const uint32_t *sel_off, const uint32_t *sel_wire, const uint32_t *sel_konst,
                                     size_t n_outputs, const uint32_t *out_wires, uint32_t *outputs, uint32_t *levels) {
    const LutSelect sel{m, sel_off, sel_wire, sel_konst};
    return circuit_entry(c, set, n_inputs, inputs, n_nodes, term_off, term_wire, term_coef, konst, lut, theta, n_outputs,
                         out_wires, outputs, levels, false, pk, sel_off ? &sel : nullptr);
}

int tfhe_gpu_lut_circuit_eval_select_dev(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk,
                                         uint32_t m, size_t n_inputs, const uint32_t *inputs_dev, size_t n_nodes,
                                         const uint32_t *term_off, const uint32_t *term_wire, const int32_t *term_coef,
                                         const uint32_t *konst, const uint32_t *lut, const uint32_t *theta,
                                         const uint32_t *sel_off, const uint32_t *sel_wire, const uint32_t *sel_konst,
                                         size_t n_outputs, const uint32_t *out_wires, uint32_t *outputs_dev,
                                         uint32_t *levels) {
    const LutSelect sel{m, sel_off, sel_wire, sel_konst};
    return circuit_entry(c, set, n_inputs, inputs_dev, n_nodes, term_off, term_wire, term_coef, konst, lut, theta,
                         n_outputs, out_wires, outputs_dev, levels, true, pk, sel_off ? &sel : nullptr);
}

int tfhe_gpu_lut_select_batch(tfhe_gpu_ctx *c, const tfhe_gpu_packing_key *pk, uint32_t m, const uint32_t *pool, size_t P,
                              const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                              const uint32_t *konst, const uint32_t *sel_src, const uint32_t *sel_konst, uint32_t *out,
                              size_t B) {
    return select_entry(c, pk, m, 0, pool, P, term_off, term_src, term_coef, konst, sel_src, sel_konst, out, B, false);
}

int tfhe_gpu_lut_select_dev(tfhe_gpu_ctx *c, const tfhe_gpu_packing_key *pk, uint32_t m, const uint32_t *pool_dev,
                            size_t P, const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                            const uint32_t *konst, const uint32_t *sel_src, const uint32_t *sel_konst, uint32_t *out_dev,
                            size_t B) {
    return select_entry(c, pk, m, 0, pool_dev, P, term_off, term_src, term_coef, konst, sel_src, sel_konst, out_dev, B,
                        true);
}

int tfhe_gpu_lut_select_ext_batch(tfhe_gpu_ctx *c, const tfhe_gpu_packing_key *pk, uint32_t m, uint32_t eta,
                                  const uint32_t *pool, size_t P, const uint32_t *term_off, const uint32_t *term_src,
                                  const int32_t *term_coef, const uint32_t *konst, const uint32_t *sel_src,
                                  const uint32_t *sel_konst, uint32_t *out, size_t B) {
    return select_entry(c, pk, m, eta, pool, P, term_off, term_src, term_coef, konst, sel_src, sel_konst, out, B, false);
}

int tfhe_gpu_lut_select_ext_dev(tfhe_gpu_ctx *c, const tfhe_gpu_packing_key *pk, uint32_t m, uint32_t eta,
                                const uint32_t *pool_dev, size_t P, const uint32_t *term_off, const uint32_t *term_src,
                                const int32_t *term_coef, const uint32_t *konst, const uint32_t *sel_src,
                                const uint32_t *sel_konst, uint32_t *out_dev, size_t B) {
    return select_entry(c, pk, m, eta, pool_dev, P, term_off, term_src, term_coef, konst, sel_src, sel_konst, out_dev, B,
                        true);
}

// eta == NULL: the _select entry
int tfhe_gpu_lut_circuit_eval_ext(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk, uint32_t m,
                                  size_t n_inputs, const uint32_t *inputs, size_t n_nodes, const uint32_t *term_off,
                                  const uint32_t *term_wire, const int32_t *term_coef, const uint32_t *konst,
                                  const uint32_t *lut, const uint32_t *theta, const uint32_t *sel_off,
                                  const uint32_t *sel_wire, const uint32_t *sel_konst, const uint32_t *eta,
                                  size_t n_outputs, const uint32_t *out_wires, uint32_t *outputs, uint32_t *levels) {
    const LutSelect sel{m, sel_off, sel_wire, sel_konst};
    return circuit_entry(c, set, n_inputs, inputs, n_nodes, term_off, term_wire, term_coef, konst, lut, theta, n_outputs,
                         out_wires, outputs, levels, false, pk, sel_off ? &sel : nullptr, eta);
}

int tfhe_gpu_lut_circuit_eval_ext_dev(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk,
                                      uint32_t m, size_t n_inputs, const uint32_t *inputs_dev, size_t n_nodes,
                                      const uint32_t *term_off, const uint32_t *term_wire, const int32_t *term_coef,
                                      const uint32_t *konst, const uint32_t *lut, const uint32_t *theta,
                                      const uint32_t *sel_off, const uint32_t *sel_wire, const uint32_t *sel_konst,
                                      const uint32_t *eta, size_t n_outputs, const uint32_t *out_wires,
                                      uint32_t *outputs_dev, uint32_t *levels) {
    const LutSelect sel{m, sel_off, sel_wire, sel_konst};
    return circuit_entry(c, set, n_inputs, inputs_dev, n_nodes, term_off, term_wire, term_coef, konst, lut, theta,
                         n_outputs, out_wires, outputs_dev, levels, true, pk, sel_off ? &sel : nullptr, eta);
}

}  // extern "C"
