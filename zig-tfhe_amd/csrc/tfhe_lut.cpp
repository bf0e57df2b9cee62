// tfhe_lut.cpp — LUT circuits of the C ABI (include/tfhe_gpu.h): resident sets
// of test vectors, batches of "linear combination, then programmable bootstrap
// with the node's own table", and the level-scheduled evaluator for DAGs of such
// nodes.  Host code: the combination runs in tfhe_kernels_lut.hip, the bootstrap
// is run_bootstrap_dev with a per-item table selector (KParams::tv_sel), and the
// planner is in tfhe_cpu.cpp.  A multi-output node (theta > 0) rounds x in the
// combine kernel, keeps the accumulator (RUN_TRLWE) and extracts its first 2^theta
// coefficients in front of one key switch over the outputs.  The bivariate node
// (lut_apply2_on) chains level 1, the pack (pack_launch, tfhe_pack.cpp), the spread
// (k_lut_spread) and a bootstrap whose per-item selector is the identity over the
// chunk's own test vectors.  A select node (select_testvecs) is the same chain inside the
// circuit evaluator, its m tables' outputs replaced by any earlier wires or constants, and
// shares its level's bootstrap launch with the ordinary nodes (KParams::tv_each).  The extended
// bootstrap (lut_apply_ext_on) is lut_apply_on with k_blind_rotate_ext (tfhe_kernels_lut_ext.hip) on
// 2^eta accumulator components in place of the blind rotation, then the extraction and the key switch.
// Extended nodes (lut_circuit_on with the plan's eta groups) run it inside the circuit
// evaluator: a select node's extended test vector is E copies of its ordinary one, so the level's one pack
// serves every eta, and each eta > 0 has one k_blind_rotate_ext launch over its ordinary and select nodes
// (BrExtBatch::tv_each); each_ext_entry and lut_select_on with an eta are the flat forms.
// Everything here runs on the context's first device.
#include "tfhe_gpu.h"

#include <algorithm>
#include <cstring>
#include <memory>
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

// B nodes over a pool of P ciphertexts (checked descriptors).  dev: pool and out are
// device pointers, and the call returns without waiting.
static int lut_apply_on(Device &d, const tfhe_gpu_lut_set &set, const uint32_t *pool, size_t P, const uint32_t *term_off,
                        const uint32_t *term_src, const int32_t *term_coef, const uint32_t *konst, const uint32_t *lut,
                        uint32_t *out, size_t B, bool dev) {
    if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t w = tlwe0_words(d.P), terms = term_off[B];
    DescBlob blob;
    const size_t off_at = blob.add(term_off, B + 1), src_at = blob.add(term_src, terms),
                 coef_at = blob.add(term_coef, terms), konst_at = blob.add(konst, B), lut_at = blob.add(lut, B);
    Frame f(d);
    Io io{f, dev};
    const uint32_t *desc = blob.upload(f);
    if (terms) io.in(pool, P * w * 4);  // no terms: the pool (may be NULL) is never read
    int rc = io.out(out, B * w * 4);
    uint32_t *x = f.take<uint32_t>(B * w);  // the combined ciphertexts, the bootstrap's inputs
    if ((rc = f.rc())) return rc;
    HIPCHK(d, launch_lut_combine(d.K, pool, desc + off_at, desc + src_at, reinterpret_cast<const int32_t *>(desc + coef_at),
                                 desc + konst_at, x, B, d.stream));
    rc = run_bootstrap_dev(d, nullptr, x, nullptr, set.tables, out, B, RUN_BOOTSTRAP, nullptr, desc + lut_at);
    return rc ? rc : io.finish();
}

// The multi-output form of a launch of B nodes with M >= B outputs: x (rounded per node by shift[])
// -> one accumulator per node -> the M extractions fan[] names -> one key switch into out
// (M TLWELv0).  desc pointers are device copies.  x, the accumulators and the extractions are the launch's own.
static int lut_multi_launch(Device &d, const tfhe_gpu_lut_set &set, const uint32_t *pool, const uint32_t *off,
                            const uint32_t *src, const int32_t *coef, const uint32_t *konst, const uint32_t *lut,
                            const uint32_t *shift, const uint32_t *fan, uint32_t *out, size_t B, size_t M) {
    Frame f(d);
    uint32_t *x = f.take<uint32_t>(B * tlwe0_words(d.P)), *acc = f.take<uint32_t>(B * 2 * (size_t)d.P.N);
    uint32_t *lv1 = f.ks_input<uint32_t>(M * 1025);
    int rc = f.rc();
    if (rc) return rc;
    HIPCHK(d, launch_lut_combine_round(d.K, pool, off, src, coef, konst, shift, x, B, d.stream));
    const size_t ev_at = d.ev_used;
    if ((rc = run_bootstrap_dev(d, nullptr, x, nullptr, set.tables, acc, B, RUN_TRLWE, nullptr, lut))) return rc;
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

// lut_apply_on for nodes of which one at least has theta > 0: out takes sum 2^theta[i] ciphertexts.
static int lut_apply_multi_on(Device &d, const tfhe_gpu_lut_set &set, const uint32_t *pool, size_t P,
                              const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                              const uint32_t *konst, const uint32_t *lut, const uint32_t *theta, uint32_t *out, size_t B,
                              bool dev) {
    if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t w = tlwe0_words(d.P), terms = term_off[B];
    std::vector<uint32_t> shift, fan;
    multi_descriptors(d.P, theta, B, shift, fan);
    const size_t M = fan.size() / 2;
    DescBlob blob;
    const size_t off_at = blob.add(term_off, B + 1), src_at = blob.add(term_src, terms),
                 coef_at = blob.add(term_coef, terms), konst_at = blob.add(konst, B), lut_at = blob.add(lut, B),
                 shift_at = blob.add(shift.data(), B), fan_at = blob.add(fan.data(), fan.size());
    Frame f(d);
    Io io{f, dev};
    const uint32_t *desc = blob.upload(f);
    if (terms) io.in(pool, P * w * 4);
    int rc = io.out(out, M * w * 4);
    if (rc) return rc;
    rc = lut_multi_launch(d, set, pool, desc + off_at, desc + src_at, reinterpret_cast<const int32_t *>(desc + coef_at),
                          desc + konst_at, desc + lut_at, desc + shift_at, desc + fan_at, out, B, M);
    return rc ? rc : io.finish();
}

static_assert(LUT_TV_EACH == TV_SEL_EACH, "the planner's selector bit is the kernels'");

// The selector of a bootstrap whose item g reads testvecs + g * 2N: 0 .. B-1, appended to a call's descriptors.
// mask: LUT_TV_EACH for the extended blind rotation, whose selector names the caller's buffer by that bit.
static size_t add_iota(DescBlob &blob, size_t B, uint32_t mask = 0) {
    const size_t at = blob.words.size();
    for (size_t i = 0; i < B; i++) blob.words.push_back((uint32_t)i | mask);
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

// A whole LUT circuit: one combine and one bootstrap launch per level into the
// wire table (in the plan's slot order), the outputs gathered at the end; a level's temporaries go with its frame.
// A level with select nodes (pk, m: theirs) builds their test vectors first; its one bootstrap launch then reads,
// item by item, the set or those (the plan's tv_sel, KParams::tv_each).  Extended nodes (the plan's eta groups) share
// the level's combination launch and its select nodes' pack, and run one k_blind_rotate_ext launch per eta, one
// extraction and one key switch behind the level's eta = 0 launches; without them a level runs what it ran before.
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
    const int32_t *coef = reinterpret_cast<const int32_t *>(desc + coef_at);
    for (uint32_t lv = 1; lv <= pl.depth; lv++) {
        const size_t at = pl.first[lv - 1], nb = pl.first[lv] - at, oat = pl.ofirst[lv - 1], no = pl.ofirst[lv] - oat;
        // the level's run: its eta = 0 nodes (ordinary, then select), then its eta = 1 and its eta = 2 nodes (the same)
        const uint32_t *ne = pl.neta.data() + 3 * (size_t)(lv - 1), *nse = pl.nsel_eta.data() + 3 * (size_t)(lv - 1);
        const size_t next = (size_t)ne[1] + ne[2], nb0 = nb - next, no0 = no - next;  // an extended node has one output
        const size_t ns = pl.nsel[lv - 1], ns0 = nse[0], nord = nb0 - ns0;
        const uint32_t *off = desc + off_at + at + (lv - 1);
        uint32_t *level_out = wires + (n_inputs + oat) * w;  // the level's outputs: one run of slots
        // reads slots below this level's first (earlier wires), writes the level's staging slices
        Frame level(d);
        uint32_t *tv = nullptr;
        if (ns) {  // the test vectors of all of the level's select nodes, whatever their eta
            tv = level.take<uint32_t>(ns * 2 * (size_t)d.P.N);
            if ((rc = level.rc())) return rc;
            const size_t e0 = (size_t)pl.sfirst[lv - 1] * m;
            rc = select_testvecs(d, *pk, m, wires, desc + eoff_at + e0, desc + esrc_at,
                                 reinterpret_cast<const int32_t *>(desc + one_at), desc + ekonst_at + e0,
                                 desc + pcoef_at, tv, ns);
            if (rc) return rc;
        }
        // a theta > 0 in this level: the ordinary nodes as before, the select nodes in one launch of their own
        const bool split = no0 != nb0;
        if (split) {
            rc = lut_multi_launch(d, set, wires, off, desc + src_at, coef, desc + konst_at + at, desc + lut_at + at,
                                  desc + shift_at + at, desc + fan_at + 2 * oat, level_out, nord, no0 - ns0);
            if (rc) return rc;
        }
        // one combination launch over the rest: the eta = 0 items of the bootstrap launch, then the extended groups
        const size_t skip = split ? nord : 0, items = nb - skip, items0 = nb0 - skip;
        if (!items) continue;
        uint32_t *x = level.take<uint32_t>(items * w);
        if ((rc = level.rc())) return rc;
        HIPCHK(d, launch_lut_combine(d.K, wires, off + skip, desc + src_at, coef, desc + konst_at + at + skip, x, items,
                                     d.stream));
        if (items0) {
            rc = run_bootstrap_dev(d, nullptr, x, nullptr, set.tables, level_out + (no0 - items0) * w, items0,
                                   RUN_BOOTSTRAP, nullptr, desc + lut_at + at + skip, tv);
            if (rc) return rc;
        }
        if (!next) continue;
        // one extended blind rotation per eta present (acc_0 of each item), then one extraction and one key switch
        // over both groups into the slots behind the eta = 0 outputs
        uint32_t *acc = level.take<uint32_t>(next * 2 * (size_t)d.P.N), *lv1 = level.ks_input<uint32_t>(next * 1025);
        if ((rc = level.rc())) return rc;
        for (size_t e = 1, done = 0; e <= 2; done += ne[e], e++) {
            if (!ne[e]) continue;
            rc = blind_rotate_ext_launch(d, (uint32_t)e, x + (items0 + done) * w, set.tables, desc + lut_at + at + nb0 + done,
                                         acc + done * 2 * (size_t)d.P.N, /*all*/ false, ne[e], tv);
            if (rc) return rc;
        }
        if ((rc = ext_extract_ks(d, level, acc, desc + zero_at, lv1, level_out + no0 * w, next))) return rc;
    }
    if (n_outputs) HIPCHK(d, launch_tlwe_gather(d.K, wires, desc + out_at, outputs, n_outputs, false, d.stream));
    return io.finish();
}

// B select nodes over a pool of P ciphertexts (checked descriptors): x, the B test vectors, and the bootstrap
// whose item b reads test vector b.
static int lut_select_on(Device &d, const tfhe_gpu_packing_key &pk, uint32_t m, const uint32_t *pool, size_t P,
                         const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                         const uint32_t *konst, const uint32_t *sel_src, const uint32_t *sel_konst, uint32_t *out,
                         size_t B, bool dev, uint32_t eta = 0) {
    if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t w = tlwe0_words(d.P), terms = term_off[B], E = B * m;
    std::vector<uint32_t> e_off(1, 0u), e_src, e_konst(E);
    for (size_t j = 0; j < E; j++) {
        const bool c = sel_src[j] == TFHE_LUT_ENTRY_CONST;
        if (!c) e_src.push_back(sel_src[j]);
        e_konst[j] = c ? sel_konst[j] : 0u;
        e_off.push_back((uint32_t)e_src.size());
    }
    const std::vector<uint32_t> ones(e_src.size(), 1u);
    DescBlob blob;
    const size_t off_at = blob.add(term_off, B + 1), src_at = blob.add(term_src, terms),
                 coef_at = blob.add(term_coef, terms), konst_at = blob.add(konst, B),
                 eoff_at = blob.add(e_off.data(), e_off.size()), esrc_at = blob.add(e_src.data(), e_src.size()),
                 one_at = blob.add(ones.data(), ones.size()), ekonst_at = blob.add(e_konst.data(), E),
                 pcoef_at = add_slot_coefs(blob, d.P.N, m), iota_at = add_iota(blob, B, eta ? LUT_TV_EACH : 0),
                 zero_at = blob.reserve(1);  // the extraction's coefficient 0 (eta > 0)
    Frame f(d);
    Io io{f, dev};
    const uint32_t *desc = blob.upload(f);
    if (terms || !e_src.empty()) io.in(pool, P * w * 4);  // neither: the pool (may be NULL) is never read
    int rc = io.out(out, B * w * 4);
    uint32_t *x = f.take<uint32_t>(B * w), *tv = f.take<uint32_t>(B * 2 * (size_t)d.P.N);
    // eta > 0: acc_0 of each item and the key switch's input
    uint32_t *acc = eta ? f.take<uint32_t>(B * 2 * (size_t)d.P.N) : nullptr;
    uint32_t *lv1 = eta ? f.ks_input<uint32_t>(B * 1025) : nullptr;
    if ((rc = f.rc())) return rc;
    HIPCHK(d, launch_lut_combine(d.K, pool, desc + off_at, desc + src_at, reinterpret_cast<const int32_t *>(desc + coef_at),
                                 desc + konst_at, x, B, d.stream));
    rc = select_testvecs(d, pk, m, pool, desc + eoff_at, desc + esrc_at, reinterpret_cast<const int32_t *>(desc + one_at),
                         desc + ekonst_at, desc + pcoef_at, tv, B);
    if (rc) return rc;
    if (eta) {  // every item reads its own test vector in all E components
        rc = blind_rotate_ext_launch(d, eta, x, nullptr, desc + iota_at, acc, /*all*/ false, B, tv);
        if (!rc) rc = ext_extract_ks(d, f, acc, desc + zero_at, lv1, out, B);
    } else {
        rc = run_bootstrap_dev(d, nullptr, x, nullptr, tv, out, B, RUN_BOOTSTRAP, nullptr, desc + iota_at);
    }
    return rc ? rc : io.finish();
}

// theta: NULL for the single-output entries
static int apply_entry(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const uint32_t *pool, size_t P,
                       const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef, const uint32_t *konst,
                       const uint32_t *lut, const uint32_t *theta, uint32_t *out, size_t B, bool dev) {
    if (!c || !set || (B && (!term_off || !konst || !lut || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (const int rc = set_mismatch(c, set, "LUT set")) return rc;
    if (B == 0) return TFHE_OK;
    if (B > 0xFFFFFFFFull || P > 0xFFFFFFFFull) return fail(c, TFHE_ERR_INVALID, "LUT batch: too many nodes or ciphertexts");
    if (term_off[B] && (!term_src || !term_coef || !pool)) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (const char *why = check_lut_nodes(B, P, set->T, term_off, term_src, lut))
        return fail(c, TFHE_ERR_INVALID, std::string("LUT batch: ") + why);
    bool multi = false;
    for (size_t i = 0; theta && i < B; i++) {
        if (theta[i] > TFHE_LUT_MULTI_MAX_LOG) return fail(c, TFHE_ERR_INVALID, "LUT batch: theta > TFHE_LUT_MULTI_MAX_LOG");
        multi |= theta[i] != 0;
    }
    if (multi && B > 0xFFFFFFFFull >> TFHE_LUT_MULTI_MAX_LOG) return fail(c, TFHE_ERR_INVALID, "LUT batch: too many outputs");
    return on_device0(c, [&](Device &d) {
        // all thetas 0: exactly the single-output path
        return multi ? lut_apply_multi_on(d, *set, pool, P, term_off, term_src, term_coef, konst, lut, theta, out, B, dev)
                     : lut_apply_on(d, *set, pool, P, term_off, term_src, term_coef, konst, lut, out, B, dev);
    });
}

// nullptr, or what is wrong with a select node's m on this context's parameters (lut_apply2's conditions)
static const char *select_m_bad(const tfhe_gpu_ctx *c, uint32_t m) {
    return m < 2 || (m & (m - 1)) || 2 * (uint64_t)m > c->P.N
               ? "select nodes: m must be a power of two with 2 <= m and 2m <= N"
               : nullptr;
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
        if (const char *why = select_m_bad(c, sel->m)) return fail(c, TFHE_ERR_INVALID, why);
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

static int select_entry(tfhe_gpu_ctx *c, const tfhe_gpu_packing_key *pk, uint32_t m, const uint32_t *pool, size_t P,
                        const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                        const uint32_t *konst, const uint32_t *sel_src, const uint32_t *sel_konst, uint32_t *out, size_t B,
                        bool dev, uint32_t eta = 0) {
    if (eta > TFHE_LUT_EXT_MAX_LOG) return fail(c, TFHE_ERR_INVALID, "lut_select: eta > TFHE_LUT_EXT_MAX_LOG");
    if (!c || !pk || (B && (!term_off || !konst || !sel_src || !sel_konst || !out)))
        return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (const int rc = set_mismatch(c, pk, "packing key")) return rc;
    if (const char *why = select_m_bad(c, m)) return fail(c, TFHE_ERR_INVALID, why);
    if (B == 0) return TFHE_OK;
    if (B > 0x7FFFFFFFull / m || P > 0xFFFFFFFFull) return fail(c, TFHE_ERR_INVALID, "lut_select: too many nodes or ciphertexts");
    if (term_off[B] && (!term_src || !term_coef || !pool)) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (const char *why = check_lut_nodes(B, P, 0, term_off, term_src, nullptr))
        return fail(c, TFHE_ERR_INVALID, std::string("lut_select: ") + why);
    for (size_t j = 0; j < B * m; j++)
        if (sel_src[j] != TFHE_LUT_ENTRY_CONST && (sel_src[j] >= P || !pool))
            return fail(c, TFHE_ERR_INVALID, "lut_select: an entry is not a ciphertext of the pool");
    return on_device0(c, [&](Device &d) {
        return lut_select_on(d, *pk, m, pool, P, term_off, term_src, term_coef, konst, sel_src, sel_konst, out, B, dev,
                             eta);
    });
}

// ---- Bivariate LUT bootstrap (include/tfhe_gpu.h): spread, a test vector per item, the fused node ----

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

static int each_entry(tfhe_gpu_ctx *c, const uint32_t *in, const uint32_t *testvecs, uint32_t *out, size_t B, bool dev) {
    if (!c || (B && (!in || !testvecs || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (B > 0xFFFFFFFFull / 2048) return fail(c, TFHE_ERR_INVALID, "bootstrap_lut_each: too many items");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) -> int {
        if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
        const size_t w = tlwe0_words(d.P);
        DescBlob blob;
        add_iota(blob, B);
        Frame f(d);
        Io io{f, dev};
        const uint32_t *iota = blob.upload(f);
        io.in(in, B * w * 4);
        io.in(testvecs, B * 2 * (size_t)d.P.N * sizeof(uint32_t));
        int rc = io.out(out, B * w * 4);
        if (rc) return rc;
        rc = run_bootstrap_dev(d, nullptr, in, nullptr, testvecs, out, B, RUN_BOOTSTRAP, nullptr, iota);
        return rc ? rc : io.finish();
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
    // one per node; ones / zeros / iota serve both (level 1 is the longer)
    std::vector<uint32_t> src1(items), lut1(items), ones(items, 1u), zeros(items, 0u), coef(m);
    for (size_t b = 0; b < B; b++)
        for (uint32_t i = 0; i < m; i++) src1[b * m + i] = y_src[b], lut1[b * m + i] = fn[b] * m + i;
    for (uint32_t i = 0; i < m; i++) coef[i] = i * slot;
    DescBlob blob;
    const size_t iota_at = add_iota(blob, items + 1), src1_at = blob.add(src1.data(), items),
                 lut1_at = blob.add(lut1.data(), items), one_at = blob.add(ones.data(), items),
                 zero_at = blob.add(zeros.data(), items), src2_at = blob.add(x_src, B), coef_at = blob.add(coef.data(), m);
    Frame f(d);
    Io io{f, dev};
    const uint32_t *desc = blob.upload(f);
    io.in(pool, P * w * 4);
    int rc = io.out(out, B * w * 4);
    // a chunk's combined ciphertexts, level 1's outputs (the pack's inputs) and test vectors: every chunk's alike
    uint32_t *x = f.take<uint32_t>(nodes * m * w), *g = f.ks_input<uint32_t>(nodes * m * w, /*pack*/ true);
    uint32_t *tv = f.take<uint32_t>(nodes * 2 * N);
    if ((rc = f.rc())) return rc;
    const uint32_t *iota = desc + iota_at, *zeros_d = desc + zero_at;
    const int32_t *ones_d = reinterpret_cast<const int32_t *>(desc + one_at);
    for (size_t b0 = 0; b0 < B; b0 += nodes) {
        const size_t nb = std::min(nodes, B - b0), ni = nb * m;
        // term_off = iota from 0 with src advanced to the chunk: item k of the chunk has the one term k
        HIPCHK(d, launch_lut_combine(d.K, pool, iota, desc + src1_at + b0 * m, ones_d, zeros_d, x, ni, d.stream));
        if ((rc = run_bootstrap_dev(d, nullptr, x, nullptr, set.tables, g, ni, RUN_BOOTSTRAP, nullptr,
                                    desc + lut1_at + b0 * m)))
            return rc;
        if ((rc = pack_launch(d, pk, g, desc + coef_at, m, tv, nb))) return rc;
        HIPCHK(d, launch_lut_spread(tv, slot, rot, tv, nb, d.stream));
        HIPCHK(d, launch_lut_combine(d.K, pool, iota, desc + src2_at + b0, ones_d, zeros_d, x, nb, d.stream));
        if ((rc = run_bootstrap_dev(d, nullptr, x, nullptr, tv, out + b0 * w, nb, RUN_BOOTSTRAP, nullptr, iota))) return rc;
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
    if (m < 2 || (m & (m - 1)) || 2 * (uint64_t)m > c->P.N)
        return fail(c, TFHE_ERR_INVALID, "lut_apply2: m must be a power of two with 2 <= m and 2m <= N");
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

// bootstrap_lut_each with the extended bootstrap: item i's one test vector serves all E components.
static int each_ext_entry(tfhe_gpu_ctx *c, uint32_t eta, const uint32_t *in, const uint32_t *testvecs, uint32_t *out,
                          size_t B, bool dev) {
    if (eta > TFHE_LUT_EXT_MAX_LOG) return fail(c, TFHE_ERR_INVALID, "bootstrap_lut_each: eta > TFHE_LUT_EXT_MAX_LOG");
    if (eta == 0) return each_entry(c, in, testvecs, out, B, dev);  // exactly the existing entry
    if (!c || (B && (!in || !testvecs || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (B > 0x7FFFFFFFull / 2048) return fail(c, TFHE_ERR_INVALID, "bootstrap_lut_each: too many items");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) -> int {
        if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
        const size_t w = tlwe0_words(d.P), TRLWE = 2 * (size_t)d.P.N;
        DescBlob blob;
        const size_t iota_at = add_iota(blob, B, LUT_TV_EACH), zero_at = blob.reserve(1);
        Frame f(d);
        Io io{f, dev};
        const uint32_t *desc = blob.upload(f);
        io.in(in, B * w * 4);
        io.in(testvecs, B * TRLWE * sizeof(uint32_t));
        int rc = io.out(out, B * w * 4);
        uint32_t *acc = f.take<uint32_t>(B * TRLWE), *lv1 = f.ks_input<uint32_t>(B * 1025);
        if ((rc = f.rc())) return rc;
        if ((rc = blind_rotate_ext_launch(d, eta, in, nullptr, desc + iota_at, acc, /*all*/ false, B, testvecs))) return rc;
        if ((rc = ext_extract_ks(d, f, acc, desc + zero_at, lv1, out, B))) return rc;
        return io.finish();
    });
}

// lut_apply_on with the extended bootstrap (checked descriptors): the same combination launch, the extended
// blind rotation with the item's extended table lut[i], then sampleExtractIndex(acc_0, 0) and the key switch.
static int lut_apply_ext_on(Device &d, const tfhe_gpu_lut_set &set, uint32_t eta, const uint32_t *pool, size_t P,
                            const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                            const uint32_t *konst, const uint32_t *lut, uint32_t *out, size_t B, bool dev) {
    if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t w = tlwe0_words(d.P), terms = term_off[B];
    DescBlob blob;
    const size_t off_at = blob.add(term_off, B + 1), src_at = blob.add(term_src, terms),
                 coef_at = blob.add(term_coef, terms), konst_at = blob.add(konst, B), lut_at = blob.add(lut, B),
                 zero_at = blob.reserve(1);  // the extraction's coefficient 0
    Frame f(d);
    Io io{f, dev};
    const uint32_t *desc = blob.upload(f);
    if (terms) io.in(pool, P * w * 4);  // no terms: the pool (may be NULL) is never read
    int rc = io.out(out, B * w * 4);
    uint32_t *x = f.take<uint32_t>(B * w), *acc = f.take<uint32_t>(B * 2 * (size_t)d.P.N);
    uint32_t *lv1 = f.ks_input<uint32_t>(B * 1025);
    if ((rc = f.rc())) return rc;
    HIPCHK(d, launch_lut_combine(d.K, pool, desc + off_at, desc + src_at, reinterpret_cast<const int32_t *>(desc + coef_at),
                                 desc + konst_at, x, B, d.stream));
    if ((rc = blind_rotate_ext_launch(d, eta, x, set.tables, desc + lut_at, acc, /*all*/ false, B))) return rc;
    if ((rc = ext_extract_ks(d, f, acc, desc + zero_at, lv1, out, B))) return rc;
    return io.finish();
}

static int apply_ext_entry(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, uint32_t eta, const uint32_t *pool, size_t P,
                           const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                           const uint32_t *konst, const uint32_t *lut, uint32_t *out, size_t B, bool dev) {
    if (eta > TFHE_LUT_EXT_MAX_LOG) return fail(c, TFHE_ERR_INVALID, "LUT batch: eta > TFHE_LUT_EXT_MAX_LOG");
    // eta = 0: exactly the existing entry
    if (eta == 0) return apply_entry(c, set, pool, P, term_off, term_src, term_coef, konst, lut, nullptr, out, B, dev);
    if (!c || !set || (B && (!term_off || !konst || !lut || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (const int rc = set_mismatch(c, set, "LUT set")) return rc;
    if (B == 0) return TFHE_OK;
    if (B > 0x7FFFFFFFull || P > 0xFFFFFFFFull) return fail(c, TFHE_ERR_INVALID, "LUT batch: too many nodes or ciphertexts");
    if (term_off[B] && (!term_src || !term_coef || !pool)) return fail(c, TFHE_ERR_INVALID, "null argument");
    // the extended table t is the entries t E .. t E + E - 1: t < floor(T / E)
    if (const char *why = check_lut_nodes(B, P, set->T >> eta, term_off, term_src, lut))
        return fail(c, TFHE_ERR_INVALID, std::string("extended LUT batch: ") + why);
    return on_device0(c, [&](Device &d) {
        return lut_apply_ext_on(d, *set, eta, pool, P, term_off, term_src, term_coef, konst, lut, out, B, dev);
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
    return apply_ext_entry(c, set, eta, pool, P, term_off, term_src, term_coef, konst, lut, out, B, false);
}

int tfhe_gpu_lut_apply_ext_dev(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, uint32_t eta, const uint32_t *pool_dev,
                               size_t P, const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                               const uint32_t *konst, const uint32_t *lut, uint32_t *out_dev, size_t B) {
    return apply_ext_entry(c, set, eta, pool_dev, P, term_off, term_src, term_coef, konst, lut, out_dev, B, true);
}

int tfhe_gpu_bootstrap_lut_each_ext_batch(tfhe_gpu_ctx *c, uint32_t eta, const uint32_t *in, const uint32_t *testvecs,
                                          uint32_t *out, size_t B) {
    return each_ext_entry(c, eta, in, testvecs, out, B, false);
}

int tfhe_gpu_bootstrap_lut_each_ext_dev(tfhe_gpu_ctx *c, uint32_t eta, const uint32_t *in_dev,
                                        const uint32_t *testvecs_dev, uint32_t *out_dev, size_t B) {
    return each_ext_entry(c, eta, in_dev, testvecs_dev, out_dev, B, true);
}

int tfhe_gpu_lut_spread_batch(tfhe_gpu_ctx *c, const uint32_t *in, uint32_t w, uint32_t rot, uint32_t *out, size_t B) {
    return spread_entry(c, in, w, rot, out, B, false);
}

int tfhe_gpu_lut_spread_dev(tfhe_gpu_ctx *c, const uint32_t *in_dev, uint32_t w, uint32_t rot, uint32_t *out_dev, size_t B) {
    return spread_entry(c, in_dev, w, rot, out_dev, B, true);
}

int tfhe_gpu_bootstrap_lut_each_batch(tfhe_gpu_ctx *c, const uint32_t *in, const uint32_t *testvecs, uint32_t *out,
                                      size_t B) {
    return each_entry(c, in, testvecs, out, B, false);
}

int tfhe_gpu_bootstrap_lut_each_dev(tfhe_gpu_ctx *c, const uint32_t *in_dev, const uint32_t *testvecs_dev,
                                    uint32_t *out_dev, size_t B) {
    return each_entry(c, in_dev, testvecs_dev, out_dev, B, true);
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
    return apply_entry(c, set, pool, P, term_off, term_src, term_coef, konst, lut, nullptr, out, B, false);
}

int tfhe_gpu_lut_apply_dev(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const uint32_t *pool_dev, size_t P,
                           const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                           const uint32_t *konst, const uint32_t *lut, uint32_t *out_dev, size_t B) {
    return apply_entry(c, set, pool_dev, P, term_off, term_src, term_coef, konst, lut, nullptr, out_dev, B, true);
}

int tfhe_gpu_lut_apply_multi_batch(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const uint32_t *pool, size_t P,
                                   const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                                   const uint32_t *konst, const uint32_t *lut, const uint32_t *theta, uint32_t *out,
                                   size_t B) {
    return apply_entry(c, set, pool, P, term_off, term_src, term_coef, konst, lut, theta, out, B, false);
}

int tfhe_gpu_lut_apply_multi_dev(tfhe_gpu_ctx *c, const tfhe_gpu_lut_set *set, const uint32_t *pool_dev, size_t P,
                                 const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                                 const uint32_t *konst, const uint32_t *lut, const uint32_t *theta, uint32_t *out_dev,
                                 size_t B) {
    return apply_entry(c, set, pool_dev, P, term_off, term_src, term_coef, konst, lut, theta, out_dev, B, true);
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
    return select_entry(c, pk, m, pool, P, term_off, term_src, term_coef, konst, sel_src, sel_konst, out, B, false);
}

int tfhe_gpu_lut_select_dev(tfhe_gpu_ctx *c, const tfhe_gpu_packing_key *pk, uint32_t m, const uint32_t *pool_dev,
                            size_t P, const uint32_t *term_off, const uint32_t *term_src, const int32_t *term_coef,
                            const uint32_t *konst, const uint32_t *sel_src, const uint32_t *sel_konst, uint32_t *out_dev,
                            size_t B) {
    return select_entry(c, pk, m, pool_dev, P, term_off, term_src, term_coef, konst, sel_src, sel_konst, out_dev, B, true);
}

int tfhe_gpu_lut_select_ext_batch(tfhe_gpu_ctx *c, const tfhe_gpu_packing_key *pk, uint32_t m, uint32_t eta,
                                  const uint32_t *pool, size_t P, const uint32_t *term_off, const uint32_t *term_src,
                                  const int32_t *term_coef, const uint32_t *konst, const uint32_t *sel_src,
                                  const uint32_t *sel_konst, uint32_t *out, size_t B) {
    return select_entry(c, pk, m, pool, P, term_off, term_src, term_coef, konst, sel_src, sel_konst, out, B, false, eta);
}

int tfhe_gpu_lut_select_ext_dev(tfhe_gpu_ctx *c, const tfhe_gpu_packing_key *pk, uint32_t m, uint32_t eta,
                                const uint32_t *pool_dev, size_t P, const uint32_t *term_off, const uint32_t *term_src,
                                const int32_t *term_coef, const uint32_t *konst, const uint32_t *sel_src,
                                const uint32_t *sel_konst, uint32_t *out_dev, size_t B) {
    return select_entry(c, pk, m, pool_dev, P, term_off, term_src, term_coef, konst, sel_src, sel_konst, out_dev, B, true,
                        eta);
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
