// tfhe_leveled.cpp — the leveled half of the C ABI (include/tfhe_gpu.h):
// resident selector sets, CMUX, table lookup by a CMUX tree, rotation by
// encrypted bits and the packed lookup built on both, the packed scatter-add
// (rotation, demultiplexer tree, sum), CMUX graphs, and sample extraction at
// any coefficient (TRLWE / TRGSW encryption is in tfhe_encrypt.cpp).  Host code;
// the arithmetic runs in tfhe_kernels_leveled.hip and the stage kernels of
// tfhe_kernels.hip.  Everything here runs on the context's first device and,
// but for the key switch after an extraction, needs no cloud key.
#include "tfhe_gpu.h"

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "tfhe_ctx.hpp"

using namespace tfhe;

// S TRGSWLv1FFT resident on one device, in the device layout of the
// bootstrapping key's rows (launch_bk_permute).
struct tfhe_gpu_trgsw_set {
    const tfhe_gpu_ctx *ctx = nullptr;  // the context that loaded it (identity only, never dereferenced)
    tfhe_params P{};
    size_t S = 0;
    DevPtr<double> rows;  // S * 2L * 2048 doubles
};

namespace tfhe {

// Bytes of the larger of the table lookup's two ping-pong level buffers (the
// other is half of it): a chunk of queries is as many as keep level 0's outputs,
// 2^(k-1) TRLWELv1 of 8 KB per query, within it.  k = 12: 16 queries per chunk.
constexpr size_t LOOKUP_SCRATCH_CAP = (size_t)256 << 20;
constexpr uint32_t LOOKUP_MAX_K = 12;
constexpr size_t TRLWE_BYTES = 2048 * sizeof(uint32_t);

// The kernels' parameter block with the parameter set's own decomposition
// offset (key.zig:121-131), whether or not a cloud key (which carries one) is loaded.
static KParams leveled_params(const Device &d) {
    KParams K = d.K;
    K.offset = decomposition_offset(d.P);
    return K;
}

// in0 / in1 / out: B TRLWELv1 each, host (dev = false: staged, synchronous) or device.
static int cmux_on(Device &d, const tfhe_gpu_trgsw_set &set, const uint32_t *sel, const uint32_t *in0, const uint32_t *in1,
                   uint32_t *out, size_t B, bool dev) {
    Frame f(d);
    Io io{f, dev};
    DescBlob blob;
    blob.add(sel, B);
    const uint32_t *sel_dev = blob.upload(f);
    io.in(in0, B * TRLWE_BYTES);
    io.in(in1, B * TRLWE_BYTES);
    if (const int rc = io.out(out, B * TRLWE_BYTES)) return rc;
    CmuxBatch b;
    b.sel_rows = set.rows;
    b.sel = sel_dev;
    b.src0 = in0;
    b.src1 = in1;
    b.out = out;
    b.B = B;
    d.last_ks = "";
    HIPCHK(d, launch_cmux(leveled_params(d), tables(d), b, /*shared*/ false, d.stream, &d.last_br));
    return io.finish();
}

// The CMUX tree (vertical packing): level j pairs entries 2i, 2i + 1 of level j - 1
// (level 0: of the table) under address bit j, one launch per level; levels ping-pong
// between two slices (level 0, 2, ... in the larger), the last one writes the outputs.
// Queries go in chunks that keep the larger slice within LOOKUP_SCRATCH_CAP.  The selector and
// gather indices of all levels go up once, in one array:
//   sel[j][q][i] = addr[q k + j]  (i < 2^(k-1-j) pairs of query q at level j), all Q queries;
//   level 0 reads table entries 2i, 2i + 1 (the table is shared by the queries);
//   level j > 0 reads slots 2g, 2g + 1 of the previous level's buffer for its item g.
static int table_lookup_on(Device &d, const tfhe_gpu_trgsw_set &set, const uint32_t *addr, uint32_t k,
                           const uint32_t *table, uint32_t *out, size_t Q, bool dev) {
    const size_t entries = (size_t)1 << k, cnt0 = entries / 2, cnt1 = cnt0 / 2;
    const size_t chunk = std::min(Q, std::max<size_t>(1, LOOKUP_SCRATCH_CAP / (cnt0 * TRLWE_BYTES)));
    std::vector<size_t> sel_at(k);
    size_t words = 0;
    for (uint32_t j = 0; j < k; j++) {
        sel_at[j] = words;
        words += Q * (cnt0 >> j);
    }
    const size_t l0a_at = words, l0b_at = l0a_at + chunk * cnt0, even_at = l0b_at + chunk * cnt0,
                 odd_at = even_at + chunk * cnt1;
    DescBlob blob;
    blob.reserve(odd_at + chunk * cnt1);
    uint32_t *idx = blob.words.data();
    for (uint32_t j = 0; j < k; j++) {
        const size_t cnt = cnt0 >> j;
        uint32_t *s = idx + sel_at[j];
        for (size_t q = 0; q < Q; q++) std::fill(s + q * cnt, s + (q + 1) * cnt, addr[q * k + j]);
    }
    for (size_t g = 0; g < chunk * cnt0; g++) {
        idx[l0a_at + g] = (uint32_t)(2 * (g % cnt0));
        idx[l0b_at + g] = (uint32_t)(2 * (g % cnt0) + 1);
    }
    for (size_t g = 0; g < chunk * cnt1; g++) {
        idx[even_at + g] = (uint32_t)(2 * g);
        idx[odd_at + g] = (uint32_t)(2 * g + 1);
    }
    Frame f(d);
    Io io{f, dev};
    const uint32_t *didx = blob.upload(f);
    uint32_t *even = k > 1 ? f.take<uint32_t>(chunk * cnt0 * 2048) : nullptr;  // levels 0, 2, ...
    uint32_t *odd = k > 2 ? f.take<uint32_t>(chunk * cnt1 * 2048) : nullptr;
    io.in(table, entries * TRLWE_BYTES);
    if (const int rc = io.out(out, Q * TRLWE_BYTES)) return rc;
    const KParams K = leveled_params(d);
    const DevTables T = tables(d);
    d.last_br = d.last_ks = "";
    for (size_t q0 = 0; q0 < Q; q0 += chunk) {
        const size_t nq = std::min(chunk, Q - q0);
        const uint32_t *prev = table;
        for (uint32_t j = 0; j < k; j++) {
            const size_t cnt = cnt0 >> j;
            CmuxBatch b;
            b.sel_rows = set.rows;
            b.sel = didx + sel_at[j] + q0 * cnt;
            b.src0 = b.src1 = prev;
            b.i0 = didx + (j ? even_at : l0a_at);
            b.i1 = didx + (j ? odd_at : l0b_at);
            b.out = j + 1 == k ? out + q0 * 2048 : (j & 1) ? odd : even;
            b.B = nq * cnt;
            // the workgroup form where 4 consecutive items share their selector (>= 4 pairs per
            // query; cnt is a power of two) unless TFHE_OPT_CMUX_FORM = 1 forces the per-wave form:
            // measured faster, 4.8 vs 9.6 ms at Q = 1024, k = 8
            const bool shared = d.opts.cmux_form != 1 && cnt >= CMUX_SHARED_ITEMS;
            const char *name = "";
            HIPCHK(d, launch_cmux(K, T, b, shared, d.stream, &name));
            // last_kernels: the first level's form, then the last level's if it differs
            if (q0 == 0 && j == 0) d.last_br = name;
            else if (q0 == 0 && j + 1 == k && name != d.last_br) d.last_ks = name;
            prev = b.out;
        }
    }
    return io.finish();
}

// h rotate-CMUX steps on B TRLWELv1 (k_rotate_chain), one launch: item g starts from src[i_src[g]]
// (i_src NULL: slot g; a host array of B entries otherwise) and takes selectors sel[g h + j]; all
// device pointers but sel / rot / i_src.  The three go up once, in one array.
static int rotate_launch_on(Device &d, const tfhe_gpu_trgsw_set &set, const uint32_t *sel, const uint32_t *rot, uint32_t h,
                            const uint32_t *src, const uint32_t *i_src, uint32_t *out, size_t B, const char **used) {
    Frame f(d);
    DescBlob blob;
    const size_t sel_at = blob.add(sel, B * h), rot_at = blob.add(rot, h), src_at = blob.add(i_src, i_src ? B : 0);
    const uint32_t *didx = blob.upload(f);
    if (f.rc()) return f.rc();
    RotateBatch b;
    b.sel_rows = set.rows;
    b.sel = didx + sel_at;
    b.rot = didx + rot_at;
    b.h = h;
    b.src = src;
    b.i_src = i_src ? didx + src_at : nullptr;
    b.out = out;
    b.B = B;
    HIPCHK(d, launch_rotate_chain(leveled_params(d), tables(d), b, d.stream, used));
    return TFHE_OK;
}

static int rotate_on(Device &d, const tfhe_gpu_trgsw_set &set, const uint32_t *sel, const uint32_t *rot, uint32_t h,
                     const uint32_t *in, uint32_t *out, size_t B, bool dev) {
    Frame f(d);
    Io io{f, dev};
    int rc = io.in(in, B * TRLWE_BYTES);
    if (!rc) rc = io.out(out, B * TRLWE_BYTES);
    if (rc) return rc;
    d.last_ks = "";
    rc = rotate_launch_on(d, set, sel, rot, h, in, nullptr, out, B, &d.last_br);
    return rc ? rc : io.finish();
}

// The packed lookup (tfhe_packed_lookup_plan): the CMUX tree over the 2^v table TRLWEs under address
// bits h .. k - 1 (table_lookup_on, into a slice of this call's frame), then one k_rotate_chain launch under bits
// 0 .. h - 1.  v = 0: every query's chain starts from table TRLWE 0; h = 0 (an entry fills a TRLWE):
// the tree alone.
static int packed_lookup_on(Device &d, const tfhe_gpu_trgsw_set &set, const uint32_t *addr, uint32_t k,
                            const tfhe_packed_plan &pl, const uint32_t *table, uint32_t *out, size_t Q, bool dev) {
    const uint32_t h = pl.h, v = pl.v;
    Frame f(d);
    Io io{f, dev};
    int rc = io.in(table, (size_t)pl.trlwes * TRLWE_BYTES);
    if (!rc) rc = io.out(out, Q * TRLWE_BYTES);
    uint32_t *tree_out = v && h ? f.take<uint32_t>(Q * 2048) : out;
    if ((rc = f.rc())) return rc;
    d.last_br = d.last_ks = "";
    if (v) {  // the table is on the device by now, staged or the caller's
        std::vector<uint32_t> hi(Q * v);
        for (size_t q = 0; q < Q; q++) std::copy(addr + q * k + h, addr + (q + 1) * k, hi.begin() + q * v);
        rc = table_lookup_on(d, set, hi.data(), v, table, tree_out, Q, /*dev*/ true);
        if (rc) return rc;
    }
    if (h) {
        std::vector<uint32_t> lo(Q * h), first(v ? 0 : Q, 0u);
        for (size_t q = 0; q < Q; q++) std::copy(addr + q * k, addr + q * k + h, lo.begin() + q * h);
        // last_kernels: the tree's first level, then the chain
        rc = rotate_launch_on(d, set, lo.data(), pl.rot, h, v ? tree_out : table,
                              v ? nullptr : first.data(), out, Q, v ? &d.last_ks : &d.last_br);
        if (rc) return rc;
    }
    return io.finish();
}

// The packed scatter-add (include/tfhe_gpu.h): one k_rotate_chain launch over all Q deltas under address bits
// 0 .. h - 1 (rot[j] = stride << j, into a slice of the call's frame), then per chunk of queries the demux tree under bits
// k - 1 .. h, one launch per level, and one k_scatter_reduce that adds the chunk's leaves into the table.  Level l
// (2^l parents per query) writes the larger of two slices when v - 1 - l is even, so the leaves (2^v TRLWELv1 per query) end up
// there and the other holds at most half as much; a chunk is as many queries as keep the leaves within
// TFHE_OPT_SCATTER_SCRATCH_MB.  v = 0: the rotation's outputs (h = 0 as well: the deltas) are the leaves.
// The address bits h .. k - 1 of all queries go up once; a level's parents find their selector in them.
static int packed_scatter_on(Device &d, const tfhe_gpu_trgsw_set &set, const uint32_t *addr, uint32_t k,
                             const tfhe_packed_plan &pl, const uint32_t *delta, uint32_t *table, size_t Q, bool dev) {
    const uint32_t h = pl.h, v = pl.v;
    const size_t leaves = (size_t)1 << v;
    const size_t chunk = std::min(Q, std::max<size_t>(1, ((size_t)d.scatter_scratch_mb << 20) / (leaves * TRLWE_BYTES)));
    Frame f(d);
    Io io{f, dev};
    int rc = io.inout(table, leaves * TRLWE_BYTES);  // the table is this call's output as well
    if (!rc) rc = io.in(delta, Q * TRLWE_BYTES);
    uint32_t *rotated = h ? f.take<uint32_t>(Q * 2048) : nullptr;
    uint32_t *big = v ? f.take<uint32_t>(chunk * leaves * 2048) : nullptr;
    uint32_t *small = v > 1 ? f.take<uint32_t>(chunk * (leaves / 2) * 2048) : nullptr;
    if ((rc = f.rc())) return rc;
    d.last_br = d.last_ks = "";
    if (h) {
        std::vector<uint32_t> lo(Q * h), rot(h);
        for (size_t q = 0; q < Q; q++) std::copy(addr + q * k, addr + q * k + h, lo.begin() + q * h);
        for (uint32_t j = 0; j < h; j++) rot[j] = pl.stride << j;
        rc = rotate_launch_on(d, set, lo.data(), rot.data(), h, delta, nullptr, rotated, Q, &d.last_br);
        if (rc) return rc;
        delta = rotated;
    }
    DescBlob hi;  // address bits h .. k - 1 of every query, uploaded behind the rotation's launch
    hi.reserve(Q * v);
    for (size_t q = 0; q < Q; q++) std::copy(addr + q * k + h, addr + (q + 1) * k, hi.words.begin() + q * v);
    const uint32_t *bits = hi.upload(f);
    if ((rc = f.rc())) return rc;
    const KParams K = leveled_params(d);
    const DevTables T = tables(d);
    for (size_t q0 = 0; q0 < Q; q0 += chunk) {
        const size_t nq = std::min(chunk, Q - q0);
        const uint32_t *prev = delta + q0 * 2048;
        for (uint32_t l = 0; l < v; l++) {
            DemuxBatch b;
            b.sel_rows = set.rows;
            b.sel = bits + q0 * v + (v - 1 - l);
            b.level = l;
            b.sel_stride = v;
            b.src = prev;
            b.out = ((v - 1 - l) & 1) ? small : big;
            b.B = nq << l;
            // the workgroup form where a query has at least 4 parents, as in table_lookup_on
            const bool shared = d.opts.cmux_form != 1 && ((size_t)1 << l) >= CMUX_SHARED_ITEMS;
            const char *name = "";
            HIPCHK(d, launch_demux(K, T, b, shared, d.stream, &name));
            // last_kernels: the chain if there is one, then the first demux level's form
            if (q0 == 0 && l == 0) (h ? d.last_ks : d.last_br) = name;
            prev = b.out;
        }
        HIPCHK(d, launch_scatter_reduce(prev, nq, leaves, table, d.stream));
    }
    return io.finish();
}

// A CMUX graph (include/tfhe_gpu.h "CMUX graphs") by its plan: per chunk of queries one k_cmux_rot launch per
// level over all the chunk's queries, each node writing its slot of the query's n_slots TRLWELv1 of scratch, then
// one copy of the roots (k_graph_roots) into the outputs, or into a slice that sampleExtractIndex(., 0) reads; the
// key switch of extract = 2 runs once, over all Q * R extractions.  A chunk is as many queries as keep the slots
// within LOOKUP_SCRATCH_CAP, and at most TFHE_OPT_GRAPH_CHUNK_QUERIES.  The address bits of all queries, the
// node descriptors in evaluation order (children and outputs as slots), the roots and the extraction's one
// coefficient go up once, in one array.
struct CmuxGraphArgs {
    uint32_t k, nL, V, R;
    const uint32_t *var, *lo, *hi, *rlo, *rhi, *roots;
};
static int cmux_graph_on(Device &d, const tfhe_gpu_trgsw_set &set, const uint32_t *addr, const CmuxGraphArgs &g,
                         const CmuxGraphPlan &pl, const uint32_t *leaves, int extract, uint32_t *out, size_t Q, bool dev) {
    if (extract == 2 && !d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t outs = Q * g.R, wo = extract == 0 ? 2048 : extract == 1 ? (size_t)d.P.N + 1 : tlwe0_words(d.P);
    size_t chunk = pl.n_slots ? std::min(Q, std::max<size_t>(1, LOOKUP_SCRATCH_CAP / (pl.n_slots * TRLWE_BYTES))) : Q;
    if (d.graph_chunk_queries) chunk = std::min(chunk, (size_t)d.graph_chunk_queries);
    const auto ref = [&](uint32_t id) { return id < g.nL ? GRAPH_LEAF_REF | id : pl.slot[id - g.nL]; };
    DescBlob blob;
    const size_t addr_at = blob.add(addr, Q * g.k), nodes_at = blob.reserve((size_t)g.V * 6),
                 roots_at = blob.reserve(g.R), coef_at = blob.reserve(1);  // coefficient 0
    for (uint32_t i = 0; i < g.V; i++) {
        const uint32_t v = pl.order[i];
        const uint32_t nd[6] = {g.var[v], ref(g.lo[v]), ref(g.hi[v]), g.rlo[v], g.rhi[v], pl.slot[v]};
        std::copy(nd, nd + 6, blob.words.begin() + nodes_at + (size_t)i * 6);
    }
    for (uint32_t r = 0; r < g.R; r++) blob.words[roots_at + r] = ref(g.roots[r]);
    Frame f(d);
    Io io{f, dev};
    const uint32_t *didx = blob.upload(f);
    io.in(leaves, (size_t)g.nL * TRLWE_BYTES);
    int rc = io.out(out, outs * wo * 4);
    uint32_t *slots = pl.n_slots ? f.take<uint32_t>(chunk * pl.n_slots * 2048) : nullptr;
    uint32_t *picked = extract ? f.take<uint32_t>(chunk * g.R * 2048) : nullptr;  // a chunk's roots before extraction
    uint32_t *lv1 = extract == 2 ? f.ks_input<uint32_t>(outs * 1025) : out;
    if ((rc = f.rc())) return rc;
    const KParams K = leveled_params(d);
    const DevTables T = tables(d);
    d.last_br = g.V ? "" : "k_graph_roots";
    d.last_ks = "";
    for (size_t q0 = 0; q0 < Q; q0 += chunk) {
        const size_t nq = std::min(chunk, Q - q0);
        for (uint32_t l = 1; l <= pl.depth; l++) {
            GraphLevel b;
            b.sel_rows = set.rows;
            b.addr = didx + addr_at + q0 * g.k;
            b.k = g.k;
            b.nodes = didx + nodes_at + (size_t)pl.first[l - 1] * 6;
            b.cnt = pl.first[l] - pl.first[l - 1];
            b.leaves = leaves;
            b.slots = slots;
            b.n_slots = pl.n_slots;
            b.nq = nq;
            HIPCHK(d, launch_cmux_graph_level(K, T, b, d.stream, &d.last_br));
        }
        uint32_t *to = extract ? picked : out + q0 * g.R * 2048;
        HIPCHK(d, launch_cmux_graph_roots(didx + roots_at, g.R, leaves, slots, pl.n_slots, to, nq, d.stream));
        if (extract)
            HIPCHK(d, launch_sample_extract(picked, didx + coef_at, 1, lv1 + q0 * g.R * 1025, nq * g.R, d.stream));
    }
    if (extract == 2) {
        KsGemm G;
        if ((rc = ks_gemm_args(f, outs, G))) return rc;
        HIPCHK(d, launch_key_switch(d.K, lv1, d.d_ksk, out, outs, d.stream, d.opts, &d.last_ks, &G));
    }
    return io.finish();
}

static int sample_extract_on(Device &d, const uint32_t *trlwe, const uint32_t *coef, size_t C, bool key_switch,
                             uint32_t *out, size_t B, bool dev) {
    if (key_switch && !d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t items = B * C, wo = key_switch ? tlwe0_words(d.P) : (size_t)d.P.N + 1;
    if (items == 0) return TFHE_OK;
    Frame f(d);
    Io io{f, dev};
    DescBlob blob;
    blob.add(coef, C);
    const uint32_t *coef_dev = blob.upload(f);
    io.in(trlwe, B * TRLWE_BYTES);
    int rc = io.out(out, items * wo * 4);
    uint32_t *lv1 = key_switch ? f.ks_input<uint32_t>(items * 1025) : out;
    if ((rc = f.rc())) return rc;
    HIPCHK(d, launch_sample_extract(trlwe, coef_dev, C, lv1, B, d.stream));
    if (key_switch) {
        KsGemm G;
        if ((rc = ks_gemm_args(f, items, G))) return rc;
        HIPCHK(d, launch_key_switch(d.K, lv1, d.d_ksk, out, items, d.stream, d.opts, &d.last_ks, &G));
    }
    return io.finish();
}

}  // namespace tfhe

extern "C" {

int tfhe_gpu_trgsw_set_load(tfhe_gpu_ctx *c, const double *trgsw_fft, size_t S, tfhe_gpu_trgsw_set **out) {
    if (out) *out = nullptr;
    if (!c || !trgsw_fft || !out || S == 0 || S > 0xFFFFFFFFull) return fail(c, TFHE_ERR_INVALID, "null argument or empty set");
    std::unique_ptr<tfhe_gpu_trgsw_set> set(new tfhe_gpu_trgsw_set);
    set->ctx = c;
    set->P = c->P;
    set->S = S;
    const int rc = on_device0(c, [&](Device &d) -> int {
        const size_t rows = S * 2 * d.P.L, bytes = rows * 2048 * sizeof(double);
        Frame f(d);
        const double *staged = f.h2d(trgsw_fft, bytes);
        if (f.rc()) return f.rc();
        if (hipMalloc((void **)set->rows.make(d.device), bytes) != hipSuccess)
            return fail(d, TFHE_ERR_OOM, "hipMalloc(selector set)");
        HIPCHK(d, launch_bk_permute(d.K, staged, set->rows, rows, d.stream));
        HIPCHK(d, hipStreamSynchronize(d.stream));
        return TFHE_OK;
    });
    if (rc) return rc;
    *out = set.release();
    return TFHE_OK;
}

void tfhe_gpu_trgsw_set_destroy(tfhe_gpu_trgsw_set *set) { delete set; }

static int cmux_entry(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *sel, const uint32_t *in0,
                      const uint32_t *in1, uint32_t *out, size_t B, bool dev) {
    if (!c || !set || (B && (!sel || !in0 || !in1 || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (const int rc = set_mismatch(c, set, "selector set")) return rc;
    for (size_t i = 0; i < B; i++)
        if (sel[i] >= set->S) return fail(c, TFHE_ERR_INVALID, "selector index >= the set's size");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) { return cmux_on(d, *set, sel, in0, in1, out, B, dev); });
}

int tfhe_gpu_cmux_batch(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *sel, const uint32_t *in0,
                        const uint32_t *in1, uint32_t *out, size_t B) {
    return cmux_entry(c, set, sel, in0, in1, out, B, false);
}

int tfhe_gpu_cmux_batch_dev(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *sel, const uint32_t *in0_dev,
                            const uint32_t *in1_dev, uint32_t *out_dev, size_t B) {
    return cmux_entry(c, set, sel, in0_dev, in1_dev, out_dev, B, true);
}

static int lookup_entry(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k,
                        const uint32_t *table, uint32_t *out, size_t Q, bool dev) {
    if (!c || !set || !table || (Q && (!addr || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (k < 1 || k > LOOKUP_MAX_K) return fail(c, TFHE_ERR_INVALID, "table lookup: k outside 1..12");
    if (const int rc = set_mismatch(c, set, "selector set")) return rc;
    if (Q > 0xFFFFFFFFull >> k) return fail(c, TFHE_ERR_INVALID, "table lookup: too many queries");
    for (size_t i = 0; i < Q * k; i++)
        if (addr[i] >= set->S) return fail(c, TFHE_ERR_INVALID, "address selector index >= the set's size");
    if (Q == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) { return table_lookup_on(d, *set, addr, k, table, out, Q, dev); });
}

int tfhe_gpu_table_lookup_batch(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k,
                                const uint32_t *table, uint32_t *out_trlwe, size_t Q) {
    return lookup_entry(c, set, addr, k, table, out_trlwe, Q, false);
}

int tfhe_gpu_table_lookup_dev(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k,
                              const uint32_t *table_dev, uint32_t *out_dev, size_t Q) {
    return lookup_entry(c, set, addr, k, table_dev, out_dev, Q, true);
}

static int rotate_entry(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *sel, const uint32_t *rot, uint32_t h,
                        const uint32_t *in, uint32_t *out, size_t B, bool dev) {
    if (!c || !set || !rot || (B && (!sel || !in || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (h < 1 || h > TFHE_ROTATE_MAX_STEPS) return fail(c, TFHE_ERR_INVALID, "rotate by bits: h outside 1..32");
    for (uint32_t j = 0; j < h; j++)
        if (rot[j] > 2 * c->P.N) return fail(c, TFHE_ERR_INVALID, "rotate by bits: exponent > 2N");
    if (const int rc = set_mismatch(c, set, "selector set")) return rc;
    if (B > 0xFFFFFFFFull / h) return fail(c, TFHE_ERR_INVALID, "rotate by bits: too many items");
    for (size_t i = 0; i < B * h; i++)
        if (sel[i] >= set->S) return fail(c, TFHE_ERR_INVALID, "selector index >= the set's size");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) { return rotate_on(d, *set, sel, rot, h, in, out, B, dev); });
}

int tfhe_gpu_rotate_by_bits_batch(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *sel, const uint32_t *rot,
                                  uint32_t h, const uint32_t *in, uint32_t *out, size_t B) {
    return rotate_entry(c, set, sel, rot, h, in, out, B, false);
}

int tfhe_gpu_rotate_by_bits_dev(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *sel, const uint32_t *rot,
                                uint32_t h, const uint32_t *in_dev, uint32_t *out_dev, size_t B) {
    return rotate_entry(c, set, sel, rot, h, in_dev, out_dev, B, true);
}

static int packed_entry(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k, uint32_t width,
                        const uint32_t *table, uint32_t *out, size_t Q, bool dev) {
    if (!c || !set || !table || (Q && (!addr || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    tfhe_packed_plan pl;
    if (tfhe_packed_lookup_plan(&c->P, k, width, &pl) != TFHE_OK)
        return fail(c, TFHE_ERR_INVALID, "packed lookup: width outside 1..N, k = 0, or more than 12 address bits left to the tree");
    if (const int rc = set_mismatch(c, set, "selector set")) return rc;
    if (Q > 0xFFFFFFFFull >> pl.v) return fail(c, TFHE_ERR_INVALID, "packed lookup: too many queries");
    for (size_t i = 0; i < Q * k; i++)
        if (addr[i] >= set->S) return fail(c, TFHE_ERR_INVALID, "address selector index >= the set's size");
    if (Q == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) { return packed_lookup_on(d, *set, addr, k, pl, table, out, Q, dev); });
}

int tfhe_gpu_packed_lookup_batch(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k,
                                 uint32_t width, const uint32_t *table, uint32_t *out_trlwe, size_t Q) {
    return packed_entry(c, set, addr, k, width, table, out_trlwe, Q, false);
}

int tfhe_gpu_packed_lookup_dev(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k,
                               uint32_t width, const uint32_t *table_dev, uint32_t *out_dev, size_t Q) {
    return packed_entry(c, set, addr, k, width, table_dev, out_dev, Q, true);
}

static int scatter_entry(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k, uint32_t width,
                         const uint32_t *delta, uint32_t *table, size_t Q, bool dev) {
    if (!c || !set || !table || (Q && (!addr || !delta))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    tfhe_packed_plan pl;
    if (tfhe_packed_lookup_plan(&c->P, k, width, &pl) != TFHE_OK)
        return fail(c, TFHE_ERR_INVALID, "packed scatter-add: width outside 1..N, k = 0, or more than 12 address bits left to the tree");
    if (const int rc = set_mismatch(c, set, "selector set")) return rc;
    if (Q > 0xFFFFFFFFull >> pl.v || Q > 0xFFFFFFFFull / k) return fail(c, TFHE_ERR_INVALID, "packed scatter-add: too many queries");
    for (size_t i = 0; i < Q * k; i++)
        if (addr[i] >= set->S) return fail(c, TFHE_ERR_INVALID, "address selector index >= the set's size");
    if (Q == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) { return packed_scatter_on(d, *set, addr, k, pl, delta, table, Q, dev); });
}

int tfhe_gpu_packed_scatter_add_batch(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k,
                                      uint32_t width, const uint32_t *delta, uint32_t *table, size_t Q) {
    return scatter_entry(c, set, addr, k, width, delta, table, Q, false);
}

int tfhe_gpu_packed_scatter_add_dev(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k,
                                    uint32_t width, const uint32_t *delta_dev, uint32_t *table_dev, size_t Q) {
    return scatter_entry(c, set, addr, k, width, delta_dev, table_dev, Q, true);
}

static int graph_entry(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, const CmuxGraphArgs &g,
                       const uint32_t *leaves, int extract, uint32_t *out, size_t Q, bool dev) {
    if (!c || !set || !leaves || (Q && ((g.k && !addr) || (g.R && !out)))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (extract < 0 || extract > 2) return fail(c, TFHE_ERR_INVALID, "CMUX graph: extract outside 0..2");
    CmuxGraphPlan pl;
    if (const char *why = plan_cmux_graph(g.nL, g.V, g.k, g.var, g.lo, g.hi, g.rlo, g.rhi, g.R, g.roots, c->P.N, pl))
        return fail(c, TFHE_ERR_INVALID, why);
    if (const int rc = set_mismatch(c, set, "selector set")) return rc;
    const size_t widest = std::max<size_t>({(size_t)g.k, (size_t)g.V, (size_t)g.R, 1});
    if (Q > 0xFFFFFFFFull / widest) return fail(c, TFHE_ERR_INVALID, "CMUX graph: too many queries");
    for (size_t i = 0; i < Q * g.k; i++)
        if (addr[i] >= set->S) return fail(c, TFHE_ERR_INVALID, "address selector index >= the set's size");
    if (dev && Q && g.R) {
        const size_t wo = extract == 0 ? 2048 : extract == 1 ? (size_t)c->P.N + 1 : tlwe0_words(c->P);
        const uint32_t *le = leaves + (size_t)g.nL * 2048, *oe = out + Q * g.R * wo;
        if (out < le && leaves < oe) return fail(c, TFHE_ERR_INVALID, "CMUX graph: out overlaps leaves");
    }
    if (Q == 0 || g.R == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) { return cmux_graph_on(d, *set, addr, g, pl, leaves, extract, out, Q, dev); });
}

int tfhe_gpu_cmux_graph_batch(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k,
                              const uint32_t *leaves, uint32_t nL, uint32_t V, const uint32_t *var, const uint32_t *lo,
                              const uint32_t *hi, const uint32_t *rlo, const uint32_t *rhi, uint32_t R,
                              const uint32_t *roots, int extract, uint32_t *out, size_t Q) {
    return graph_entry(c, set, addr, CmuxGraphArgs{k, nL, V, R, var, lo, hi, rlo, rhi, roots}, leaves, extract, out, Q, false);
}

int tfhe_gpu_cmux_graph_dev(tfhe_gpu_ctx *c, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k,
                            const uint32_t *leaves_dev, uint32_t nL, uint32_t V, const uint32_t *var, const uint32_t *lo,
                            const uint32_t *hi, const uint32_t *rlo, const uint32_t *rhi, uint32_t R,
                            const uint32_t *roots, int extract, uint32_t *out_dev, size_t Q) {
    return graph_entry(c, set, addr, CmuxGraphArgs{k, nL, V, R, var, lo, hi, rlo, rhi, roots}, leaves_dev, extract, out_dev, Q,
                       true);
}

static int extract_entry(tfhe_gpu_ctx *c, const uint32_t *trlwe, const uint32_t *coef, size_t C, int key_switch,
                         uint32_t *out, size_t B, bool dev) {
    if (!c || (C && !coef) || (B && C && (!trlwe || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    for (size_t i = 0; i < C; i++)
        if (coef[i] >= c->P.N) return fail(c, TFHE_ERR_INVALID, "coefficient index >= N");
    if (B * C > 0xFFFFFFFFull) return fail(c, TFHE_ERR_INVALID, "sample extract: too many outputs");
    return on_device0(c, [&](Device &d) { return sample_extract_on(d, trlwe, coef, C, key_switch != 0, out, B, dev); });
}

int tfhe_gpu_sample_extract_batch(tfhe_gpu_ctx *c, const uint32_t *trlwe, const uint32_t *coef, size_t C, int key_switch,
                                  uint32_t *out, size_t B) {
    return extract_entry(c, trlwe, coef, C, key_switch, out, B, false);
}

int tfhe_gpu_sample_extract_dev(tfhe_gpu_ctx *c, const uint32_t *trlwe_dev, const uint32_t *coef, size_t C, int key_switch,
                                uint32_t *out_dev, size_t B) {
    return extract_entry(c, trlwe_dev, coef, C, key_switch, out_dev, B, true);
}

}  // extern "C"
