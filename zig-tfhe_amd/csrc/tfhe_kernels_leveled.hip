// tfhe_kernels_leveled.hip — the leveled half of zig-tfhe on the device: CMUX
// against caller-supplied TRGSW selectors (trgsw.zig:260-284), the rotation by
// encrypted bits built from it (k_rotate_chain), the CMUX graph's level
// (k_cmux_rot) and sampleExtractIndex at any
// coefficient (trlwe.zig:146-162).  Its own unit: the
// bootstrap kernels' objects (tfhe_kernels.o, tfhe_kernels_whole.o), which
// tfhe_gpu_build_id() hashes, do not change with it.  Same flags as theirs
// (-ffp-contract=off: every f64 multiply and add rounds separately).
//
// Arithmetic: the reference's expression trees (FU = false, SMALL = false)
// whatever TFHE_OPT_ARITH says.  A caller's selector is not a keygen'd BK row,
// so the fused arithmetic's admission regime says nothing
// about it; the near-tie counter and flags are not touched.
#include "tfhe_device.hpp"

namespace tfhe {

// Waves (items) per workgroup of k_cmux.  Each wave exchanges its transforms
// through a private 16 KB LDS buffer (wave_sync only, no workgroup barrier).
// Registers, not LDS, set the occupancy (make resource-usage): at L = 3 the
// kernel takes 256 VGPRs + 68 AGPRs without scratch, i.e. one wave per SIMD,
// and capping it at 256 registers for two (__launch_bounds__(256, 2)) spills
// 272 bytes per lane.  So one workgroup of 4 waves fills a CU (64 KB of its
// 160 KB LDS); a wider workgroup could not be resident and would idle more
// waves in a ragged tail.
constexpr int CMUX_WAVES = 4;

// out[g] = ExtProd(sel_rows[sel[g]], in1 - in0) + in0 with in0 = src0[i0[g]],
// in1 = src1[i1[g]] (i0 / i1 NULL: g itself), one wavefront per item; lane t
// owns coefficients t + 64m as in k_external_product.  tmp = in1 - in0 + offset
// stays in registers, and the accumulators start from in0, so inverse_and_add's
// `acc += ExtProd` is the CMUX add (tmp2 + in1 of trgsw.zig:277-281; wrapping
// u32 adds commute).  Waves past B (the last workgroup's tail) return before
// they read or write anything; nothing below is a workgroup barrier.
template <int L>
__global__ __launch_bounds__(64 * CMUX_WAVES) void k_cmux(KParams P, DevTables TT,
                                                          const double2 *__restrict__ sel_rows,
                                                          const uint32_t *__restrict__ sel,
                                                          const uint32_t *__restrict__ src0,
                                                          const uint32_t *__restrict__ i0,
                                                          const uint32_t *__restrict__ src1,
                                                          const uint32_t *__restrict__ i1, uint32_t *__restrict__ out,
                                                          size_t B) {
    __shared__ C2 s_x[CMUX_WAVES][2 * 512];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), t = threadIdx.x & 63;
    const size_t g = (size_t)blockIdx.x * CMUX_WAVES + w;
    if (g >= B) return;
    const uint32_t *x0 = src0 + (size_t)(i0 ? i0[g] : g) * 2048;
    const uint32_t *x1 = src1 + (size_t)(i1 ? i1[g] : g) * 2048;
    const double2 *row = sel_rows + (size_t)sel[g] * (2 * L * 1024);
    RegTw T;
    T.init(TT.tw, t);
    C2 twl[8];
#pragma unroll
    for (int m = 0; m < 8; m++) twl[m] = TT.twist[t + 64 * m];
    uint32_t tA[16], tB[16], accA[16], accB[16];
#pragma unroll
    for (int m = 0; m < 16; m++) {
        accA[m] = x0[t + 64 * m];
        accB[m] = x0[1024 + t + 64 * m];
        tA[m] = x1[t + 64 * m] - accA[m] + P.offset;
        tB[m] = x1[1024 + t + 64 * m] - accB[m] + P.offset;
    }
    C2 fa[8], fb[8];
    ext_pairs_global<L>(tA, tB, row, P.bgbit, T, twl, s_x[w], t, fa, fb);
    uint32_t near = NEAR_NONE;
    inverse_and_add<false, 1>(fa, fb, s_x[w], T, twl, t, accA, accB, near);
    uint32_t *o = out + g * 2048;
#pragma unroll
    for (int m = 0; m < 16; m++) {
        o[t + 64 * m] = accA[m];
        o[1024 + t + 64 * m] = accB[m];
    }
}

// One level of a CMUX graph (include/tfhe_gpu.h "CMUX graphs"): k_cmux with its two inputs
// gathered per item and multiplied by a power of X as they are read.  Item g is node
// i = g % cnt of the level for query q = g / cnt of the chunk; the node's six words
// nd[i] = {var, lo, hi, rlo, rhi, slot} are shared by the queries.  lo / hi name a leaf of the
// shared leaves array (GRAPH_LEAF | index) or a slot of the query's own scratch
// slots[q * n_slots ..], the selector is addr[q * k + var], and the output goes to the query's
// slot nd.slot.  tA / tB = X^rhi in1 - X^rlo in0 + offset and the accumulators X^rlo in0 come
// straight from global memory through rot_read (polyMulWithXK, trgsw.zig:442-466: index and sign
// only, so a wave still reads 64 consecutive words mod N); everything after that is k_cmux, and
// with rlo = rhi = 0 so are the words.  All of the item's descriptors are wave-uniform.  A slot
// written in this launch is read by no item of it (tfhe_cmux_graph_plan), so reads and writes
// need no order.  Waves past B return before they read or write anything; no workgroup barrier.
constexpr uint32_t GRAPH_LEAF = GRAPH_LEAF_REF;  // tfhe_internal.hpp
constexpr int GRAPH_NODE_WORDS = 6;
template <int L>
__global__ __launch_bounds__(64 * CMUX_WAVES) void k_cmux_rot(KParams P, DevTables TT,
                                                              const double2 *__restrict__ sel_rows,
                                                              const uint32_t *__restrict__ addr, uint32_t k,
                                                              const uint32_t *__restrict__ nd, uint32_t cnt,
                                                              const uint32_t *leaves, uint32_t *slots,
                                                              uint32_t n_slots, uint32_t B) {
    __shared__ C2 s_x[CMUX_WAVES][2 * 512];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), t = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * CMUX_WAVES + w;
    if (g >= B) return;
    const uint32_t q = g / cnt;
    const uint32_t *me = nd + (size_t)(g - q * cnt) * GRAPH_NODE_WORDS;
    const uint32_t lo = me[1], hi = me[2];
    const int r0 = (int)me[3], r1 = (int)me[4];
    uint32_t *mine = slots + (size_t)q * n_slots * 2048;
    const uint32_t *x0 = (lo & GRAPH_LEAF) ? leaves + (size_t)(lo & ~GRAPH_LEAF) * 2048 : mine + (size_t)lo * 2048;
    const uint32_t *x1 = (hi & GRAPH_LEAF) ? leaves + (size_t)(hi & ~GRAPH_LEAF) * 2048 : mine + (size_t)hi * 2048;
    const double2 *row = sel_rows + (size_t)addr[(size_t)q * k + me[0]] * (2 * L * 1024);
    uint32_t *o = mine + (size_t)me[5] * 2048;
    RegTw T;
    T.init(TT.tw, t);
    C2 twl[8];
#pragma unroll
    for (int m = 0; m < 8; m++) twl[m] = TT.twist[t + 64 * m];
    uint32_t tA[16], tB[16], accA[16], accB[16];
#pragma unroll
    for (int m = 0; m < 16; m++) {
        accA[m] = rot_read(x0, t + 64 * m, r0);
        accB[m] = rot_read(x0 + 1024, t + 64 * m, r0);
        tA[m] = rot_read(x1, t + 64 * m, r1) - accA[m] + P.offset;
        tB[m] = rot_read(x1 + 1024, t + 64 * m, r1) - accB[m] + P.offset;
    }
    C2 fa[8], fb[8];
    ext_pairs_global<L>(tA, tB, row, P.bgbit, T, twl, s_x[w], t, fa, fb);
    uint32_t near = NEAR_NONE;
    inverse_and_add<false, 1>(fa, fb, s_x[w], T, twl, t, accA, accB, near);
#pragma unroll
    for (int m = 0; m < 16; m++) {
        o[t + 64 * m] = accA[m];
        o[1024 + t + 64 * m] = accB[m];
    }
}

// out[g] = the value `roots[g % R]` names (a leaf, or a slot of query g / R of the chunk) for the
// nq * R outputs of a chunk: a copy of 2N words, one block each.
__global__ __launch_bounds__(256) void k_graph_roots(const uint32_t *__restrict__ roots, uint32_t R,
                                                     const uint32_t *__restrict__ leaves,
                                                     const uint32_t *__restrict__ slots, uint32_t n_slots,
                                                     uint32_t *__restrict__ out) {
    const uint32_t q = blockIdx.x / R, r = roots[blockIdx.x % R];
    const uint32_t *x = (r & GRAPH_LEAF) ? leaves + (size_t)(r & ~GRAPH_LEAF) * 2048
                                         : slots + ((size_t)q * n_slots + r) * 2048;
    uint32_t *o = out + (size_t)blockIdx.x * 2048;
    for (uint32_t i = threadIdx.x; i < 2048; i += 256) o[i] = x[i];
}

// Workgroup form for items that share their selector: the 4 waves' items
// g0 .. g0 + 3 (g0 = 4 * blockIdx.x) all use selector sel[g0] (the launcher's
// contract: the tree levels with at least 4 pairs per query).  The per-wave form
// reads each item's 2L rows (96 KB at L = 3) from L2, about four times the
// item's ciphertext traffic (3 x 8 KB); here the 256 threads stage every row
// pair (32 KB) in LDS once and all four waves run the LDS MAC of the blind
// rotation (mac_pair_lds) on it.  No DMA and no slot counters: each thread reads
// its 8 x 16 B of a pair into registers, runs the pair's forward transforms,
// meets a workgroup barrier (all waves are through the previous pair's MAC),
// stores its piece into LDS, and a second barrier opens the MAC.  fmaInFd1024 accumulates from 0.0 here as in
// the blind rotation (0.0 + x == x).  There is no ragged tail: launch_cmux
// refuses a B that is not a multiple of 4 (a wave that left early would miss
// the barriers; one kept in by a flag until a late return made hipcc spill
// 2.6 KB per lane at L = 3).
constexpr int CS_LDS_BK = 2048 * 16;
template <int L, int RP = 0>
DEV void ext_pairs_shared(const uint32_t *tA, const uint32_t *tB, const double2 *__restrict__ row,
                          int bgbit, const RegTw &T, const C2 *twl, C2 *xb, int t, int tid, double2 *s_bk, C2 *fa,
                          C2 *fb) {
    if constexpr (RP < L) {
        // This thread's 8 x 16 B of the pair, read before the forward transforms so that they hide
        // the L2 latency (4.81 against 6.88 ms per 1,024 lookups without, profiles/
        // lookup_ab_shared_prefetch.txt).  The address goes through an opaque asm: hipcc otherwise
        // hoists all L pairs' loads to the top of the kernel and spills.  Plain doubles: an array
        // of double2 is not split into registers here but promoted to LDS, 64 KB of it.
        const double2 *src = row + (size_t)RP * 2048 + tid;
        asm volatile("" : "+v"(src)::"memory");
        double prx[8], pry[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double2 v = src[256 * k];
            prx[k] = v.x;
            pry[k] = v.y;
        }
        C2 d[2][8];
        forward_pair<L, RP, 1>(tA, tB, bgbit, T, twl, xb, t, d);
        if (RP > 0) __syncthreads();  // every wave is through the previous pair's MAC
#pragma unroll
        for (int k = 0; k < 8; k++) s_bk[256 * k + tid] = make_double2(prx[k], pry[k]);
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        mac_pair_lds<false>(fa, fb, d[0], d[1], s_bk, t);
        __builtin_amdgcn_sched_barrier(0);
        ext_pairs_shared<L, RP + 1>(tA, tB, row, bgbit, T, twl, xb, t, tid, s_bk, fa, fb);
    }
}

template <int L>
__global__ __launch_bounds__(64 * CMUX_WAVES) void k_cmux_shared(KParams P, DevTables TT,
                                                                 const double2 *__restrict__ sel_rows,
                                                                 const uint32_t *__restrict__ sel,
                                                                 const uint32_t *__restrict__ src0,
                                                                 const uint32_t *__restrict__ i0,
                                                                 const uint32_t *__restrict__ src1,
                                                                 const uint32_t *__restrict__ i1,
                                                                 uint32_t *__restrict__ out, size_t B) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[CS_LDS_BK + CMUX_WAVES * 2 * 512 * 16];
    double2 *s_bk = reinterpret_cast<double2 *>(smem);
    const int tid = threadIdx.x, t = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    C2 *s_x = reinterpret_cast<C2 *>(smem + CS_LDS_BK) + w * 2 * 512;
    const size_t g0 = (size_t)blockIdx.x * CMUX_WAVES, g = g0 + w;  // g < B: B is a multiple of 4 (launch_cmux)
    const double2 *row = sel_rows + (size_t)sel[g0] * (2 * L * 1024);
    RegTw T;
    T.init(TT.tw, t);
    C2 twl[8];
#pragma unroll
    for (int m = 0; m < 8; m++) twl[m] = TT.twist[t + 64 * m];
    const uint32_t *x0 = src0 + (size_t)(i0 ? i0[g] : g) * 2048;
    const uint32_t *x1 = src1 + (size_t)(i1 ? i1[g] : g) * 2048;
    uint32_t tA[16], tB[16], accA[16], accB[16];
#pragma unroll
    for (int m = 0; m < 16; m++) {
        accA[m] = x0[t + 64 * m];
        accB[m] = x0[1024 + t + 64 * m];
        tA[m] = x1[t + 64 * m] - accA[m] + P.offset;
        tB[m] = x1[1024 + t + 64 * m] - accB[m] + P.offset;
    }
    C2 fa[8], fb[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        fa[q] = c2(0.0, 0.0);
        fb[q] = c2(0.0, 0.0);
    }
    ext_pairs_shared<L>(tA, tB, row, P.bgbit, T, twl, s_x, t, tid, s_bk, fa, fb);
    uint32_t near = NEAR_NONE;
    inverse_and_add<false, 1>(fa, fb, s_x, T, twl, t, accA, accB, near);
    uint32_t *o = out + g * 2048;
#pragma unroll
    for (int m = 0; m < 16; m++) {
        o[t + 64 * m] = accA[m];
        o[1024 + t + 64 * m] = accB[m];
    }
}

// Rotation by encrypted bits (horizontal packing): h CMUX steps on one TRLWE,
//   acc <- cmux(acc, X^rot[j] acc, selector sel[g h + j]),  j = 0 .. h - 1
// (trgsw.zig:260-284 on polyMulWithXK, :442-466), one wavefront per item for the
// whole chain.  The accumulator lives in a wave-private 8 KB of LDS beside the
// wave's 16 KB transform exchange (96 KB per workgroup): a step reads
// tmp = X^rot acc - acc + offset out of it (rot_read, as the blind rotation
// does), runs the external product on the item's own selector rows, reloads acc
// into the accumulator registers only for inverse_and_add and stores the sum
// back, so no ciphertext goes to HBM between steps and in0 is not held in 32
// registers across the transforms.  The LDS executes one wave's DS instructions
// in issue order, so a wavefront fence between the store and the next step's
// rotated reads (other lanes' words) is the whole synchronisation.  rot[] and h
// are wave-uniform; rot[j] in [0, 2N] (rot_read masks the index: no value of it
// reads outside the accumulator).  acc_0 = src[i_src[g]] (i_src NULL: g).  Waves
// past B return before they read or write anything; no workgroup barrier.
// The pairs go through ext_pairs_chain (tfhe_device.hpp): ext_pairs_global with each pair's sums completed
// at the pair, which keeps the loop free of scratch.
template <int L>
__global__ __launch_bounds__(64 * CMUX_WAVES) void k_rotate_chain(KParams P, DevTables TT,
                                                                  const double2 *__restrict__ sel_rows,
                                                                  const uint32_t *__restrict__ sel,
                                                                  const uint32_t *__restrict__ rot, uint32_t h,
                                                                  const uint32_t *__restrict__ src,
                                                                  const uint32_t *__restrict__ i_src,
                                                                  uint32_t *__restrict__ out, size_t B) {
    __shared__ C2 s_x[CMUX_WAVES][2 * 512];
    __shared__ uint32_t s_acc[CMUX_WAVES][2048];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const size_t g = (size_t)blockIdx.x * CMUX_WAVES + w;
    if (g >= B) return;
    const uint32_t *x = src + (size_t)(i_src ? i_src[g] : g) * 2048;
    const uint32_t *s = sel + g * h;
    uint32_t *acc = s_acc[w];
#pragma unroll
    for (int m = 0; m < 16; m++) {
        acc[lane + 64 * m] = x[lane + 64 * m];
        acc[1024 + lane + 64 * m] = x[1024 + lane + 64 * m];
    }
    wave_sync();
    uint32_t accA[16], accB[16];
    for (uint32_t j = 0; j < h; j++) {
        // The lane index goes through an opaque asm in every step: everything a step derives
        // from it (the exchanges' swizzled LDS addresses, the twiddle and twist reads, the
        // accumulator's addresses) is then computed in the step.  Hoisted out of the loop, as
        // hipcc does otherwise, some 60 such values stay live across all of it and are spilled
        // in the loop's preheader.
        int t = lane;
        asm volatile("" : "+v"(t));
        const int r = __builtin_amdgcn_readfirstlane((int)rot[j]);
        const double2 *row = sel_rows + (size_t)s[j] * (2 * L * 1024);
        RegTw T;
        T.init(TT.tw, t);
        C2 twl[8];
#pragma unroll
        for (int m = 0; m < 8; m++) twl[m] = TT.twist[t + 64 * m];
        uint32_t tA[16], tB[16];
#pragma unroll
        for (int m = 0; m < 16; m++) {
            tA[m] = rot_read(acc, t + 64 * m, r) - acc[t + 64 * m] + P.offset;
            tB[m] = rot_read(acc + 1024, t + 64 * m, r) - acc[1024 + t + 64 * m] + P.offset;
        }
        C2 fa[8], fb[8];
        ext_pairs_chain<L>(tA, tB, row, P.bgbit, T, twl, s_x[w], t, fa, fb);
        // acc_j again, from LDS: not held in 32 registers across the transforms
        int tr = lane;
        asm volatile("" : "+v"(tr));
#pragma unroll
        for (int m = 0; m < 16; m++) {
            accA[m] = acc[tr + 64 * m];
            accB[m] = acc[1024 + tr + 64 * m];
        }
        uint32_t near = NEAR_NONE;
        inverse_and_add<false, 1>(fa, fb, s_x[w], T, twl, t, accA, accB, near);
        if (j + 1 < h) {
            wave_sync();  // this step's reads of acc precede the stores
#pragma unroll
            for (int m = 0; m < 16; m++) {
                acc[tr + 64 * m] = accA[m];
                acc[1024 + tr + 64 * m] = accB[m];
            }
            wave_sync();  // the stores precede the next step's rotated reads (other lanes' words)
        }
    }
    uint32_t *o = out + g * 2048;
#pragma unroll
    for (int m = 0; m < 16; m++) {
        o[lane + 64 * m] = accA[m];
        o[1024 + lane + 64 * m] = accB[m];
    }
}

// One level of the demultiplexer tree (the packed scatter-add), the mirror of a
// CMUX level: parent g with value x = src[g] has the children
//   out[2g + 1] = hi = ExtProd(selector, x)   (externalProductWithFft, trgsw.zig:111-154)
//   out[2g]     = lo = x - hi                 (wrapping u32 on all 2N words)
// so x goes on to the child the selector names and noise to the other.  One wavefront per parent
// in k_cmux's lane layout; tmp = x + offset stays in registers and the accumulators start from
// zero, so inverse_and_add's `acc += ExtProd` leaves hi in them.  x is read again after the
// transforms for lo (its address behind an opaque asm: hipcc otherwise keeps the first read's 32
// registers across them).  The pairs go through ext_pairs_chain, ext_pairs_global with each
// pair's sums completed at the pair: with ext_pairs_global hipcc defers them here as it does in
// k_rotate_chain's loop (256 + 256 registers and 924 B of scratch per lane at L = 3 against
// 256 + 38 and none).  The 2^level parents of a query share the level's selector,
// sel[(g >> level) * sel_stride].  Waves past B return before they read or write anything;
// nothing below is a workgroup barrier.
template <int L>
__global__ __launch_bounds__(64 * CMUX_WAVES) void k_demux(KParams P, DevTables TT,
                                                           const double2 *__restrict__ sel_rows,
                                                           const uint32_t *__restrict__ sel, uint32_t level,
                                                           uint32_t sel_stride, const uint32_t *__restrict__ src,
                                                           uint32_t *__restrict__ out, size_t B) {
    __shared__ C2 s_x[CMUX_WAVES][2 * 512];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), t = threadIdx.x & 63;
    const size_t g = (size_t)blockIdx.x * CMUX_WAVES + w;
    if (g >= B) return;
    const uint32_t *x = src + g * 2048;
    const double2 *row = sel_rows + (size_t)sel[(g >> level) * sel_stride] * (2 * L * 1024);
    RegTw T;
    T.init(TT.tw, t);
    C2 twl[8];
#pragma unroll
    for (int m = 0; m < 8; m++) twl[m] = TT.twist[t + 64 * m];
    uint32_t tA[16], tB[16];
#pragma unroll
    for (int m = 0; m < 16; m++) {
        tA[m] = x[t + 64 * m] + P.offset;
        tB[m] = x[1024 + t + 64 * m] + P.offset;
    }
    C2 fa[8], fb[8];
    ext_pairs_chain<L>(tA, tB, row, P.bgbit, T, twl, s_x[w], t, fa, fb);
    uint32_t hiA[16], hiB[16];
#pragma unroll
    for (int m = 0; m < 16; m++) hiA[m] = hiB[m] = 0;
    uint32_t near = NEAR_NONE;
    inverse_and_add<false, 1>(fa, fb, s_x[w], T, twl, t, hiA, hiB, near);
    const uint32_t *xr = x;
    asm volatile("" : "+s"(xr)::"memory");
    uint32_t *lo = out + g * 4096, *hi = lo + 2048;
#pragma unroll
    for (int m = 0; m < 16; m++) {
        hi[t + 64 * m] = hiA[m];
        hi[1024 + t + 64 * m] = hiB[m];
        lo[t + 64 * m] = xr[t + 64 * m] - hiA[m];
        lo[1024 + t + 64 * m] = xr[1024 + t + 64 * m] - hiB[m];
    }
}

// The workgroup form of a demux level, as k_cmux_shared is of a CMUX level: the 4 waves' parents
// g0 .. g0 + 3 (g0 = 4 * blockIdx.x) belong to one query (levels of at least 4 parents per
// query, level >= 2) and so share their selector, whose row pairs are staged in LDS once for
// all four (ext_pairs_shared).  launch_demux refuses a B that is not a multiple of 4.
template <int L>
__global__ __launch_bounds__(64 * CMUX_WAVES) void k_demux_shared(KParams P, DevTables TT,
                                                                  const double2 *__restrict__ sel_rows,
                                                                  const uint32_t *__restrict__ sel, uint32_t level,
                                                                  uint32_t sel_stride,
                                                                  const uint32_t *__restrict__ src,
                                                                  uint32_t *__restrict__ out, size_t B) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[CS_LDS_BK + CMUX_WAVES * 2 * 512 * 16];
    double2 *s_bk = reinterpret_cast<double2 *>(smem);
    const int tid = threadIdx.x, t = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    C2 *s_x = reinterpret_cast<C2 *>(smem + CS_LDS_BK) + w * 2 * 512;
    const size_t g0 = (size_t)blockIdx.x * CMUX_WAVES, g = g0 + w;  // g < B: B is a multiple of 4 (launch_demux)
    const double2 *row = sel_rows + (size_t)sel[(g0 >> level) * sel_stride] * (2 * L * 1024);
    RegTw T;
    T.init(TT.tw, t);
    C2 twl[8];
#pragma unroll
    for (int m = 0; m < 8; m++) twl[m] = TT.twist[t + 64 * m];
    const uint32_t *x = src + g * 2048;
    uint32_t tA[16], tB[16];
#pragma unroll
    for (int m = 0; m < 16; m++) {
        tA[m] = x[t + 64 * m] + P.offset;
        tB[m] = x[1024 + t + 64 * m] + P.offset;
    }
    C2 fa[8], fb[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        fa[q] = c2(0.0, 0.0);
        fb[q] = c2(0.0, 0.0);
    }
    ext_pairs_shared<L>(tA, tB, row, P.bgbit, T, twl, s_x, t, tid, s_bk, fa, fb);
    uint32_t hiA[16], hiB[16];
#pragma unroll
    for (int m = 0; m < 16; m++) hiA[m] = hiB[m] = 0;
    uint32_t near = NEAR_NONE;
    inverse_and_add<false, 1>(fa, fb, s_x, T, twl, t, hiA, hiB, near);
    const uint32_t *xr = x;
    asm volatile("" : "+s"(xr)::"memory");
    uint32_t *lo = out + g * 4096, *hi = lo + 2048;
#pragma unroll
    for (int m = 0; m < 16; m++) {
        hi[t + 64 * m] = hiA[m];
        hi[1024 + t + 64 * m] = hiB[m];
        lo[t + 64 * m] = xr[t + 64 * m] - hiA[m];
        lo[1024 + t + 64 * m] = xr[1024 + t + 64 * m] - hiB[m];
    }
}

// The scatter-add's sum: table[i][w] += sum over q < nq of leaves[(q * trlwes + i) * 2N + w] in
// wrapping u32.  Block = 64 consecutive words of the table, whose lane-0-wave thread alone reads
// and writes the word: no atomics, and integer adds commute, so the split of the queries over
// the 16 waves (q = wave, wave + 16, ...; joined through LDS as in k_pack_rotate_acc) changes no
// word.  One thread per word would leave a table of few TRLWEs on a handful of CUs (v = 1: 64
// waves walking all the queries).
constexpr int SCATTER_WAVES = 16;
__global__ __launch_bounds__(64 * SCATTER_WAVES) void k_scatter_reduce(const uint32_t *__restrict__ leaves, size_t nq,
                                                                       size_t trlwes, uint32_t *__restrict__ table) {
    __shared__ uint32_t red[SCATTER_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t x = (size_t)blockIdx.x * 64 + lane;  // word of the table: TRLWE x >> 11 (the grid covers it exactly)
    const size_t stride = trlwes * 2048;
    uint32_t acc = 0;
#pragma unroll 4
    for (size_t q = wave; q < nq; q += SCATTER_WAVES) acc += leaves[q * stride + x];
    red[wave][lane] = acc;
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int w = 1; w < SCATTER_WAVES; w++) acc += red[w][lane];
    table[x] += acc;
}

// sampleExtractIndex(trlwe, k) (trlwe.zig:146-162) for k < N = 1024: block
// b * C + c extracts coefficient coef[c] of TRLWE b into TLWELv1 b * C + c
// (1025 words): p[i] = a[k - i] (i <= k), -a[N + k - i] (i > k), p[N] = b[k].
__global__ __launch_bounds__(256) void k_sample_extract(const uint32_t *__restrict__ trlwe,
                                                        const uint32_t *__restrict__ coef, unsigned C,
                                                        uint32_t *__restrict__ out) {
    const uint32_t *x = trlwe + (size_t)(blockIdx.x / C) * 2048;
    const uint32_t k = coef[blockIdx.x % C];
    uint32_t *o = out + (size_t)blockIdx.x * 1025;
    for (uint32_t i = threadIdx.x; i < 1024; i += 256) o[i] = i <= k ? x[k - i] : 0u - x[1024 + k - i];
    if (threadIdx.x == 0) o[1024] = x[1024 + k];
}

// The packing key switch's epilogue, one pass over the GEMM's sums.  Item g = b C + c of
// the batch has R_g = (0, (in_g.b, 0, ..., 0)) - sum_z part[z][g - item0][.] - bias in all 2N words (the
// bias of k_ks_gemm_reduce) and goes into out[b] as X^coef[c] R_g (polyMulWithXK, trgsw.zig:442-466, on
// each half): word p of a half takes R[p - k] for p >= k and -R[p - k + N] below.  Block = 64 consecutive
// words of one output TRLWE; its lane-0-wave thread owns the word: it alone reads (when the TRLWE's first
// items went through in an earlier chunk) and writes it, so there are no atomics.  The 16 waves walk the
// TRLWE's items of this chunk c = wave, wave + 16, ... and add up through LDS (wrapping sums commute): one
// TRLWE of 1,024 items is 32 blocks only, so the walk is what bounds it (4 waves: 0.34 ms per pack of
// 1,024 against 0.10 ms for the key switch, profiles/pack_bench_epilogue_4waves.json).
constexpr int PACK_ACC_WAVES = 16;
__global__ __launch_bounds__(64 * PACK_ACC_WAVES) void k_pack_rotate_acc(
    const uint32_t *__restrict__ in, int in_stride, int n_in, const uint32_t *__restrict__ part, int splits,
    uint32_t bias, const uint32_t *__restrict__ coef, size_t C, size_t item0, size_t M, uint32_t *__restrict__ out) {
    __shared__ uint32_t red[PACK_ACC_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t b = item0 / C + blockIdx.x / 32;
    const uint32_t x = (blockIdx.x % 32) * 64 + lane;  // word of the TRLWE: half x >> 10, coefficient p
    const uint32_t half = x >> 10, p = x & 1023u;
    const size_t first = b * C, lo = first > item0 ? first : item0;
    const size_t hi = first + C < item0 + M ? first + C : item0 + M;
    uint32_t acc = 0;
#pragma unroll 4
    for (size_t g = lo + wave; g < hi; g += PACK_ACC_WAVES) {
        const uint32_t k = coef[g - first];
        const size_t m = g - item0;
        const uint32_t q = (p - k) & 1023u;
        uint32_t r = bias;
        for (int z = 0; z < splits; z++) r += part[((size_t)z * M + m) * 2048 + half * 1024 + q];
        const uint32_t v = (half && q == 0 ? in[m * (size_t)in_stride + n_in] : 0u) - r;
        acc += p < k ? 0u - v : v;
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int w = 1; w < PACK_ACC_WAVES; w++) acc += red[w][lane];
    uint32_t *o = out + b * 2048 + x;
    *o = (lo == first ? 0u : *o) + acc;
}

hipError_t launch_pack_rotate_acc(const uint32_t *in, int n_in, const uint32_t *part, const PackSums &sums,
                                  const uint32_t *coef, size_t C, size_t item0, size_t M, uint32_t *out, hipStream_t s,
                                  const char **used) {
    if (M == 0 || C == 0) return hipSuccess;
    const size_t trlwes = (item0 + M - 1) / C - item0 / C + 1;  // output TRLWEs this chunk's items go to
    hipLaunchKernelGGL(k_pack_rotate_acc, dim3((unsigned)(trlwes * 32)), dim3(64 * PACK_ACC_WAVES), 0, s, in, n_in + 1,
                       n_in, part, sums.splits, sums.bias, coef, C, item0, M, out);
    if (used) *used = "k_pack_rotate_acc";
    return hipGetLastError();
}

template <int L>
static const char *cmux_launch(bool shared, dim3 grid, dim3 block, hipStream_t s, const KParams &P, const DevTables &T,
                               const CmuxBatch &b) {
    const double2 *rows = reinterpret_cast<const double2 *>(b.sel_rows);
    if (shared) {
        hipLaunchKernelGGL(k_cmux_shared<L>, grid, block, 0, s, P, T, rows, b.sel, b.src0, b.i0, b.src1, b.i1, b.out, b.B);
        return L == 1 ? "k_cmux_shared<1>" : L == 2 ? "k_cmux_shared<2>" : "k_cmux_shared<3>";
    }
    hipLaunchKernelGGL(k_cmux<L>, grid, block, 0, s, P, T, rows, b.sel, b.src0, b.i0, b.src1, b.i1, b.out, b.B);
    return L == 1 ? "k_cmux<1>" : L == 2 ? "k_cmux<2>" : "k_cmux<3>";
}

hipError_t launch_cmux(const KParams &P, const DevTables &T, const CmuxBatch &b, bool shared, hipStream_t s,
                       const char **used) {
    if (b.B == 0) return hipSuccess;
    if (shared && b.B % CMUX_WAVES != 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((b.B + CMUX_WAVES - 1) / CMUX_WAVES)), block(64 * CMUX_WAVES);
    const char *name = "";
    switch (P.L) {
    case 1: name = cmux_launch<1>(shared, grid, block, s, P, T, b); break;
    case 2: name = cmux_launch<2>(shared, grid, block, s, P, T, b); break;
    case 3: name = cmux_launch<3>(shared, grid, block, s, P, T, b); break;
    default: return hipErrorInvalidValue;
    }
    if (used) *used = name;
    return hipGetLastError();
}

template <int L>
static const char *graph_launch(dim3 grid, dim3 block, hipStream_t s, const KParams &P, const DevTables &T,
                                const GraphLevel &b) {
    hipLaunchKernelGGL(k_cmux_rot<L>, grid, block, 0, s, P, T, reinterpret_cast<const double2 *>(b.sel_rows), b.addr, b.k,
                       b.nodes, b.cnt, b.leaves, b.slots, b.n_slots, (uint32_t)(b.nq * b.cnt));
    return L == 1 ? "k_cmux_rot<1>" : L == 2 ? "k_cmux_rot<2>" : "k_cmux_rot<3>";
}

hipError_t launch_cmux_graph_level(const KParams &P, const DevTables &T, const GraphLevel &b, hipStream_t s,
                                   const char **used) {
    if (b.nq == 0 || b.cnt == 0) return hipSuccess;
    if (b.nq > 0xFFFFFFFFull / b.cnt) return hipErrorInvalidValue;  // the item index is 32 bits wide
    const size_t B = b.nq * b.cnt;
    const dim3 grid((unsigned)((B + CMUX_WAVES - 1) / CMUX_WAVES)), block(64 * CMUX_WAVES);
    const char *name = "";
    switch (P.L) {
    case 1: name = graph_launch<1>(grid, block, s, P, T, b); break;
    case 2: name = graph_launch<2>(grid, block, s, P, T, b); break;
    case 3: name = graph_launch<3>(grid, block, s, P, T, b); break;
    default: return hipErrorInvalidValue;
    }
    if (used) *used = name;
    return hipGetLastError();
}

hipError_t launch_cmux_graph_roots(const uint32_t *roots, uint32_t R, const uint32_t *leaves, const uint32_t *slots,
                                   uint32_t n_slots, uint32_t *out, size_t nq, hipStream_t s) {
    if (nq == 0 || R == 0) return hipSuccess;
    if (nq > 0xFFFFFFFFull / R) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_graph_roots, dim3((unsigned)(nq * R)), dim3(256), 0, s, roots, R, leaves, slots, n_slots, out);
    return hipGetLastError();
}

template <int L>
static const char *rotate_launch(dim3 grid, dim3 block, hipStream_t s, const KParams &P, const DevTables &T,
                                 const RotateBatch &b) {
    hipLaunchKernelGGL(k_rotate_chain<L>, grid, block, 0, s, P, T, reinterpret_cast<const double2 *>(b.sel_rows), b.sel,
                       b.rot, b.h, b.src, b.i_src, b.out, b.B);
    return L == 1 ? "k_rotate_chain<1>" : L == 2 ? "k_rotate_chain<2>" : "k_rotate_chain<3>";
}

hipError_t launch_rotate_chain(const KParams &P, const DevTables &T, const RotateBatch &b, hipStream_t s,
                               const char **used) {
    if (b.B == 0) return hipSuccess;
    if (b.h == 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((b.B + CMUX_WAVES - 1) / CMUX_WAVES)), block(64 * CMUX_WAVES);
    const char *name = "";
    switch (P.L) {
    case 1: name = rotate_launch<1>(grid, block, s, P, T, b); break;
    case 2: name = rotate_launch<2>(grid, block, s, P, T, b); break;
    case 3: name = rotate_launch<3>(grid, block, s, P, T, b); break;
    default: return hipErrorInvalidValue;
    }
    if (used) *used = name;
    return hipGetLastError();
}

template <int L>
static const char *demux_launch(bool shared, dim3 grid, dim3 block, hipStream_t s, const KParams &P, const DevTables &T,
                                const DemuxBatch &b) {
    const double2 *rows = reinterpret_cast<const double2 *>(b.sel_rows);
    if (shared) {
        hipLaunchKernelGGL(k_demux_shared<L>, grid, block, 0, s, P, T, rows, b.sel, b.level, b.sel_stride, b.src, b.out, b.B);
        return L == 1 ? "k_demux_shared<1>" : L == 2 ? "k_demux_shared<2>" : "k_demux_shared<3>";
    }
    hipLaunchKernelGGL(k_demux<L>, grid, block, 0, s, P, T, rows, b.sel, b.level, b.sel_stride, b.src, b.out, b.B);
    return L == 1 ? "k_demux<1>" : L == 2 ? "k_demux<2>" : "k_demux<3>";
}

hipError_t launch_demux(const KParams &P, const DevTables &T, const DemuxBatch &b, bool shared, hipStream_t s,
                        const char **used) {
    if (b.B == 0) return hipSuccess;
    // the workgroup form's 4 parents must belong to one query
    if (shared && (b.B % CMUX_WAVES != 0 || ((size_t)1 << b.level) < CMUX_SHARED_ITEMS)) return hipErrorInvalidValue;
    if (b.level > 31) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((b.B + CMUX_WAVES - 1) / CMUX_WAVES)), block(64 * CMUX_WAVES);
    const char *name = "";
    switch (P.L) {
    case 1: name = demux_launch<1>(shared, grid, block, s, P, T, b); break;
    case 2: name = demux_launch<2>(shared, grid, block, s, P, T, b); break;
    case 3: name = demux_launch<3>(shared, grid, block, s, P, T, b); break;
    default: return hipErrorInvalidValue;
    }
    if (used) *used = name;
    return hipGetLastError();
}

hipError_t launch_scatter_reduce(const uint32_t *leaves, size_t nq, size_t trlwes, uint32_t *table, hipStream_t s) {
    if (nq == 0 || trlwes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scatter_reduce, dim3((unsigned)(trlwes * 32)), dim3(64 * SCATTER_WAVES), 0, s, leaves, nq, trlwes,
                       table);
    return hipGetLastError();
}

hipError_t launch_sample_extract(const uint32_t *trlwe, const uint32_t *coef, size_t C, uint32_t *out_lv1, size_t B,
                                 hipStream_t s) {
    if (B == 0 || C == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sample_extract, dim3((unsigned)(B * C)), dim3(256), 0, s, trlwe, coef, (unsigned)C, out_lv1);
    return hipGetLastError();
}

}  // namespace tfhe
