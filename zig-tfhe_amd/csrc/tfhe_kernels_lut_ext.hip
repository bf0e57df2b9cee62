// tfhe_kernels_lut_ext.hip — the extended LUT bootstrap's blind rotation (include/tfhe_gpu.h
// "Extended LUT bootstrap"): the blind rotation in Z[X]/(X^(N E) + 1), E = 2 or 4,
// on E accumulator components over the key's own ring, so that the mod switch rounds to 2N E
// positions and a 5- or 6-bit digit survives it on the N = 1024 key.  Its own unit, like
// tfhe_kernels_leveled.hip: the bootstrap kernels' objects (tfhe_kernels.o,
// tfhe_kernels_whole.o), which tfhe_gpu_build_id() hashes, do not change with it.  Same flags as
// theirs (-ffp-contract=off: every f64 multiply and add rounds separately).
//
// Arithmetic: the reference's expression trees (FU = false, SMALL = false) whatever
// TFHE_OPT_ARITH says, as in every leveled kernel; the near-tie counter and flags are not touched.
#include "tfhe_device.hpp"

namespace tfhe {

// One workgroup per item, E waves; wave k owns component k for all n steps (k_rotate_chain's step
// with the rotated reads taken from another wave's accumulator).  LDS per wave: the accumulator
// (8 KB) and the transform exchange (16 KB, wave_sync only), plus the item's a~ as u16 (a~ <= 2N E
// = 8192): 50 KB at E = 2, 98 KB at E = 4, before the staged BK row pair of the LDS form below.
//   acc_k = mulxk(tv_{(k - r) mod E}, q + [k < r])           b~ = q E + r
//   step i, a~_i = q E + r:
//     tmp_k  = mulxk(acc_{(k - r) mod E}, q + [k < r]) - acc_k + offset     (rot_read: index and sign)
//     acc_k += ExtProd(BK_i, tmp_k)                                         (the pairs below, inverse_and_add)
// Every wave reads another wave's accumulator in a step and stores its own at the end of it, so a step
// has two workgroup barriers: one between the last use of the rotated reads' source (every wave is
// past its reads once it is past its transforms) and the stores, one between the stores and the next
// step's reads.  All E waves run all n steps (n and the barriers are workgroup-uniform; the grid is B
// blocks), so no wave leaves a barrier behind; after the last step nothing is stored to LDS and the
// accumulators go out from registers: component 0 only, or all E (the stage entry).
// The exponent q + [k < r] reaches 2N (q = 2N - 1 with k < r, and a~ = 2N E): it is reduced mod 2N
// before rot_read, whose index mask would take it as well.
// tv: the item's extended table, E consecutive TRLWELv1 at testvec + tv_sel[g] * E * 2N (tv_sel NULL:
// the one shared table at testvec); or, where tv_sel[g] has TV_SEL_EACH set, the one TRLWELv1 (any a) at
// tv_each + (tv_sel[g] & ~TV_SEL_EACH) * 2N for every component: the extended test vector of a select node is E
// copies of its ordinary one, so all E waves read it, each with its own exponent.  g is
// workgroup-uniform, so the choice is a scalar branch in the prologue only; the steps do not change.
//
// The BK rows, two forms (EXT_BK_LDS<E>), both measured at UINT4 with 1,024 items:
//   global  every wave reads its rows from global memory (ext_pairs_chain); all workgroups walk the BK in
//           the same order, so L2 serves them.  19.5 ms at E = 2, 37.8 ms at E = 4.
//   LDS     the E waves of a workgroup multiply by the same BK_i, so its 64 E threads stage each row pair
//           (32 KB) in LDS once, as k_cmux_shared does, and every wave runs the LDS MAC on it
//           (ext_pairs_lds; 82 KB of LDS at E = 2, 130 KB at E = 4, two more workgroup barriers per pair).
//           22.8 ms at E = 2, 26.0 ms at E = 4.
// The default is the faster form at each E: global at E = 2, LDS at E = 4.  TFHE_EXT_BK_FORM (a
// development switch: an A/B library, tools/libvar_build.sh) forces one form at both: 0 global, 1 LDS.
#ifdef TFHE_EXT_BK_FORM
template <int E>
constexpr bool EXT_BK_LDS = TFHE_EXT_BK_FORM != 0;
#else
template <int E>
constexpr bool EXT_BK_LDS = E == 4;
#endif

template <int L, int E, int RP = 0>
DEV void ext_pairs_lds(const uint32_t *tA, const uint32_t *tB, const double2 *__restrict__ row, int bgbit,
                       const RegTw &T, const C2 *twl, C2 *xb, int t, int tid, double2 *s_bk, C2 *fa, C2 *fb) {
    if constexpr (RP < L) {
        constexpr int PER = 2048 / (64 * E);  // double2 per thread of a pair
        // this thread's piece of the pair, read before the forward transforms so that they hide the L2
        // latency; the address behind an opaque asm keeps the L pairs' loads at their pairs
        const double2 *src = row + (size_t)RP * 2048 + tid;
        asm volatile("" : "+v"(src)::"memory");
        double prx[PER], pry[PER];
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const double2 v = src[64 * E * j];
            prx[j] = v.x;
            pry[j] = v.y;
        }
        C2 d[2][8];
        forward_pair<L, RP, 1>(tA, tB, bgbit, T, twl, xb, t, d);
        if (RP > 0) __syncthreads();  // every wave is through the previous pair's MAC
#pragma unroll
        for (int j = 0; j < PER; j++) s_bk[64 * E * j + tid] = make_double2(prx[j], pry[j]);
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        mac_pair_lds<false>(fa, fb, d[0], d[1], s_bk, t);
        __builtin_amdgcn_sched_barrier(0);
        ext_pairs_lds<L, E, RP + 1>(tA, tB, row, bgbit, T, twl, xb, t, tid, s_bk, fa, fb);
    }
}

template <int L, int E>
__global__ __launch_bounds__(64 * E) void k_blind_rotate_ext(KParams P, DevTables TT, const uint32_t *__restrict__ in,
                                                             const uint32_t *__restrict__ testvec,
                                                             const uint32_t *__restrict__ tv_sel,
                                                             const uint32_t *__restrict__ tv_each,
                                                             const double2 *__restrict__ bk, uint32_t *__restrict__ out,
                                                             int all) {
    constexpr int ETA = E == 2 ? 1 : 2;
    static_assert(E == 2 || E == 4, "E = 1 is the ordinary blind rotation");
    __shared__ C2 s_x[E][2 * 512];
    __shared__ uint32_t s_acc[E][2048];
    __shared__ uint16_t s_at[1024];
    constexpr bool BK_LDS = EXT_BK_LDS<E>;
    __shared__ __attribute__((aligned(16))) double2 s_bk[BK_LDS ? 2048 : 1];  // one row pair (the LDS form)
    const int k = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const size_t g = blockIdx.x;
    const uint32_t n = (uint32_t)P.n;
    const uint32_t *x = in + g * (size_t)(n + 1);
    constexpr int SH = 32 - 11 - ETA;  // N = 1024: nbit + 1 = 11
    constexpr uint64_t HALF = (uint64_t)1 << (SH - 1);
    for (uint32_t i = threadIdx.x; i < n; i += 64 * E) s_at[i] = (uint16_t)(((uint64_t)x[i] + HALF) >> SH);
    uint32_t *acc = s_acc[k];
    {
        const uint32_t bt = (uint32_t)(2048 * E) - (uint32_t)(((uint64_t)x[n] + HALF) >> SH);  // in [0, 2N E]
        const int q = (int)(bt >> ETA), r = (int)(bt & (E - 1));
        const uint32_t sel = tv_sel ? tv_sel[g] : 0u;
        const uint32_t *tv = (sel & TV_SEL_EACH) ? tv_each + (size_t)(sel & ~TV_SEL_EACH) * 2048
                                                 : testvec + ((size_t)sel * E + ((k - r) & (E - 1))) * 2048;
        const int ex = (q + (k < r ? 1 : 0)) & 2047;
#pragma unroll
        for (int m = 0; m < 16; m++) {
            acc[lane + 64 * m] = rot_read(tv, lane + 64 * m, ex);
            acc[1024 + lane + 64 * m] = rot_read(tv + 1024, lane + 64 * m, ex);
        }
    }
    __syncthreads();
    uint32_t accA[16], accB[16];
    for (uint32_t i = 0; i < n; i++) {
        // the lane index behind an opaque asm in every step, as in k_rotate_chain: what a step
        // derives from it is computed in the step and not kept live across the loop
        int t = lane;
        asm volatile("" : "+v"(t));
        const uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_at[i]);
        const int q = (int)(at >> ETA), r = (int)(at & (E - 1));
        const uint32_t *from = s_acc[(k - r) & (E - 1)];
        const int ex = (q + (k < r ? 1 : 0)) & 2047;
        const double2 *row = bk + (size_t)i * (2 * L * 1024);
        RegTw T;
        T.init(TT.tw, t);
        C2 twl[8];
#pragma unroll
        for (int m = 0; m < 8; m++) twl[m] = TT.twist[t + 64 * m];
        uint32_t tA[16], tB[16];
#pragma unroll
        for (int m = 0; m < 16; m++) {
            tA[m] = rot_read(from, t + 64 * m, ex) - acc[t + 64 * m] + P.offset;
            tB[m] = rot_read(from + 1024, t + 64 * m, ex) - acc[1024 + t + 64 * m] + P.offset;
        }
        C2 fa[8], fb[8];
        if constexpr (BK_LDS) {
            int tid = (int)threadIdx.x;
            asm volatile("" : "+v"(tid));
#pragma unroll
            for (int q2 = 0; q2 < 8; q2++) fa[q2] = fb[q2] = c2(0.0, 0.0);  // fmaInFd1024 from 0.0 (0.0 + x == x)
            ext_pairs_lds<L, E>(tA, tB, row, P.bgbit, T, twl, s_x[k], t, tid, s_bk, fa, fb);
        } else {
            ext_pairs_chain<L>(tA, tB, row, P.bgbit, T, twl, s_x[k], t, fa, fb);
        }
        // acc_k again, from LDS: not held in 32 registers across the transforms
        int tr = lane;
        asm volatile("" : "+v"(tr));
#pragma unroll
        for (int m = 0; m < 16; m++) {
            accA[m] = acc[tr + 64 * m];
            accB[m] = acc[1024 + tr + 64 * m];
        }
        uint32_t near = NEAR_NONE;
        inverse_and_add<false, 1>(fa, fb, s_x[k], T, twl, t, accA, accB, near);
        if (i + 1 < n) {
            __syncthreads();  // every wave's rotated reads of this step precede the stores
#pragma unroll
            for (int m = 0; m < 16; m++) {
                acc[tr + 64 * m] = accA[m];
                acc[1024 + tr + 64 * m] = accB[m];
            }
            __syncthreads();  // the stores precede the next step's rotated reads (other waves' words)
        }
    }
    if (!all && k != 0) return;
    uint32_t *o = out + (all ? g * E + k : g) * 2048;
#pragma unroll
    for (int m = 0; m < 16; m++) {
        o[lane + 64 * m] = accA[m];
        o[1024 + lane + 64 * m] = accB[m];
    }
}

template <int L, int E>
static const char *ext_launch(dim3 grid, hipStream_t s, const KParams &P, const DevTables &T, const BrExtBatch &b) {
    hipLaunchKernelGGL((k_blind_rotate_ext<L, E>), grid, dim3(64 * E), 0, s, P, T, b.in, b.testvec, b.tv_sel, b.tv_each,
                       reinterpret_cast<const double2 *>(b.bk), b.out, b.all ? 1 : 0);
    // the dispatch table: (L, E) -> the name last_kernels() reports
    static const char *const names[3][2] = {{"k_blind_rotate_ext<1,2>", "k_blind_rotate_ext<1,4>"},
                                            {"k_blind_rotate_ext<2,2>", "k_blind_rotate_ext<2,4>"},
                                            {"k_blind_rotate_ext<3,2>", "k_blind_rotate_ext<3,4>"}};
    return names[L - 1][E == 4];
}

hipError_t launch_blind_rotate_ext(const KParams &P, const DevTables &T, const BrExtBatch &b, hipStream_t s,
                                   const char **used) {
    if (b.B == 0) return hipSuccess;
    // the staged a~ fill 1024 u16; one block per item
    if (P.n < 1 || P.n > 1024 || P.N != 1024 || b.B > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)b.B);
    const char *name = nullptr;
    switch (P.L * 8 + (int)b.eta) {
    case 8 + 1: name = ext_launch<1, 2>(grid, s, P, T, b); break;
    case 8 + 2: name = ext_launch<1, 4>(grid, s, P, T, b); break;
    case 16 + 1: name = ext_launch<2, 2>(grid, s, P, T, b); break;
    case 16 + 2: name = ext_launch<2, 4>(grid, s, P, T, b); break;
    case 24 + 1: name = ext_launch<3, 2>(grid, s, P, T, b); break;
    case 24 + 2: name = ext_launch<3, 4>(grid, s, P, T, b); break;
    default: return hipErrorInvalidValue;  // eta = 0 has no instantiation here: it is the ordinary blind rotation
    }
    if (used) *used = name;
    return hipGetLastError();
}

}  // namespace tfhe
