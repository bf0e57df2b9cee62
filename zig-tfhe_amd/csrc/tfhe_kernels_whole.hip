// tfhe_kernels_whole.hip — the default whole-form blind-rotation kernels, in
// their own compilation unit, built with hipcc's max-memory-clause machine
// scheduler (Makefile).  That scheduler groups the kernels' LDS operations into
// clauses: 6.37-6.41 vs 6.48-6.55 ms per 1,024 gates, alternating on two boxes,
// the same words (profiles/r03r_ab_sched_strategy.txt).  Applied to the whole
// library it cost the latency form 2 % (16-bit adder 101.5 vs 99.7 ms), hence
// the separate unit.
//
//  - L = 3 (the 128/80-bit sets, fused arithmetic): k_blind_rotate_assist, the
//    whole form whose loader waves also own the accumulator's b polynomial
//    (round 5, below);
//  - L = 1, 2 (fused): k_blind_rotate<L, true, true> (tfhe_device.hpp).
//
// Whole form with loader assist (round 5, VERDICT r04 item 2: "give the loader
// waves VALU work").  In k_blind_rotate a loader wave sleeps ~23.7 k cycles per
// step beside its gate wave, on the same SIMD.  Here it owns the accumulator's
// b polynomial: after the gate's last MAC of step i the gate hands it the
// product spectrum fb (8 KB through LDS), and the loader runs the inverse
// transform of b, the untwist, the guarded torus conversion and the acc_b
// update, then (knowing a~_{i+1}) the rotation gather of b and the flipped tmp
// words tB of step i+1, which it hands back (4 KB).  The gate keeps polynomial
// a: one inverse transform instead of the pipelined pair, a-only gather and tmp
// words, and it reads tB only before row pair 1 (rows 0, 1 are a's levels 0, 1
// at L = 3), so the loader's work runs beside the gate's inverse of a, the next
// step's gather and pair 0.  Measured (device-resident NAND, 1,024 gates,
// alternating with k_blind_rotate<3,true,true> on one box): 6.08-6.11 vs
// 6.15-6.16 ms.  Measured and not kept: the b work after the loader's refill
// wait (6.65 ms: the 96-unit sleep makes tB late), exchange 2 in registers in
// the loader's inverse (6.15 ms) or through LDS in the gate's (6.23 ms), the
// gate waves at issue priority 1 (6.17-6.18 ms), the loader at priority 1 for
// its b work (6.70 ms), loader polls at sleep 16 / 32 / 64 (6.33-6.41 ms)
// (profiles/r05_ab_assist.txt).
//
// LDS (152 KB): BK slots 2 x 32 KB, twiddles + twist 16 KB; per gate X (8 KB:
// acc_a copy in its first 4 KB between steps, the gate's exchange buffer during
// its transforms) and Y (8 KB: the fb hand-off, then the loader's exchange
// buffer, then acc_b copy [0, 4 KB) + tB [4, 8 KB)); a~ 2 KB per gate; counters.
// Same arithmetic, row order and words as k_blind_rotate at L = 3 (fused).
//
// Loader schedule, pair k = 3i + rp (slot protocol unchanged): publish k; at
// k = 3i: wait fb(i - 1), inverse b of step i - 1, acc_b copy, gather + tB of
// step i, publish tB(i); wait until the gates are done with k - 1, issue k + 1.
#include "tfhe_device.hpp"

namespace tfhe {

constexpr int BA_LDS_X = 512 * 16;  // per gate
constexpr int BA_LDS_Y = 512 * 16;  // per gate (its loader's)
constexpr int BA_LDS_AT = 1024 * 2;
constexpr int BA_LDS_SYNC = 64;  // pub[2] done[2] fb_ready[4] tb_ready[4]
constexpr int BA_X_AT = BR_LDS_BK + BR_LDS_TW + BR_LDS_TWIST;
constexpr int BA_Y_AT = BA_X_AT + BR_WAVES * BA_LDS_X;
constexpr int BA_AT_AT = BA_Y_AT + BR_WAVES * BA_LDS_Y;
constexpr int BA_LDS_TOTAL = BA_AT_AT + BR_WAVES * BA_LDS_AT + BA_LDS_SYNC;
static_assert(BA_LDS_TOTAL <= 160 * 1024, "assist form LDS");
static_assert(BA_X_AT % 4096 == 0 && BA_Y_AT % 4096 == 0 && BA_LDS_X % 4096 == 0, "gathers need 4 KB-aligned copies");

// Rotation gather of ONE polynomial (1,024 words at the 4 KB-aligned byte address
// `base`), as gather_rot: lane word m = coefficient t + 64m of X^a~ p, sign in bit
// 12 of xb[m].
DEV void gather_rot_one(uint32_t base, int t, int at, uint32_t *xb, uint32_t *v) {
    const uint32_t rbb = (uint32_t)((t - at) & 2047) << 2;
    const uint32_t mask = __builtin_amdgcn_readfirstlane(0xFFCu);
    uint32_t vmask;
    asm volatile("v_mov_b32 %0, %1" : "=v"(vmask) : "s"(mask));
#pragma unroll
    for (int m = 0; m < 16; m++) {
        xb[m] = rbb + 256u * m;
        uint32_t a;
        asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(a) : "v"(xb[m]), "v"(vmask), "s"(base));
        v[m] = lds_read_u32(a);
    }
}

// Inverse transform of ONE accumulated spectrum (fft1024), untwist, guarded
// conversion and the CMUX add into acc (lane-local); exchange 1 through xb,
// exchange 2 in registers.  The single-transform fft512<1, true> written out, so
// that the 8 untwist factors are read as one group ahead of pass C, whose
// butterflies cover them: behind pass C hipcc reads them two at a time, each
// pair three instructions before its use, and this wave has no second transform
// to fill the waits.  The empty asm pins pass C behind the reads (instruction
// selection places pure arithmetic freely across a scheduling fence).  Measured
// the same way and not kept: the pass-B twiddles ahead of exchange 1's stores
// (slower), the pass-C twiddles ahead of exchange 2 (slower alone, level with
// this when combined with it); profiles/ab_lds_read_groups.txt.
// tres: the caller's resident twist factors, tres[m] = twist_t[64 m] for m < nres
// (the gate wave's, TWIST_RES below); those are not read again.
template <bool FU, bool EX2LDS = false>
DEV void inverse_one(const C2 *f, C2 *xb, const LdsTw &T, const C2 *twist_t, int t, uint32_t *acc, uint32_t &near,
                     const C2 *tres = nullptr, int nres = 0) {
    C2 e[1][8], tu[8];
#pragma unroll
    for (int q = 0; q < 8; q++) e[0][q] = f[br3(q)];
    passA<true, FU>(e[0], T.a);
    exchange1<1>(e, xb, t);
    {
        C2 w[7];
        T.pass_b(w, t);
        passBC<true, FU>(e[0], w);
    }
    exchange2<1, EX2LDS>(e, xb, t);
    {
        C2 w[7];
        T.pass_c(w, t);
#pragma unroll
        for (int q = 0; q < 8; q++) tu[q] = q < nres ? tres[q] : twist_t[64 * q];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 8; q++) asm volatile("" : "+v"(e[0][q].x), "+v"(e[0][q].y));
        passBC<true, FU>(e[0], w);
    }
    uint32_t nq[2] = {NEAR_NONE, NEAR_NONE};
#pragma unroll
    for (int q = 0; q < 8; q++) {
        double re, im;
        untwist_out<false, FU>(e[0][q], tu[q], re, im);
        acc[q] += to_torus<true, FU>(re, nq[0]);
        acc[q + 8] += to_torus<true, FU>(im, nq[1]);
    }
    near &= nq[0] & nq[1];
}

// Bounded poll with a short sleep (hand-offs between a gate and its loader).
// Its own SGPR flag, ORed into `fail` through a vector value (one shared "+s"
// flag across this loop's asm blocks made hipcc emit an illegal VGPR-to-SGPR copy).
DEV void spin_short(const uint32_t *p, uint32_t target, uint32_t cap, uint32_t &fail) {
    uint32_t f = 0;
    spin_until_ge<1>(p, target, cap, f);
    fail |= f;
}

// spin_short on the loader's tB counter with the 16 tB words (tb_t[64 m], m < 16)
// read in the counter's LDS batch, as wait_pair_first_group reads the MAC's first
// group: one LDS round trip instead of the counter's and then the words'.  A
// wave's LDS operations execute in order, so words read behind a counter value
// that says "written" are the written ones; a counter that is short sleeps and
// reads all of them again, bounded as spin_short is.  Alone it measured level with
// the parent, with the resident twist factors (TWIST_RES) 0.2-0.5 % below them
// alone (profiles/gate_wave_early_reads_ab.txt).
DEV void wait_tb_words(const uint32_t *p, uint32_t target, const uint32_t *tb_t, uint32_t cap, uint32_t &fail,
                       uint32_t *tb) {
    typedef __attribute__((ext_vector_type(2))) unsigned int u2;
    u2 w0, w1, w2, w3, w4, w5, w6, w7;
    uint32_t v, sv, cnt, f = 0;
    const uint32_t caddr = (uint32_t)(size_t)(const lds_void_t *)p;
    const uint32_t taddr = (uint32_t)(size_t)(const lds_void_t *)tb_t;
    asm volatile(
        "s_mov_b32 %[cnt], %[cap]\n"
        "1:\n\t"
        "ds_read_b32 %[v], %[ca]\n\t"
        "ds_read2st64_b32 %[w0], %[ta] offset1:1\n\t"
        "ds_read2st64_b32 %[w1], %[ta] offset0:2 offset1:3\n\t"
        "ds_read2st64_b32 %[w2], %[ta] offset0:4 offset1:5\n\t"
        "ds_read2st64_b32 %[w3], %[ta] offset0:6 offset1:7\n\t"
        "ds_read2st64_b32 %[w4], %[ta] offset0:8 offset1:9\n\t"
        "ds_read2st64_b32 %[w5], %[ta] offset0:10 offset1:11\n\t"
        "ds_read2st64_b32 %[w6], %[ta] offset0:12 offset1:13\n\t"
        "ds_read2st64_b32 %[w7], %[ta] offset0:14 offset1:15\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_readfirstlane_b32 %[sv], %[v]\n\t"
        "s_cmp_ge_u32 %[sv], %[tgt]\n\t"
        "s_cbranch_scc1 2f\n\t"
        "s_sleep 1\n\t"
        "s_sub_u32 %[cnt], %[cnt], 1\n\t"
        "s_cmp_eq_u32 %[cnt], 0\n\t"
        "s_cbranch_scc0 1b\n\t"
        "s_mov_b32 %[fail], 1\n"
        "2:"
        : [v] "=&v"(v), [w0] "=&v"(w0), [w1] "=&v"(w1), [w2] "=&v"(w2), [w3] "=&v"(w3), [w4] "=&v"(w4),
          [w5] "=&v"(w5), [w6] "=&v"(w6), [w7] "=&v"(w7), [sv] "=&s"(sv), [cnt] "=&s"(cnt), [fail] "+s"(f)
        : [ca] "v"(caddr), [ta] "v"(taddr), [tgt] "s"(target), [cap] "s"(cap)
        : "memory", "scc");
    fail |= f;
    const u2 w[8] = {w0, w1, w2, w3, w4, w5, w6, w7};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        tb[2 * j] = w[j].x;
        tb[2 * j + 1] = w[j].y;
    }
}

// Twist factors the gate wave keeps in VGPRs across its step loop: the factors
// of coefficients t + 64 m, m < TWIST_RES.  The step uses the same 8 factors four
// times (pair 0's, pairs 1 and 2's, the untwist's): 32 ds_read_b128 per step, 8
// with 6 resident.  6 is what fits: 254 VGPRs, no scratch, 2 waves per SIMD; 7
// spill 16 B per lane.  4 / 6 resident: 0.5 / 0.7 % below the parent
// (profiles/gate_wave_early_reads_ab.txt).
constexpr int TWIST_RES = 6;
// The gate wave's 8 twist factors in transform order, tw[q] = factor of
// coefficient t + 64 br3(q) (read_twist8), from the resident ones or LDS.
DEV void twist8_resident(C2 *tw, const C2 *tres, const C2 *twist_t) {
#pragma unroll
    for (int q = 0; q < 8; q++) tw[q] = br3(q) < TWIST_RES ? tres[br3(q)] : twist_t[64 * br3(q)];
}

template <bool FU, bool TV = false>
__global__ __launch_bounds__(512, 1) void k_blind_rotate_assist(
    KParams P, DevTables TT, const uint8_t *__restrict__ ops, const uint32_t *__restrict__ in_a,
    const uint32_t *__restrict__ in_b, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ testvec,
    const double2 *__restrict__ bkd, uint32_t *__restrict__ out, int out_mode, size_t B) {
    constexpr int L = 3;
    __shared__ __attribute__((aligned(16))) unsigned char smem[BA_LDS_TOTAL];
    const int tid = threadIdx.x;
    const int t = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader = w >= BR_WAVES;
    const int gi = loader ? w - BR_WAVES : w;  // the gate this wave serves
    double2 *s_bk = reinterpret_cast<double2 *>(smem);
    C2 *s_tw = reinterpret_cast<C2 *>(smem + BR_LDS_BK);
    C2 *s_twist = reinterpret_cast<C2 *>(smem + BR_LDS_BK + BR_LDS_TW);
    C2 *X = reinterpret_cast<C2 *>(smem + BA_X_AT + gi * BA_LDS_X);
    C2 *Y = reinterpret_cast<C2 *>(smem + BA_Y_AT + gi * BA_LDS_Y);
    uint32_t *X32 = reinterpret_cast<uint32_t *>(X), *Y32 = reinterpret_cast<uint32_t *>(Y);
    uint16_t *s_at = reinterpret_cast<uint16_t *>(smem + BA_AT_AT + gi * BA_LDS_AT);
    uint32_t *s_sync = reinterpret_cast<uint32_t *>(smem + BA_LDS_TOTAL - BA_LDS_SYNC);
    uint32_t *fb_ready = s_sync + 4, *tb_ready = s_sync + 8;
    if (lds_layout_bad(smem)) {
        if (tid == 0) __hip_atomic_fetch_or(P.err, (uint32_t)DEV_ERR_LDS_LAYOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int n = P.n;
    const size_t g_raw = (size_t)blockIdx.x * BR_WAVES + gi;
    const bool valid = g_raw < B;
    const size_t g = valid ? g_raw : B - 1;  // ragged tail: compute a copy, store nothing
    const size_t ia = idx ? idx[2 * g] : g, ib = idx ? idx[2 * g + 1] : g;
    const uint32_t *A = in_a + ia * (size_t)(n + 1);
    const uint32_t *Bv = in_b ? in_b + ib * (size_t)(n + 1) : A;
    const int op = ops ? (int)ops[g] : 255;
    // the item's own table (the clamped g), for the gate wave's polynomial a and the loader wave's b alike
    if constexpr (TV) testvec = item_testvec(P, testvec, g);
    const uint32_t spin_cap = P.spin_cap ? P.spin_cap : BR_SPIN_CAP_DEFAULT;
    const uint32_t msbs = digit_msbs(L, P.bgbit);
    const uint32_t pairs = (uint32_t)n * L;

    if (loader) {
        const int ltid = tid - 64 * BR_WAVES;
        __builtin_amdgcn_s_setprio(LOADER_PRIO);
        const size_t stride = (size_t)L * 2048;
        const uint32_t loader_cap = spin_cap / LOADER_SLEEP > 0 ? spin_cap / LOADER_SLEEP : 1u;
        uint32_t near = NEAR_NONE, fail = 0;
        issue_bk_pair_async(bkd, s_bk, ltid);  // pair 0 into slot 0
        // b~ of this wave's item (trgsw.zig:312), as the gate computes it
        int bt = 0;
        if (t == (n & 63)) {
            const uint32_t c = gate_combine(op, A[n], Bv[n], true);
            bt = 2048 - (int)(uint32_t)(((uint64_t)c + (1ull << 20)) >> 21);
        }
        bt = __builtin_amdgcn_readlane(bt, n & 63);
        uint32_t accB[16];
#pragma unroll
        for (int m = 0; m < 16; m++) accB[m] = rot_read(testvec + 1024, t + 64 * m, bt);
        __syncthreads();  // the gates' prologue: counters zeroed, tables and a~ in LDS
        LdsTw T;
        T.init(s_tw);  // pass-A twiddles from LDS (VGPRs): in SGPRs this loop failed to compile
        const C2 *twist_t = s_twist + t;
        const uint32_t base = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(lds_void_t *)Y32);  // acc_b copy: Y[0, 4 KB)
        PhaseProf lp;  // tools/phase_prof.hip assist: 0 vmcnt + pub, 1 fb wait, 2 inverse b, 3 gather + tB, 4 refill wait + issue
        lp.start();
        for (uint32_t k = 0; k < pairs; k++) {
            lp.mark(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of pair k landed
            counter_add(s_sync + (k & 1));
            // the b work as soon as the own gate's fb is in, before the wait for the next refill (with its
            // 96-unit sleep): 6.15 vs 6.65 ms after it
            if (k % L == 0) {
                const uint32_t i = k / L;
                if (i > 0) {  // step i - 1's b polynomial: fb from the gate, inverse, CMUX add
                    lp.mark(1);
                    spin_short(fb_ready + gi, i, spin_cap, fail);
                    lp.mark(2);
                    C2 f[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) f[q] = Y[q * 64 + t];
                    inverse_one<FU, true>(f, Y, T, twist_t, t, accB, near);
                }
                lp.mark(3);
                wave_sync();  // the exchange's reads precede the copy's writes
#pragma unroll
                for (int m = 0; m < 16; m++) Y32[t + 64 * m] = accB[m];
                wave_sync();
                // step i's tB: X^{a~_i} acc_b - acc_b + offset, flipped (tmp_word)
                const int at = __builtin_amdgcn_readfirstlane((int)s_at[i]);
                uint32_t v[16], xb[16];
                gather_rot_one(base, t, at, xb, v);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int m = 0; m < 16; m++) {
                    const uint32_t sg = gather_sign(xb[m]), off_s = P.offset - sg;
                    Y32[1024 + t + 64 * m] = tmp_word(v[m], sg, off_s, accB[m], msbs);
                }
                __builtin_amdgcn_sched_barrier(0);
                counter_add(tb_ready + gi);  // tB(i) written (the LDS runs this wave's ops in order)
                lp.mark(0);
            }
            if (k + 1 < pairs) {
                const uint32_t k1 = k + 1;
                lp.mark(4);
                spin_until_ge<LOADER_SLEEP>(s_sync + 2 + (k1 & 1), 4u * (k1 >> 1), loader_cap, fail);
                issue_bk_pair_async(bkd + (size_t)(k1 / L) * stride + (size_t)(k1 % L) * 2048, s_bk + (k1 & 1) * 2048,
                                    ltid);
            }
        }
        spin_short(fb_ready + gi, (uint32_t)n, spin_cap, fail);  // the last step's b polynomial
        {
            C2 f[8];
#pragma unroll
            for (int q = 0; q < 8; q++) f[q] = Y[q * 64 + t];
            inverse_one<FU, true>(f, Y, T, twist_t, t, accB, near);
        }
        lp.mark(5);
#ifdef TFHE_PHASE_PROF
        if (t == 0)
            lp.flush(g_phase_cycles + 8, 6);
#endif
        report_wait_failure(P, fail, DEV_ERR_LOADER_WAIT);
        if (FU) near_tie_flag(P, near, g, valid);
        if (!valid) return;
        // the b parts of the outputs (accB: coefficient t + 64m)
        if (out_mode == BR_OUT_LV1) {
            if (t == 0) out[g * (size_t)1025 + 1024] = accB[0];
        } else if (out_mode == BR_OUT_LV0_EXTRACT2) {
            if (t == 0) out[g * (size_t)(n + 1) + n] = accB[0];
        } else {
            uint32_t *o = out + g * (size_t)2048 + 1024;
#pragma unroll
            for (int m = 0; m < 16; m++) o[t + 64 * m] = accB[m];
        }
        return;
    }

    // ---- gate wave ----
    if (tid < 12) s_sync[tid] = 0u;
    for (int x = tid; x < 511; x += 256) s_tw[x] = TT.tw[x];
    for (int x = tid; x < 512; x += 256) s_twist[x] = TT.twist[x];
    int bt = 0;
    for (int i = t; i <= n; i += 64) {
        const uint32_t c = gate_combine(op, A[i], Bv[i], i == n);
        const uint32_t tl = (uint32_t)(((uint64_t)c + (1ull << 20)) >> 21);
        if (i < n) s_at[i] = (uint16_t)tl;
        else bt = 2048 - (int)tl;
    }
    bt = __builtin_amdgcn_readlane(bt, n & 63);
    uint32_t accA[16];
#pragma unroll
    for (int m = 0; m < 16; m++) {
        accA[m] = rot_read(testvec, t + 64 * m, bt);
        X32[t + 64 * m] = accA[m];
    }
    __syncthreads();  // tables, a~ and counters visible to every wave
    LdsTw T;
    T.init(s_tw, TT);
    const C2 *twist_t = s_twist + t;
    const uint32_t base = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(lds_void_t *)X32);  // acc_a copy: X[0, 4 KB)
    int at_next = s_at[0];
    uint32_t near = NEAR_NONE, fail = 0;
    C2 tres[TWIST_RES];
#pragma unroll
    for (int m = 0; m < TWIST_RES; m++) tres[m] = twist_t[64 * m];
    PhaseProf pp;  // tools/phase_prof.hip assist: 0 gather + tmp, 1 pair 0 fft, 2 pub waits, 3 macs, 4 tB wait, 5 pairs 1-2 fft, 6 fb hand-off, 7 inverse a
    pp.start();
    for (int i = 0; i < n; i++) {
        pp.mark(0);
        const int at = __builtin_amdgcn_readfirstlane(at_next);
        uint32_t tA[16], xb[16];
        C2 tw0[8];
        gather_rot_one(base, t, at, xb, tA);
        // the empty asm pins the resident factors in their registers: one definition per step, so hipcc
        // neither reads them again at a use nor moves the reads into the loop
#pragma unroll
        for (int m = 0; m < TWIST_RES; m++) asm volatile("" : "+v"(tres[m].x), "+v"(tres[m].y));
        twist8_resident(tw0, tres, twist_t);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < 16; m++) {
            const uint32_t sg = gather_sign(xb[m]), off_s = P.offset - sg;
            tA[m] = tmp_word(tA[m], sg, off_s, accA[m], msbs);
        }
        wave_sync();  // the gather's reads precede the exchanges' writes into X
        at_next = s_at[i + 1 < n ? i + 1 : i];
        C2 fa[8], fb[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            fa[q] = c2(0.0, 0.0);
            fb[q] = c2(0.0, 0.0);
        }
        uint32_t tbx[16];
#pragma unroll
        for (int rp = 0; rp < L; rp++) {
            C2 d[2][8];
            double2 kpre[4];
            if (rp == 0) {
                pp.mark(1);
                load_digits_pair0_regs<FU>(d, tA, nullptr, L, P.bgbit, tw0);  // rows 0, 1: a's levels 0, 1
            } else {
                // the pair's twist factors that are not resident as one read group: ahead of the tB wait (pair 1)
                // and of the digit conversions, which cover its latency (load_digits_pair_tbx)
                C2 twn[8];
                twist8_resident(twn, tres, twist_t);
                __builtin_amdgcn_sched_barrier(0);
                if (rp == 1) {  // tB(i) from the loader, packed with a's level 2 (load_digits_pair_tbx)
                    pp.mark(4);
                    uint32_t tb[16];
                    wait_tb_words(tb_ready + gi, (uint32_t)i + 1u, Y32 + 1024 + t, spin_cap, fail, tb);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int m = 0; m < 16; m++)
                        tbx[m] = __builtin_amdgcn_ubfe(tA[m], 32 - L * P.bgbit, P.bgbit) |
                                 (tb[m] & ~((1u << P.bgbit) - 1u));
                }
                pp.mark(5);
                load_digits_pair_tbx<FU>(d, tbx, rp, P.bgbit, twn);
            }
            fft512_x2<false, true, FU>(d, X, T, t);
            const uint32_t k = (uint32_t)(L * i + rp);
            pp.mark(2);
            wait_pair_first_group(s_sync, s_bk + (k & 1) * 2048 + t, k, spin_cap, fail, kpre);
            __builtin_amdgcn_sched_barrier(0);
            pp.mark(3);
            mac_pair_lds<FU>(fa, fb, d[0], d[1], s_bk + (k & 1) * 2048, t, kpre);
            __builtin_amdgcn_sched_barrier(0);
            counter_add(s_sync + 2 + (k & 1));
        }
        // hand fb to the loader (it read tB(i) from Y before: this wave's reads came first)
        pp.mark(6);
#pragma unroll
        for (int q = 0; q < 8; q++) Y[q * 64 + t] = fb[q];
        __builtin_amdgcn_sched_barrier(0);
        counter_add(fb_ready + gi);
        pp.mark(7);
        inverse_one<FU, false>(fa, X, T, twist_t, t, accA, near, tres, TWIST_RES);
        wave_sync();
#pragma unroll
        for (int m = 0; m < 16; m++) X32[t + 64 * m] = accA[m];
        wave_sync();
    }
    pp.mark(0);
#ifdef TFHE_PHASE_PROF
    if (t == 0)
        pp.flush(g_phase_cycles, 8);
#endif
    report_wait_failure(P, fail, DEV_ERR_GATE_WAIT);
    if (FU) near_tie_flag(P, near, g, valid);
    if (!valid) return;
    // the a parts of the outputs from the acc_a copy (the loader writes b's)
    if (out_mode == BR_OUT_LV1) {  // sampleExtractIndex(acc, 0): p[0] = a[0], p[j] = -a[N-j]; p[N] = b[0]: loader
        uint32_t *o = out + g * (size_t)1025;
        for (int j = t; j < 1024; j += 64) o[j] = j == 0 ? X32[0] : 0u - X32[1024 - j];
    } else if (out_mode == BR_OUT_LV0_EXTRACT2) {  // sampleExtractIndex2 (trlwe.zig:165-180)
        uint32_t *o = out + g * (size_t)(n + 1);
        for (int j = t; j < n; j += 64) o[j] = j == 0 ? X32[0] : 0u - X32[n - j];
    } else {
        uint32_t *o = out + g * (size_t)2048;
        for (int j = t; j < 1024; j += 64) o[j] = X32[j];
    }
}

BrEntry whole_default_kernel(int L, bool tv) {
    static const BrEntry kernels[2][3] = {
        {{k_blind_rotate<1, true, true>, "k_blind_rotate<1,true,true> (whole form, fused)"},
         {k_blind_rotate<2, true, true>, "k_blind_rotate<2,true,true> (whole form, fused)"},
         {k_blind_rotate_assist<true>, "k_blind_rotate_assist<true> (whole form, loader waves own polynomial b, fused)"}},
        // a test vector per item (KParams::tv_sel)
        {{k_blind_rotate<1, true, true, true>, "k_blind_rotate<1,true,true,TV> (per-item tables; whole form, fused)"},
         {k_blind_rotate<2, true, true, true>, "k_blind_rotate<2,true,true,TV> (per-item tables; whole form, fused)"},
         {k_blind_rotate_assist<true, true>,
          "k_blind_rotate_assist<true,TV> (per-item tables; whole form, loader waves own polynomial b, fused)"}},
    };
    return L >= 1 && L <= 3 ? kernels[tv][L - 1] : BrEntry{nullptr, ""};
}

}  // namespace tfhe
