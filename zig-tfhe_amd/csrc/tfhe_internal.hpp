// tfhe_internal.hpp — shared declarations between the C-ABI host layer
// (tfhe_gpu.cpp) and the HIP kernels (tfhe_kernels.hip).  Not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace tfhe {

struct C2 {
    double x, y;
};

// Device-side parameter block passed by value to every kernel.
struct KParams {
    int n;          // lv0 dimension
    int N;          // 1024
    int L;          // gadget levels
    int bgbit;      // log2 Bg
    int basebit;    // key-switch base bits
    int iks_t;      // key-switch levels
    uint32_t offset;  // decomposition offset (key.zig:121-131)
    int ks_stride;    // words per device KSK row: n+1 rounded up to 4 (16-B aligned rows)
    // Device error word of the context (sticky, OR of DEV_ERR_* bits; the host
    // reads it at every synchronisation point and fails the call, never
    // returning TFHE_OK over the words of a broken launch).  err[1] counts the
    // items the margin guard's recompute redid (cumulative).
    uint32_t *err;
    uint32_t spin_cap;  // polls before a slot-counter wait gives up (TFHE_OPT_BR_SPIN_CAP; 0 = default)
    // A second base for the TV = true instantiations (select nodes of LUT circuits),
    // in two halves that fill the block's two padding words (this one and the one behind `fallback`):
    // an entry of tv_sel with TV_SEL_EACH set reads tv_each + (entry & ~TV_SEL_EACH) * 2N, a test
    // vector the call built in its own frame, so one launch mixes the set's tables with those.  The
    // block keeps its size and every other member its place, so every kernel that does not read the
    // halves compiles to the code it had (a member appended moved the arguments behind the block).
    uint32_t tv_each_lo = 0;
    // Near-tie flags of the fused arithmetic's margin guard,
    // one byte per item of a blind-rotation launch, all zero between launches:
    // a fused kernel sets tie_flags[g] when item g rounded a value 1/4 or more off
    // its integer (within 1/4 of a tie); the reference-tree recompute launched
    // after it (fallback = 1) redoes the flagged items' workgroups and clears
    // their flags.  Sound while |v_fused - v_reference| < 1/4: measured max 0.094
    // on keygen'd keys, an empirical bound; keys outside that regime are refused
    // the fused arithmetic at load (key admission).
    uint8_t *tie_flags;
    int fallback;
    uint32_t tv_each_hi = 0;
    // Per-item test vector (LUT circuits): NULL, or one entry per item of the
    // launch; item g then starts from the TRLWELv1 at testvec + tv_sel[g] * 2N.  An item has
    // its own wave or workgroup in every form, so the offset is wave-uniform.  The host checks
    // every entry against the set's size before a launch.  Only the kernels' TV = true
    // instantiations read it (the launchers pick them when it is set): as a run-time branch it
    // changed the default kernel's registers and schedule and cost the bench 2.5 %.
    const uint32_t *tv_sel = nullptr;
};
constexpr uint32_t TV_SEL_EACH = 0x80000000u;
static_assert(sizeof(KParams) == 72, "KParams: tv_each_lo / tv_each_hi fill padding, the block keeps its size");
// Item g's test vector in a TV = true instantiation (g is wave-uniform, so these are scalar loads).
__device__ __forceinline__ const uint32_t *item_testvec(const KParams &P, const uint32_t *testvec, size_t g) {
    const uint32_t s = P.tv_sel[g];
    const uint32_t *each = reinterpret_cast<const uint32_t *>((uint64_t)P.tv_each_hi << 32 | P.tv_each_lo);
    return ((s & TV_SEL_EACH) ? each : testvec) + (size_t)(s & ~TV_SEL_EACH) * 2048;
}
inline void set_tv_each(KParams &P, const uint32_t *p) {
    P.tv_each_lo = (uint32_t)(uintptr_t)p;
    P.tv_each_hi = (uint32_t)((uint64_t)(uintptr_t)p >> 32);
}

// Bits of the device error word.
enum DevErr : uint32_t {
    DEV_ERR_GATE_WAIT = 1u,    // a gate wave's wait for a published BK slot timed out
    DEV_ERR_LOADER_WAIT = 2u,  // a loader wave's wait for a retired BK slot timed out
    DEV_ERR_LDS_LAYOUT = 4u,   // the blind rotation's LDS array is not at address 0 (gather_rot)
};
// Default bound of one slot-counter wait (sleep units).
constexpr uint32_t BR_SPIN_CAP_DEFAULT = 1u << 22;

// Device KSK: the reference's rows [(2^basebit*t*i) + 2^basebit*j + k] of
// n+1 words (key.zig:148-172), each padded to ks_stride words, plus a tail of
// KS_TAIL_WORDS zero words so chunked 16-B loads of the last row stay inside.
constexpr int KS_TAIL_WORDS = 64;
inline int ks_stride_for(int n) { return (n + 1 + 3) & ~3; }

// Output forms of the blind-rotation kernel.
enum BrOut : int {
    BR_OUT_LV1 = 0,    // sampleExtractIndex(acc, 0): TLWELv1, N+1 words per item
    BR_OUT_TRLWE = 1,  // the accumulator itself: TRLWELv1, 2N words per item
    // sampleExtractIndex2(acc, 0) (trlwe.zig:165-180), n+1 words per item: the
    // reference loops i < tlwe_lv0.N, so p[0] = a[0], p[i] = -a[n-i] (0<i<n), p[n] = b[0]
    BR_OUT_LV0_EXTRACT2 = 2,
};

// Device constant tables uploaded once per context (build_tables in tfhe_gpu.cpp).
struct DevTables {
    const C2 *twist;  // N/2 twisting factors exp(i*pi*k/N)        fft.zig:92-106
    const C2 *tw;     // N/2-1 forward stage twiddles (recurrence)  fft.zig:590-616
    C2 twa[4];        // tw[2], tw[4], tw[5], tw[6]: the lane-uniform pass-A twiddles, by value (SGPRs)
};

// Kernel-form choices of one context (tfhe_gpu_set_option, include/tfhe_gpu.h
// TFHE_OPT_*).  The defaults are the measured-fastest forms; the others stay
// for A/B runs and parity tests.  `used` (may be NULL) receives the name of
// the kernel a launcher ran.
struct LaunchOpts {
    int br_form = 0;     // 0 auto, 1 whole, 3 latency (wide), 5 octo (L = 1); 6 duo, 7 wide2, 8 whole without
                         // loader assist, 30 latency with row counters (A/B libraries only)
    int ks_form = 3;     // 0 lanes, 1 select / gather, 2 one-hot GEMM on the matrix cores (basebit 2), 3 auto
    int ks_narrow = 0;   // basebit 2: 1 forces the 32-word x 4-wave blocks
    int ks_groups = 0;   // basebit >= 5: item groups per block (0 auto = 4; 1, 2, 4, 8)
    int ks_sel_items = 8;  // select/gather form: items per block (8, 16, 32)
    int arith_strict = 0;  // 1: the reference's f64 expression trees even where fused multiply-adds round
                           // to the same integers (the L=3 / Bg=2^6 sets); 2: fused even on
                           // a key the admission check refused (margin-guard tests only)
    int key_fused_ok = 1;  // the resident BK passed the fused arithmetic's admission check
    int cmux_form = 0;     // table lookup's CMUX levels: 1 one wave per item; 0 auto and 2: the workgroup form where
                           // 4 consecutive items share a selector (levels with >= 4 pairs per query)
};
// The fused arithmetic runs unless the reference's trees are requested, and only on
// an admitted key unless forced (TFHE_OPT_ARITH, LaunchOpts::key_fused_ok).
inline bool fused_allowed(const LaunchOpts &O) {
    return O.arith_strict == 2 || (O.arith_strict == 0 && O.key_fused_ok != 0);
}

// The whole form exists for this gadget.  At L = 3 its gate waves keep tmp_a's level-2 field
// in the low bgbit bits of tmp_b's word (load_digits_pair_tbx, tfhe_device.hpp), which are
// free only while tmp_b's own lowest field starts at or above them: 32 - 3 bgbit >= bgbit.
// (3, 9) and (3, 10) run the latency form for every batch (launch_blind_rotate), and
// TFHE_OPT_BR_FORM 1 is refused there (option_ok).
inline bool whole_form_packs(int L, int bgbit) { return L != 3 || 4 * bgbit <= 32; }

// An A/B build (any -D define that changes the kernels or their timing:
// tools/ab_forms.sh, tools/libvar_build.sh, tools/phase_prof.hip, a Makefile
// EXTRA) compiles every unit with TFHE_AB_BUILD; tfhe_gpu_create refuses such a
// library unless TFHE_ALLOW_AB_BUILD=1 is set (tfhe_gpu_build_kind).
#if defined(TFHE_PHASE_PROF) && !defined(TFHE_AB_BUILD)
#define TFHE_AB_BUILD 1
#endif
bool kernels_ab_build();  // tfhe_kernels.hip: this unit was compiled as an A/B build
// The A/B-only blind-rotation forms (TFHE_OPT_BR_FORM 6, 7, 8, 30) are linked in
// (tools/ab/tfhe_ab_forms.hip), i.e. this is an A/B library.
bool ab_forms_linked();

// ---- launchers (tfhe_kernels.hip); all asynchronous on `s` --------------
// One batch of blind rotations, as the launchers pass it on (device pointers).
struct BrBatch {
    const uint8_t *ops = nullptr;   // gate op per item, or NULL (plain bootstrap)
    const uint32_t *in_a = nullptr;
    const uint32_t *in_b = nullptr;  // second gate input, or NULL
    const uint32_t *idx = nullptr;   // NULL, or B pairs (a, b) of ciphertext indices into in_a / in_b (circuit gather)
    const uint32_t *testvec = nullptr;
    const double *bk = nullptr;  // device-layout bootstrapping key (launch_bk_permute)
    uint32_t *out = nullptr;
    int out_mode = BR_OUT_LV1;
    size_t B = 0;
};
// The signature every blind-rotation kernel shares, and a kernel with the name
// last_kernels() reports for it.
using BrKernel = void (*)(KParams, DevTables, const uint8_t *, const uint32_t *, const uint32_t *, const uint32_t *,
                          const uint32_t *, const double2 *, uint32_t *, int, size_t);
struct BrEntry {
    BrKernel fn;
    const char *name;
};
// The default whole-form kernels (fused arithmetic; L = 3: k_blind_rotate_assist), built in
// their own unit with the max-memory-clause scheduler (tfhe_kernels_whole.hip).
BrEntry whole_default_kernel(int L, bool tv = false);  // tv: the per-item test vector instantiation (KParams::tv_sel)
// Grid and block of a form ('w' whole, 'W' latency, 'o' octo) over B items, and the one
// launch of a blind-rotation kernel: hipErrorInvalidValue for an entry without a kernel.
struct BrGeometry {
    dim3 grid, block;
};
BrGeometry br_geometry(char form, size_t B);
hipError_t launch_br(const BrEntry &k, const BrGeometry &g, const KParams &P, const DevTables &T, const BrBatch &b,
                     hipStream_t s, const char **used);
// The batch through the measured-fastest plan (or the form TFHE_OPT_BR_FORM forces), then the
// margin guard's recompute where the fused arithmetic ran.
hipError_t launch_blind_rotate(const KParams &P, const DevTables &T, const BrBatch &b, hipStream_t s,
                               const LaunchOpts &O = LaunchOpts(), const char **used = nullptr);
// CUs of the current device (256 when it cannot be queried) and
// launch_blind_rotate's modelled time for B items on `cus` CUs, in whole-form
// rounds of 4 x cus items (the circuit scheduler's level packing)
size_t device_cus();
double blind_rotate_cost(size_t B, size_t cus, int L = 3);
// dst[k] = (negate ? -1 : 1) * src[idx[k]] for k < count, n+1 words each
// (TLWELv0.neg: gates.zig:132-135)
hipError_t launch_tlwe_gather(const KParams &P, const uint32_t *src, const uint32_t *idx, uint32_t *dst,
                              size_t count, bool negate, hipStream_t s);
// The gemm form's device buffers: the MFMA-layout KSK
// (ks_gemm_bytes) and the K splits' partial sums (ks_gemm_part_bytes(B)).
struct KsGemm {
    const uint32_t *kg = nullptr;
    uint32_t *part = nullptr;
};
// n_in: input coefficients (1024 for the identity key switch, n for a proxy
// re-encryption key); (t, basebit) a shape with the GEMM form (ks_gemm_supported)
size_t ks_gemm_bytes(const KParams &P, int n_in, int t, int basebit);
size_t ks_gemm_part_bytes(const KParams &P, size_t B, int n_in, int basebit);
bool ks_gemm_supported(int t, int basebit);
// This call takes the GEMM form: the shape has it, its buffers are there (G may be
// NULL: the question before they are built) and TFHE_OPT_KS_FORM asks for it (2) or is auto (3).
bool ks_use_gemm(const LaunchOpts &O, int t, int basebit, size_t B, const KsGemm *G);
constexpr size_t KS_GEMM_INPUT_SLACK = 16;  // bytes past the last input row the gemm form may read
hipError_t launch_ksk_to_gemm(const KParams &P, const uint32_t *ksk, uint32_t *kg, int n_in, int t, int basebit,
                              hipStream_t s);
hipError_t launch_key_switch(const KParams &P, const uint32_t *lv1, const uint32_t *ksk,
                             uint32_t *out, size_t B, hipStream_t s, const LaunchOpts &O = LaunchOpts(),
                             const char **used = nullptr, const KsGemm *G = nullptr);
// The packing key switch (TLWELv0 -> a coefficient slot of a TRLWELv1) runs the same GEMM
// over a key whose n * t * 2^basebit rows are TRLWELv1: 2N output words (64 tiles), n input coefficients.
// pack_gemm_bytes: the MFMA-layout key; pack_gemm_part_bytes: the K splits' sums for `items` inputs,
// part[z][item][2N].  launch_pack_gemm takes items <= sized_for inputs with the split count of sized_for (the
// chunk size G.part holds pack_gemm_part_bytes of: a ragged last chunk on its own would take more splits and more
// scratch), leaves the sums in G.part and tells the epilogue (launch_pack_rotate_acc,
// tfhe_kernels_leveled.hip) how many splits there are and the bias every sum carries; `in` as for the
// re-encryption (rows of n + 1 words, KS_GEMM_INPUT_SLACK readable bytes past the last).
struct PackSums {
    int splits = 0;
    uint32_t bias = 0;  // CB * blocks * t * 128 * 0x01010101, as k_ks_gemm_reduce subtracts
};
size_t pack_gemm_bytes(const KParams &P, int t, int basebit);
size_t pack_gemm_part_bytes(const KParams &P, size_t items, int basebit);
hipError_t launch_pack_key_to_gemm(const KParams &P, const uint32_t *rows, uint32_t *kg, int t, int basebit,
                                   hipStream_t s);
hipError_t launch_pack_gemm(const KParams &P, int t, int basebit, const uint32_t *in, const KsGemm &G, size_t items,
                            size_t sized_for, hipStream_t s, const char **used, PackSums *sums);
// zero the k = 0 rows (never read by the reference; the kernels subtract them unconditionally)
hipError_t launch_ksk_zero_k0(const KParams &P, uint32_t *ksk, hipStream_t s);
// same for a key-switch-shaped key over n_in input coefficients (proxy re-encryption key)
hipError_t launch_key_zero_k0(const KParams &P, uint32_t *key, int n_in, int t, int basebit, hipStream_t s);
// reencryptTLWELv0 (proxy_reenc.zig:267-306): key-switch-shaped key of n*t*2^basebit
// rows in the padded device layout; in/out B TLWELv0
hipError_t launch_reencrypt(const KParams &P, int t, int basebit, const uint32_t *in, const uint32_t *key,
                            uint32_t *out, size_t B, hipStream_t s, const LaunchOpts &O = LaunchOpts(),
                            const char **used = nullptr, const KsGemm *G = nullptr);
bool reencrypt_supported(int t, int basebit);
hipError_t launch_fft_forward(const DevTables &T, const uint32_t *in, double *out, size_t B,
                              hipStream_t s);
hipError_t launch_fft_inverse(const DevTables &T, const double *in, uint32_t *out, size_t B,
                              hipStream_t s);
// b_stride: words between consecutive b polynomials (0 = one b for all items)
hipError_t launch_poly_mul(const DevTables &T, const uint32_t *a, const uint32_t *b, size_t b_stride,
                           uint32_t *out, size_t B, hipStream_t s);
hipError_t launch_external_product(const KParams &P, const DevTables &T, const double *bkd_row,
                                   const uint32_t *in, uint32_t *out, size_t B, hipStream_t s);
// reference BK layout [n][2L][2][N] -> device layout [n][2L][8][64] x {a_re,a_im,b_re,b_im}
hipError_t launch_bk_permute(const KParams &P, const double *bk_ref, double *bkd, size_t rows,
                             hipStream_t s);
// 64-bit fingerprint of bytes (a multiple of 16) at p into *out (device), async
hipError_t launch_checksum(const void *p, size_t bytes, unsigned long long *out, hipStream_t s);
hipError_t launch_absmax(const double *p, size_t count, unsigned long long *out, hipStream_t s);
// largest spectrum energy of one TRGSW row part (re^2 + im^2 over its N/2 values) over
// `rows` device-layout BK rows (n * 2L), into *out (device, double bits), async
hipError_t launch_row_energy_max(const double *bkd, size_t rows, unsigned long long *out, hipStream_t s);
hipError_t launch_bk_unpermute(const KParams &P, const double *bkd, double *bk_ref, size_t rows,
                               hipStream_t s);

// ---- launchers (tfhe_kernels_leveled.hip); asynchronous on `s` ----------
// One batch of CMUXes (trgsw.zig:260-284), device pointers: item g computes
// out[g] = cmux(src0[i0[g]], src1[i1[g]], selector sel[g]) on TRLWELv1 of 2N
// words; selectors in device layout (launch_bk_permute), 2L * 2048 doubles each.
// i0 / i1 may be NULL: item g reads slot g.  P.offset is the decomposition offset.
struct CmuxBatch {
    const double *sel_rows = nullptr;
    const uint32_t *sel = nullptr;
    const uint32_t *src0 = nullptr, *i0 = nullptr;
    const uint32_t *src1 = nullptr, *i1 = nullptr;
    uint32_t *out = nullptr;
    size_t B = 0;
};
// shared: the workgroup form (k_cmux_shared), whose 4 items g0 .. g0 + 3 (g0 a multiple of 4) must
// have sel[g0] as their selector; else one independent wavefront per item (k_cmux).
constexpr size_t CMUX_SHARED_ITEMS = 4;
hipError_t launch_cmux(const KParams &P, const DevTables &T, const CmuxBatch &b, bool shared, hipStream_t s,
                       const char **used = nullptr);
// One batch of rotations by encrypted bits (k_rotate_chain), device pointers: item g runs the h steps
// acc <- cmux(acc, X^rot[j] acc, selector sel[g h + j]) from acc = src[i_src[g]] (i_src NULL: slot g) and
// writes out[g]; rot[j] <= 2N, h >= 1; out must not overlap src.
struct RotateBatch {
    const double *sel_rows = nullptr;
    const uint32_t *sel = nullptr, *rot = nullptr;
    uint32_t h = 0;
    const uint32_t *src = nullptr, *i_src = nullptr;
    uint32_t *out = nullptr;
    size_t B = 0;
};
hipError_t launch_rotate_chain(const KParams &P, const DevTables &T, const RotateBatch &b, hipStream_t s,
                               const char **used = nullptr);
// One level of a CMUX graph (k_cmux_rot), device pointers: item q * cnt + i is the level's node i for
// query q < nq of the chunk.  nodes: cnt descriptors of 6 words {var, lo, hi, rlo, rhi, slot}; lo / hi are
// GRAPH_LEAF_REF | leaf index (into leaves) or a slot index < n_slots; slot < n_slots; rlo, rhi <= 2N;
// addr[q * k + var] is the item's selector.  Query q's slots are slots[q * n_slots ..], 2N words each; the
// host's plan (tfhe_cmux_graph_plan) keeps a level's outputs apart from every slot the level reads.
constexpr uint32_t GRAPH_LEAF_REF = 0x80000000u;
struct GraphLevel {
    const double *sel_rows = nullptr;
    const uint32_t *addr = nullptr;
    uint32_t k = 0;
    const uint32_t *nodes = nullptr;
    uint32_t cnt = 0;
    const uint32_t *leaves = nullptr;
    uint32_t *slots = nullptr;
    uint32_t n_slots = 0;
    size_t nq = 0;
};
hipError_t launch_cmux_graph_level(const KParams &P, const DevTables &T, const GraphLevel &b, hipStream_t s,
                                   const char **used = nullptr);
// out[q * R + r] = the value roots[r] names (GRAPH_LEAF_REF | leaf, or a slot of query q), 2N words each, for
// the nq queries of a chunk; roots on the device.  out must not overlap leaves or slots.
hipError_t launch_cmux_graph_roots(const uint32_t *roots, uint32_t R, const uint32_t *leaves, const uint32_t *slots,
                                   uint32_t n_slots, uint32_t *out, size_t nq, hipStream_t s);
// One level of the demultiplexer tree (k_demux / k_demux_shared), device pointers: parent g reads
// x = src[g] and writes hi = ExtProd(selector, x) to out[2g + 1] and lo = x - hi to out[2g], under
// selector sel[(g >> level) * sel_stride]: the 2^level parents of a query share the level's
// selector, sel points at that bit of the first query's address and sel_stride is the number of
// address bits per query.  out must not overlap src.
struct DemuxBatch {
    const double *sel_rows = nullptr;
    const uint32_t *sel = nullptr;
    uint32_t level = 0, sel_stride = 0;
    const uint32_t *src = nullptr;
    uint32_t *out = nullptr;
    size_t B = 0;
};
// shared: the workgroup form, for levels of at least CMUX_SHARED_ITEMS parents per query (level >= 2).
hipError_t launch_demux(const KParams &P, const DevTables &T, const DemuxBatch &b, bool shared, hipStream_t s,
                        const char **used = nullptr);
// table[i][w] += sum over q < nq of leaves[(q * trlwes + i) * 2N + w] in wrapping u32 (k_scatter_reduce),
// device pointers; leaves must not overlap table.
hipError_t launch_scatter_reduce(const uint32_t *leaves, size_t nq, size_t trlwes, uint32_t *table, hipStream_t s);
// sampleExtractIndex (trlwe.zig:146-162) at the C coefficients coef[] (device, each < N) of each
// of B TRLWELv1: B * C TLWELv1 of N + 1 words, TRLWE-major
hipError_t launch_sample_extract(const uint32_t *trlwe, const uint32_t *coef, size_t C, uint32_t *out_lv1, size_t B,
                                 hipStream_t s);
// The packing key switch's epilogue (k_pack_rotate_acc): items item0 .. item0 + M - 1 of a batch of B * C
// (item b C + c goes to coefficient coef[c] of out[b]; coef on the device, distinct, each < N) from the
// GEMM's sums of those M items.  The first item of an output TRLWE starts its sum, later ones (a later
// call's included) add to it, so a batch may go through in chunks of any size, in order.
hipError_t launch_pack_rotate_acc(const uint32_t *in, int n_in, const uint32_t *part, const PackSums &sums,
                                  const uint32_t *coef, size_t C, size_t item0, size_t M, uint32_t *out, hipStream_t s,
                                  const char **used = nullptr);

// ---- launcher (tfhe_kernels_lut.hip); asynchronous on `s` ---------------
// The linear step of B LUT-circuit nodes: dst[i] = sum_{k in [off[i], off[i+1])} coef[k] * pool[src[k]]
// + (0, ..., 0, konst[i]) in wrapping u32 arithmetic, n + 1 words each; every pointer is a device
// pointer, off has B + 1 entries that index src / coef, and the host has checked src[k] against the pool.
hipError_t launch_lut_combine(const KParams &P, const uint32_t *pool, const uint32_t *off, const uint32_t *src,
                              const int32_t *coef, const uint32_t *konst, uint32_t *dst, size_t B, hipStream_t s);
// The same with the multi-output bootstrap's rounding as each word is stored: shift[i] (device, B entries)
// is 0 for none, or s: dst word = (x + (1 << (s-1))) & ~((1 << s) - 1) in wrapping u32, 1 <= s <= 31.
hipError_t launch_lut_combine_round(const KParams &P, const uint32_t *pool, const uint32_t *off, const uint32_t *src,
                                    const int32_t *coef, const uint32_t *konst, const uint32_t *shift, uint32_t *dst,
                                    size_t B, hipStream_t s);
// The fan-out of a level of multi-output nodes: output o (of M) is sampleExtractIndex(acc[fan[2 o]], fan[2 o + 1])
// (trlwe.zig:146-162), a TLWELv1 of N + 1 = 1025 words at out_lv1 + 1025 o, ready for launch_key_switch over M
// items.  acc: the level's TRLWELv1 accumulators, 2N words per node; fan: device pairs the host has built
// (node < the level's nodes, coefficient < N).
hipError_t launch_lut_fanout_extract(const uint32_t *acc, const uint32_t *fan, uint32_t *out_lv1, size_t M,
                                     hipStream_t s, const char **used = nullptr);
// spread of the bivariate LUT bootstrap (k_lut_spread) over B TRLWELv1 of 2N words: the window sum of width
// w (1 <= w <= N) on each half, rotated by X^rot (rot <= 2N); N = 1024; out may be in.
hipError_t launch_lut_spread(const uint32_t *in, uint32_t w, uint32_t rot, uint32_t *out, size_t B, hipStream_t s,
                             const char **used = nullptr);

// ---- launcher (tfhe_kernels_lut_ext.hip); asynchronous on `s` -----------
// One batch of extended blind rotations (k_blind_rotate_ext, include/tfhe_gpu.h "Extended LUT bootstrap"),
// device pointers: item g rotates in[g] (n + 1 words) over the extended table at
// testvec + tv_sel[g] * E * 2N (tv_sel NULL: the one table at testvec), E = 2^eta components of 2N words, with
// the BK in device layout.  An entry of tv_sel with TV_SEL_EACH set names instead the one TRLWELv1 (any a) at
// tv_each + (entry & ~TV_SEL_EACH) * 2N, which all E components start from (select nodes).  all: out takes the E accumulators of every item (item-major, B * E * 2N words);
// else acc_0 only (B * 2N words).  eta is 1 or 2: hipErrorInvalidValue otherwise.  P.offset is the key's
// decomposition offset.
struct BrExtBatch {
    uint32_t eta = 0;
    const uint32_t *in = nullptr;
    const uint32_t *testvec = nullptr, *tv_sel = nullptr, *tv_each = nullptr;
    const double *bk = nullptr;
    uint32_t *out = nullptr;
    bool all = false;
    size_t B = 0;
};
hipError_t launch_blind_rotate_ext(const KParams &P, const DevTables &T, const BrExtBatch &b, hipStream_t s,
                                   const char **used = nullptr);

}  // namespace tfhe
