// tfhe_kernels_lut.hip — the linear step of a LUT circuit node on the device:
// a small integer combination of TLWELv0 ciphertexts (TLWELv0.add / neg /
// addMul / subMul, tlwe.zig:120-240) in front of the programmable bootstrap,
// and the two ends of a multi-output node: the rounding of the combined words
// and the fan-out extraction of its accumulator's first coefficients; and the
// spread of the bivariate bootstrap: coefficient slots -> a test vector.
// Its own unit, like tfhe_kernels_leveled.hip: the bootstrap kernels' objects
// (tfhe_kernels.o, tfhe_kernels_whole.o), which tfhe_gpu_build_id() hashes, do
// not change with it.  Integer arithmetic only.
#include "tfhe_internal.hpp"

namespace tfhe {

constexpr int LUT_COMBINE_THREADS = 256;

// Node i of the launch (one workgroup):
//   dst[i] = sum over k in [off[i], off[i+1]) of coef[k] * pool[src[k]]  +  (0, ..., 0, konst[i])
// in wrapping u32 arithmetic on all n1 = n + 1 words (coef: int32 as a Torus word
// in two's complement), so the order of the terms does not matter.  Lanes stride
// the n1 words (821 at UINT4, 701 at the 128-bit set: the loop bound is n1, not a
// multiple of the wave).  A node without terms is the trivial ciphertext of
// konst[i].  dst is dense, n1 words per node, and never aliases pool's read slots
// (the host writes a staging buffer).  off / src / coef / konst are device copies
// of descriptors the host has checked: src[k] < the pool's size.
__global__ __launch_bounds__(LUT_COMBINE_THREADS) void k_lut_combine(
    const uint32_t *__restrict__ pool, const uint32_t *__restrict__ off, const uint32_t *__restrict__ src,
    const int32_t *__restrict__ coef, const uint32_t *__restrict__ konst, uint32_t *__restrict__ dst, int n1) {
    const size_t i = blockIdx.x;
    const uint32_t k0 = off[i], k1 = off[i + 1];
    const uint32_t kb = konst[i];
    uint32_t *y = dst + i * (size_t)n1;
    for (int j = threadIdx.x; j < n1; j += LUT_COMBINE_THREADS) {
        uint32_t acc = j == n1 - 1 ? kb : 0u;
        for (uint32_t k = k0; k < k1; k++) acc += (uint32_t)coef[k] * pool[(size_t)src[k] * n1 + j];
        y[j] = acc;
    }
}

// k_lut_combine with the multi-output bootstrap's round_theta on each word as it is stored, so
// the rounded x costs no extra pass: shift[i] = 0 stores the word as is, s in [1, 31] stores
// (w + (1 << (s-1))) & ~((1 << s) - 1) in wrapping u32 (0xFFFFFFFF goes to 0).  Nodes of
// different theta share a launch.  A kernel of its own: calls without a theta launch
// k_lut_combine as before.
__global__ __launch_bounds__(LUT_COMBINE_THREADS) void k_lut_combine_round(
    const uint32_t *__restrict__ pool, const uint32_t *__restrict__ off, const uint32_t *__restrict__ src,
    const int32_t *__restrict__ coef, const uint32_t *__restrict__ konst, const uint32_t *__restrict__ shift,
    uint32_t *__restrict__ dst, int n1) {
    const size_t i = blockIdx.x;
    const uint32_t k0 = off[i], k1 = off[i + 1];
    const uint32_t kb = konst[i], sh = shift[i];
    const uint32_t half = sh ? 1u << (sh - 1) : 0u, mask = sh ? ~((1u << sh) - 1u) : ~0u;
    uint32_t *y = dst + i * (size_t)n1;
    for (int j = threadIdx.x; j < n1; j += LUT_COMBINE_THREADS) {
        uint32_t acc = j == n1 - 1 ? kb : 0u;
        for (uint32_t k = k0; k < k1; k++) acc += (uint32_t)coef[k] * pool[(size_t)src[k] * n1 + j];
        y[j] = (acc + half) & mask;
    }
}

// sampleExtractIndex(acc[node], k) (trlwe.zig:146-162) for one output per workgroup, N = 1024:
//   p[i] = a[k - i] (i <= k), -a[N + k - i] (i > k), p[N] = b[k]
// with (node, k) = fan[2 o], fan[2 o + 1].  Index arithmetic and negations only.  Thread t of a
// pass writes word i = t + 256 * pass, so a wave stores 64 consecutive words, and reads word
// (k - i) mod N: the 64 consecutive words below (k - i0) mod N in descending lane order (the span
// wraps once per output, inside one wave for k < 64), so both sides stay whole 256-byte runs per
// wave and every word of a[] is read once.  The output's stride is 1025 words, so 4-byte
// accesses are the widest that are aligned for every output.
constexpr int LUT_FANOUT_THREADS = 256;
__global__ __launch_bounds__(LUT_FANOUT_THREADS) void k_lut_fanout_extract(const uint32_t *__restrict__ acc,
                                                                           const uint32_t *__restrict__ fan,
                                                                           uint32_t *__restrict__ out) {
    const size_t o = blockIdx.x;
    const uint32_t *x = acc + (size_t)fan[2 * o] * 2048;
    const uint32_t k = fan[2 * o + 1] & 1023u;
    uint32_t *p = out + o * 1025;
    for (uint32_t i = threadIdx.x; i < 1024; i += LUT_FANOUT_THREADS) {
        const uint32_t v = x[(k - i) & 1023u];
        p[i] = i <= k ? v : 0u - v;
    }
    if (threadIdx.x == 0) p[1024] = x[1024 + k];
}

// spread of the bivariate LUT bootstrap (include/tfhe_gpu.h) on one half (N = 1024 words) per workgroup:
//   S[i] = sum_{j<w} +-x[(i - j) mod N], negated where i - j wraps (the sum of polyMulWithXK(x, j)), and
//   y = polyMulWithXK(S, rot)  (trgsw.zig:442-466).
// With the inclusive prefix sums E of x and T = E[N-1], in wrapping u32 (so the differences are exact),
//   S[i] = E[i] - E[i - w] for i >= w, and E[i] - (T - E[N + i - w]) for i < w
// (the second form at i = w - 1 is E[i]): two LDS reads per output whatever w is.  The half is staged in LDS
// by 4-byte loads (a caller's TRLWE need not be 16-byte aligned); thread t then owns words 4t .. 4t+3: its
// own running sums, a shuffle scan of the 64 lane totals, the 4 wave totals through LDS, and E back over
// the same words (each thread overwrites only what it alone read).  Output word o reads S at
// (o - rot) mod N, negated when the rotation wraps an odd number of times, so a wave stores 64 consecutive
// words and reads 64 consecutive (mod N) LDS words twice.  Every read of x comes before the barrier in front
// of the stores: out may be in.  1 <= w <= N and rot <= 2N are the host's checks; N + i - w stays in [i, N).
constexpr int LUT_SPREAD_THREADS = 256;
__global__ __launch_bounds__(LUT_SPREAD_THREADS) void k_lut_spread(const uint32_t *in, uint32_t *out,
                                                                   uint32_t w, uint32_t rot) {
    __shared__ __attribute__((aligned(16))) uint32_t E[1024];
    __shared__ uint32_t wave_total[LUT_SPREAD_THREADS / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t *x = in + (size_t)blockIdx.x * 1024;
    uint32_t *y = out + (size_t)blockIdx.x * 1024;
    for (uint32_t i = t; i < 1024; i += LUT_SPREAD_THREADS) E[i] = x[i];
    __syncthreads();
    uint4 v = reinterpret_cast<const uint4 *>(E)[t];
    v.y += v.x, v.z += v.y, v.w += v.z;
    uint32_t inc = v.w;  // inclusive scan of the lanes' totals
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += up;
    }
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    uint32_t base = inc - v.w;
    for (uint32_t k = 0; k < wave; k++) base += wave_total[k];
    v.x += base, v.y += base, v.z += base, v.w += base;
    reinterpret_cast<uint4 *>(E)[t] = v;
    __syncthreads();
    const uint32_t T = E[1023];
    for (uint32_t o = t; o < 1024; o += LUT_SPREAD_THREADS) {
        const uint32_t q = o + 2048u - rot, i = q & 1023u;  // q in [0, 3N): wraps = 2 - q / N
        const uint32_t s = i >= w ? E[i] - E[i - w] : E[i] - (T - E[1024 + i - w]);
        y[o] = (q >> 10) & 1u ? 0u - s : s;
    }
}

hipError_t launch_lut_spread(const uint32_t *in, uint32_t w, uint32_t rot, uint32_t *out, size_t B, hipStream_t s,
                             const char **used) {
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lut_spread, dim3((unsigned)(2 * B)), dim3(LUT_SPREAD_THREADS), 0, s, in, out, w, rot);
    if (used) *used = "k_lut_spread";
    return hipGetLastError();
}

hipError_t launch_lut_combine(const KParams &P, const uint32_t *pool, const uint32_t *off, const uint32_t *src,
                              const int32_t *coef, const uint32_t *konst, uint32_t *dst, size_t B, hipStream_t s) {
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lut_combine, dim3((unsigned)B), dim3(LUT_COMBINE_THREADS), 0, s, pool, off, src, coef, konst,
                       dst, P.n + 1);
    return hipGetLastError();
}

hipError_t launch_lut_combine_round(const KParams &P, const uint32_t *pool, const uint32_t *off, const uint32_t *src,
                                    const int32_t *coef, const uint32_t *konst, const uint32_t *shift, uint32_t *dst,
                                    size_t B, hipStream_t s) {
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lut_combine_round, dim3((unsigned)B), dim3(LUT_COMBINE_THREADS), 0, s, pool, off, src, coef,
                       konst, shift, dst, P.n + 1);
    return hipGetLastError();
}

hipError_t launch_lut_fanout_extract(const uint32_t *acc, const uint32_t *fan, uint32_t *out_lv1, size_t M,
                                     hipStream_t s, const char **used) {
    if (M == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lut_fanout_extract, dim3((unsigned)M), dim3(LUT_FANOUT_THREADS), 0, s, acc, fan, out_lv1);
    if (used) *used = "k_lut_fanout_extract";
    return hipGetLastError();
}

}  // namespace tfhe
