// tfhe_kernels_lut.hip — the linear step of a LUT circuit node on the device:
// a small integer combination of TLWELv0 ciphertexts (TLWELv0.add / neg /
// addMul / subMul, tlwe.zig:120-240) in front of the programmable bootstrap.
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

hipError_t launch_lut_combine(const KParams &P, const uint32_t *pool, const uint32_t *off, const uint32_t *src,
                              const int32_t *coef, const uint32_t *konst, uint32_t *dst, size_t B, hipStream_t s) {
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lut_combine, dim3((unsigned)B), dim3(LUT_COMBINE_THREADS), 0, s, pool, off, src, coef, konst,
                       dst, P.n + 1);
    return hipGetLastError();
}

}  // namespace tfhe
