// tfhe_pack.cpp — the packing key switch of the C ABI (include/tfhe_gpu.h): the resident
// key, its load, and the pack call with its chunking.  Host code; the arithmetic is the
// one-hot GEMM of the key switch (k_key_switch_gemm, tfhe_kernels.hip) 64 tiles wide and
// the epilogue k_pack_rotate_acc (tfhe_kernels_leveled.hip); key generation is in
// tfhe_encrypt.cpp, the host-only definition (tfhe_pack_tlwe) in tfhe_cpu.cpp.  Runs on
// the context's first device and needs no cloud key.
#include "tfhe_gpu.h"

#include <algorithm>
#include <memory>

#include "tfhe_ctx.hpp"

using namespace tfhe;

namespace tfhe {

// Items per chunk: as many as keep the K splits' sums (pack_gemm_part_bytes; fewer items take
// more splits, at most 4 of 2N words each) within the scratch bound, and at least one.  Every
// chunk of the call, a shorter last one included, runs with this chunk size's split count
// (launch_pack_gemm), so none needs more scratch than the first.
size_t pack_chunk_items(const Device &d, size_t items, int basebit) {
    const size_t cap = (size_t)d.pack_scratch_mb << 20;
    size_t chunk = std::min(items, std::max<size_t>(1, cap / (2 * d.P.N * sizeof(uint32_t))));
    while (chunk > 1 && pack_gemm_part_bytes(d.K, chunk, basebit) > cap) chunk = (chunk + 1) / 2;
    return chunk;
}

// The launches of a pack over device buffers (tfhe_ctx.hpp): per chunk the GEMM, then the epilogue.
int pack_launch(Device &d, const tfhe_gpu_packing_key &key, const uint32_t *x0, const uint32_t *coef_dev, size_t C,
                uint32_t *out, size_t B) {
    const size_t items = B * C, w = tlwe0_words(d.P);
    const int basebit = (int)key.basebit, t = (int)key.t;
    const size_t chunk = pack_chunk_items(d, items, basebit);
    Frame f(d);  // the K splits' sums, every chunk's in the same slice
    KsGemm G;
    G.kg = key.key_gemm;
    G.part = static_cast<uint32_t *>(f.bytes(pack_gemm_part_bytes(d.K, chunk, basebit)));
    if (f.rc()) return f.rc();
    d.last_br = d.last_ks = "";
    for (size_t item0 = 0; item0 < items; item0 += chunk) {
        const size_t M = std::min(chunk, items - item0);
        const uint32_t *x = x0 + item0 * w;
        PackSums sums;
        // last_kernels: the GEMM instantiation, then the epilogue
        HIPCHK(d, launch_pack_gemm(d.K, t, basebit, x, G, M, chunk, d.stream, &d.last_br, &sums));
        HIPCHK(d, launch_pack_rotate_acc(x, (int)d.P.n, G.part, sums, coef_dev, C, item0, M, out, d.stream, &d.last_ks));
    }
    return TFHE_OK;
}

// in: B * C TLWELv0, out: B TRLWELv1; host (dev = false: staged, synchronous) or device.  The
// inputs always go through the library's own staging, which has the slack the GEMM's
// whole-block reads need past the last row.
static int pack_on(Device &d, const tfhe_gpu_packing_key &key, const uint32_t *in, const uint32_t *coef, size_t C,
                   uint32_t *out, size_t B, bool dev) {
    const size_t in_bytes = B * C * tlwe0_words(d.P) * sizeof(uint32_t);
    Frame f(d);
    Io io{f, dev};
    // the last block of 8 coefficients may reach 6 words past the last row's n + 1 (n = 8q + 1)
    uint32_t *x = f.ks_input<uint32_t>(in_bytes / sizeof(uint32_t), /*pack*/ true);
    DescBlob blob;
    blob.add(coef, C);
    const uint32_t *coef_dev = blob.upload(f);
    int rc = io.out(out, B * 2 * d.P.N * sizeof(uint32_t));
    if (rc) return rc;
    if (dev) HIPCHK(d, hipMemcpyAsync(x, in, in_bytes, hipMemcpyDeviceToDevice, d.stream));
    else if ((rc = h2d_copy(d, x, in, in_bytes))) return rc;
    rc = pack_launch(d, key, x, coef_dev, C, out, B);
    return rc ? rc : io.finish();
}

}  // namespace tfhe

extern "C" {

int tfhe_gpu_packing_key_load(tfhe_gpu_ctx *c, const uint32_t *rows, size_t len, uint32_t basebit, uint32_t t,
                              tfhe_gpu_packing_key **out) {
    if (out) *out = nullptr;
    if (!c || !rows || !out) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (!pack_shape_ok(basebit, t) || !ks_gemm_supported((int)t, (int)basebit))
        return fail(c, TFHE_ERR_INVALID, "packing key: (basebit, t) has no GEMM form (basebit 2: t 7..9, basebit 5: t 2..3)");
    if (len != pack_key_words(c->P, basebit, t))
        return fail(c, TFHE_ERR_INVALID, "packing key: len != n * t * 2^basebit * 2N words");
    std::unique_ptr<tfhe_gpu_packing_key> key(new tfhe_gpu_packing_key);
    key->ctx = c;
    key->P = c->P;
    key->basebit = basebit;
    key->t = t;
    const int rc = on_device0(c, [&](Device &d) -> int {
        // The u32 rows are staged in HBM by a plain copy from the caller's pageable buffer (not through the
        // pinned staging arena, which a key of hundreds of MB would only grow: ADVICE.md) and freed on return.
        DevPtr<uint32_t> staged;
        if (hipMalloc((void **)staged.make(d.device), len * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc((void **)key->key_gemm.make(d.device), pack_gemm_bytes(d.K, (int)t, (int)basebit)) != hipSuccess)
            return fail(d, TFHE_ERR_OOM, "hipMalloc(packing key)");
        HIPCHK(d, hipMemcpyAsync(staged, rows, len * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
        HIPCHK(d, launch_pack_key_to_gemm(d.K, staged, key->key_gemm, (int)t, (int)basebit, d.stream));
        HIPCHK(d, hipStreamSynchronize(d.stream));
        return TFHE_OK;
    });
    if (rc) return rc;
    *out = key.release();
    return TFHE_OK;
}

void tfhe_gpu_packing_key_destroy(tfhe_gpu_packing_key *key) { delete key; }

static int pack_entry(tfhe_gpu_ctx *c, const tfhe_gpu_packing_key *key, const uint32_t *in, const uint32_t *coef, size_t C,
                      uint32_t *out, size_t B, bool dev) {
    if (!c || !key || !coef || (B && (!in || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (dev && is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (const int rc = set_mismatch(c, key, "packing key")) return rc;
    if (const char *why = check_pack_args(c->P, key->basebit, key->t, coef, C)) return fail(c, TFHE_ERR_INVALID, why);
    if (B > 0xFFFFFFFFull / C) return fail(c, TFHE_ERR_INVALID, "pack: too many items");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) { return pack_on(d, *key, in, coef, C, out, B, dev); });
}

int tfhe_gpu_pack_tlwe_batch(tfhe_gpu_ctx *c, const tfhe_gpu_packing_key *key, const uint32_t *in, const uint32_t *coef,
                             size_t C, uint32_t *out_trlwe, size_t B) {
    return pack_entry(c, key, in, coef, C, out_trlwe, B, false);
}

int tfhe_gpu_pack_tlwe_dev(tfhe_gpu_ctx *c, const tfhe_gpu_packing_key *key, const uint32_t *in_dev, const uint32_t *coef,
                           size_t C, uint32_t *out_dev, size_t B) {
    return pack_entry(c, key, in_dev, coef, C, out_dev, B, true);
}

}  // extern "C"
