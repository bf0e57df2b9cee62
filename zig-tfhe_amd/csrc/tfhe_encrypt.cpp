// tfhe_encrypt.cpp — seeded key material of the C ABI (include/tfhe_gpu.h):
// TRLWE encryption and decryption, TRGSW encryption and cloud-key generation.
// Host code: every RNG draw in reference order on the host; the FFT-based
// poly_mul of each TRLWE encryption (trlwe.zig:56-61) and the TRGSWLv1FFT
// forward transforms (trgsw.zig:81-91) on the context's first device.  The
// bootstrapping key is n TRGSW encryptions like any other: keygen and
// tfhe_gpu_trgsw_encrypt_batch differ in their seed schedule and in where the
// spectra go.
#include "tfhe_gpu.h"

#include <cmath>
#include <cstring>
#include <vector>

#include "host_math.hpp"
#include "tfhe_ctx.hpp"

using namespace tfhe;

namespace tfhe {

// as = a * s (k_poly_mul) for R polynomials a and the key s: host buffers, synchronous.
static int mul_by_key(Device &d, const uint32_t *key_lv1, const uint32_t *a, uint32_t *as, size_t R) {
    const size_t N = d.P.N;
    Frame f(d);
    Io io{f, /*dev*/ false};
    int rc = io.in(key_lv1, N * sizeof(uint32_t));
    if (!rc) rc = io.in(a, R * N * sizeof(uint32_t));
    if (!rc) rc = io.out(as, R * N * sizeof(uint32_t));
    if (rc) return rc;
    HIPCHK(d, launch_poly_mul(tables(d), a, key_lv1, 0, as, R, d.stream));
    return io.finish();
}

// TRLWELv1.encryptF64 (trlwe.zig:30-64) of R rows, row r from DefaultPrng(seeds[r]):
// a uniform, b = gaussianTorus(f64ToTorus(mu), alpha) + a * s.  mu: R * N values, or
// NULL for zeros but for coefficient 0 of row r, which is mu0[r] (mu0 NULL: zero too).
// rows receives R TRLWELv1 (a then b).
static int trlwe_encrypt_rows(Device &d, const uint32_t *key_lv1, const std::vector<uint64_t> &seeds, const double *mu,
                              double alpha, uint32_t *rows, const double *mu0 = nullptr) {
    const size_t N = d.P.N, R = seeds.size();
    std::vector<uint32_t> a_only(R * N), as(R * N);
    for (size_t row = 0; row < R; row++) {
        host::Rng r(seeds[row]);
        uint32_t *a = rows + row * 2 * N, *b = a + N;
        for (size_t x = 0; x < N; x++) a[x] = r.u32();
        host::NormalDist nd(0.0, alpha);
        for (size_t x = 0; x < N; x++) {
            const double m = mu ? mu[row * N + x] : (mu0 && x == 0) ? mu0[row] : 0.0;
            b[x] = host::gaussian_torus(host::f64_to_torus(m), nd, r);
        }
        std::memcpy(a_only.data() + row * N, a, N * sizeof(uint32_t));
    }
    const int rc = mul_by_key(d, key_lv1, a_only.data(), as.data(), R);
    if (rc) return rc;
    for (size_t row = 0; row < R; row++) {
        uint32_t *b = rows + row * 2 * N + N;
        for (size_t x = 0; x < N; x++) b[x] += as[row * N + x];
    }
    return TFHE_OK;
}

// S TRGSWLv1 encryptTorus (trgsw.zig:35-71) of the plaintexts mu, TRLWE row r of the
// S * 2L from DefaultPrng(seeds[r]): 2L TRLWE encryptions of zero each, the gadget on a[0]
// of row l and b[0] of row L + l.  Then TRGSWLv1FFT.new (trgsw.zig:81-91), the ifft of every
// a and b polynomial: the S * 2L * 2 spectra are left in a slice of the caller's frame, *spectra
// (reference BK layout), queued on the device's stream.
static int trgsw_spectra(Frame &f, double **spectra, const uint32_t *key_lv1, const std::vector<uint64_t> &seeds, const uint32_t *mu,
                         double alpha) {
    Device &d = f.d;
    const size_t N = d.P.N, L = d.P.L, R = seeds.size(), S = R / (2 * L);
    std::vector<uint32_t> rows(R * 2 * N);
    int rc = trlwe_encrypt_rows(d, key_lv1, seeds, nullptr, alpha, rows.data());
    if (rc) return rc;
    for (size_t s = 0; s < S; s++)
        for (size_t l = 0; l < L; l++) {
            const uint32_t h = host::f64_to_torus(std::ldexp(1.0, -(int)((l + 1) * d.P.bgbit)));
            rows[(s * 2 * L + l) * 2 * N] += mu[s] * h;
            rows[(s * 2 * L + L + l) * 2 * N + N] += mu[s] * h;
        }
    // hipMemcpyAsync stages a pageable source before it returns (upload_plan): rows may go
    *spectra = f.take<double>(R * 2 * N);
    const uint32_t *rows_dev = f.h2d(rows.data(), rows.size() * sizeof(uint32_t));
    if (f.rc()) return f.rc();
    HIPCHK(d, launch_fft_forward(tables(d), rows_dev, *spectra, R * 2, d.stream));
    return TFHE_OK;
}

}  // namespace tfhe

extern "C" {

int tfhe_gpu_trlwe_encrypt_batch(tfhe_gpu_ctx *c, const uint32_t *key_lv1, const double *mu, double alpha, uint64_t seed0,
                                 uint32_t *out, size_t B) {
    if (!c || !key_lv1 || (B && (!mu || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) -> int {
        std::vector<uint64_t> seeds(B);
        for (size_t i = 0; i < B; i++) seeds[i] = seed0 + i;
        return trlwe_encrypt_rows(d, key_lv1, seeds, mu, alpha, out);
    });
}

int tfhe_gpu_trlwe_decrypt_bool_batch(tfhe_gpu_ctx *c, const uint32_t *key_lv1, const uint32_t *ct, uint8_t *bits,
                                      size_t B) {
    if (!c || !key_lv1 || (B && (!ct || !bits))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) -> int {
        const size_t N = d.P.N;
        std::vector<uint32_t> a_only(B * N), as(B * N);
        for (size_t i = 0; i < B; i++) std::memcpy(a_only.data() + i * N, ct + i * 2 * N, N * sizeof(uint32_t));
        const int rc = mul_by_key(d, key_lv1, a_only.data(), as.data(), B);
        if (rc) return rc;
        for (size_t i = 0; i < B; i++)
            for (size_t x = 0; x < N; x++) bits[i * N + x] = (int32_t)(ct[i * 2 * N + N + x] - as[i * N + x]) >= 0;
        return TFHE_OK;
    });
}

// The packing key (include/tfhe_gpu.h): row idx = base t i + base j + k, k >= 1, encrypts the polynomial
// whose coefficient 0 is k key_lv0[i] / 2^((j+1) basebit) (key.zig:164) from DefaultPrng(seed0 + idx); the
// k = 0 rows are zero.  The rows to encrypt go through trlwe_encrypt_rows in runs of PACK_GEN_ROWS, each with
// its coefficient-0 plaintext only.
int tfhe_gpu_packing_key_gen(tfhe_gpu_ctx *c, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha,
                             uint32_t basebit, uint32_t t, uint64_t seed0, uint32_t *rows) {
    if (!c || !key_lv0 || !key_lv1 || !rows) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (!pack_shape_ok(basebit, t))
        return fail(c, TFHE_ERR_INVALID, "packing key: (basebit, t) has no GEMM form (basebit 2: t 7..9, basebit 5: t 2..3)");
    return on_device0(c, [&](Device &d) -> int {
        constexpr size_t PACK_GEN_ROWS = 2048;
        const size_t N = d.P.N, n = d.P.n, base = (size_t)1 << basebit, total = n * t * base;
        std::memset(rows, 0, total * 2 * N * sizeof(uint32_t));
        std::vector<uint64_t> seeds;
        std::vector<double> mu0;
        std::vector<size_t> at;
        std::vector<uint32_t> run(PACK_GEN_ROWS * 2 * N);
        auto flush = [&]() -> int {
            if (seeds.empty()) return TFHE_OK;
            const int rc = trlwe_encrypt_rows(d, key_lv1, seeds, nullptr, alpha, run.data(), mu0.data());
            for (size_t r = 0; !rc && r < at.size(); r++)
                std::memcpy(rows + at[r] * 2 * N, run.data() + r * 2 * N, 2 * N * sizeof(uint32_t));
            seeds.clear();
            mu0.clear();
            at.clear();
            return rc;
        };
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j < t; j++)
                for (size_t k = 1; k < base; k++) {
                    const size_t idx = base * t * i + base * j + k;
                    seeds.push_back(seed0 + idx);
                    mu0.push_back(((double)k * (double)key_lv0[i]) / (double)(1u << ((j + 1) * basebit)));
                    at.push_back(idx);
                    if (seeds.size() == PACK_GEN_ROWS)
                        if (const int rc = flush()) return rc;
                }
        return flush();
    });
}

// TRGSW s from DefaultPrng(seed0 + s): one next() per TRLWE row.
int tfhe_gpu_trgsw_encrypt_batch(tfhe_gpu_ctx *c, const uint32_t *key_lv1, const uint32_t *mu, double alpha,
                                 uint64_t seed0, double *out_fft, size_t S) {
    if (!c || !key_lv1 || (S && (!mu || !out_fft))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (S == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) -> int {
        const size_t L = d.P.L, R = S * 2 * L;
        std::vector<uint64_t> seeds(R);
        for (size_t s = 0; s < S; s++) {
            host::Rng master(seed0 + s);
            for (size_t r = 0; r < 2 * L; r++) seeds[s * 2 * L + r] = master.next();
        }
        Frame f(d);
        double *spectra = nullptr;
        const int rc = trgsw_spectra(f, &spectra, key_lv1, seeds, mu, alpha);
        return rc ? rc : d2h_sync(d, out_fft, spectra, R * 2 * d.P.N * sizeof(double));
    });
}

// SecretKey.new + CloudKey.new, seeded: one master generator (cloud_seed) hands out every
// KSK row's seed, then every BK row's.
int tfhe_gpu_keygen(tfhe_gpu_ctx *c, uint64_t secret_seed, uint64_t cloud_seed, uint32_t *key_lv0,
                    uint32_t *key_lv1, double *bsk_out, uint32_t *ksk_out) {
    if (!c || !key_lv0 || !key_lv1) return fail(c, TFHE_ERR_INVALID, "null argument");
    const int rc = on_device0(c, [&](Device &d) -> int {
        const tfhe_params &p = d.P;
        const uint32_t N = p.N, n = p.n, T = p.iks_t, base = 1u << p.basebit;
        tfhe_secret_key_new(&p, secret_seed, key_lv0, key_lv1);
        host::Rng master(cloud_seed);
        // genKeySwitchingKey (key.zig:148-172): k = 0 rows are zeroed
        std::vector<uint32_t> ksk(ksk_words(p), 0u);
        for (uint32_t i = 0; i < N; i++)
            for (uint32_t j = 0; j < T; j++)
                for (uint32_t k = 1; k < base; k++) {
                    size_t idx = (size_t)base * T * i + (size_t)base * j + k;
                    uint32_t shift = (j + 1) * p.basebit;
                    double pv = ((double)k * (double)key_lv1[i]) / (double)(1u << shift);
                    tlwe_encrypt(n, pv, p.alpha_ksk, key_lv0, master.next(), ksk.data() + idx * (n + 1));
                }
        // genBootstrappingKey (key.zig:175-212): per i, TRGSW encryptTorus of key_lv0[i]
        const size_t R = bk_rows(p);  // n*2L TRLWE rows
        std::vector<uint64_t> seeds(R);
        for (uint64_t &s : seeds) s = master.next();
        Frame f(d);  // the BK spectra, until the stream has been waited for
        double *spectra = nullptr;
        int rc = trgsw_spectra(f, &spectra, key_lv1, seeds, key_lv0, p.alpha_bsk);
        if (rc) return rc;
        std::vector<uint32_t> tv(2 * N);
        for (uint32_t x = 0; x < N; x++) {  // genTestvec (key.zig:134-145)
            tv[x] = 0;
            tv[N + x] = host::f64_to_torus(0.125);
        }
        rc = set_key_common(d, decomposition_offset(p), tv.data(), tv.data() + N);
        if (rc) return rc;
        HIPCHK(d, launch_bk_permute(d.K, spectra, d.d_bk, R, d.stream));
        rc = upload_ksk(d, ksk.data());
        if (rc) return rc;
        if (bsk_out)
            HIPCHK(d, hipMemcpyAsync(bsk_out, spectra, R * 2 * N * sizeof(double), hipMemcpyDeviceToHost, d.stream));
        HIPCHK(d, hipStreamSynchronize(d.stream));
        if (ksk_out) std::memcpy(ksk_out, ksk.data(), ksk.size() * sizeof(uint32_t));
        return key_loaded(d, /*from_keygen*/ true);
    });
    return rc ? rc : broadcast_key(c);
}

}  // extern "C"
