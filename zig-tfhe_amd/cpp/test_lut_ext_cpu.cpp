// Stand-alone test of the extended LUT bootstrap's host half (csrc/tfhe_cpu.cpp): the extended
// test vector's components (tfhe_lut_generate_ext), X^a on E components (tfhe_lut_ext_rotate)
// against the rotation of the interleaved polynomial of degree N * E, and the mod switch to
// 2N * E positions (tfhe_lut_ext_mod_switch).  Links tfhe_cpu.o only — no HIP, no
// libtfhe_gpu.so — and builds and runs under the host sanitizers too (make cpu-check).
// Exit status 0 = all passed.
#include "tfhe_cpu.hpp"

#include <cstdio>
#include <vector>

namespace {
int failures = 0;
void expect(bool ok, const char *test, const char *what) {
    if (!ok) {
        std::printf("FAIL %s: %s\n", test, what);
        failures++;
    }
}
using U = std::vector<uint32_t>;
// UINT4 (n = 820) as far as these host entries read it
tfhe_params uint4() {
    tfhe_params p{};
    p.n = 820, p.N = 1024, p.nbit = 10, p.L = 1, p.bgbit = 22, p.basebit = 5, p.iks_t = 3;
    return p;
}
uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

// generateLookupTableAssign's b half (lut/generator.zig:85-135) at degree D, restated: values[x] over
// [divRound(x D, m), divRound((x + 1) D, m)), rotated left by divRound(D, 2m), the wrapped tail negated
U generator_b(size_t D, size_t m, const U &values) {
    auto div_round = [](size_t a, size_t b) { return (a + b / 2) / b; };
    U raw(D, 0u), b(D);
    for (size_t x = 0; x < m; x++)
        for (size_t i = div_round(x * D, m); i < div_round((x + 1) * D, m); i++) raw[i] = values[x];
    const size_t off = div_round(D, 2 * m);
    for (size_t i = 0; i < D; i++) b[i] = i < D - off ? raw[(i + off) % D] : 0u - raw[(i + off) % D];
    return b;
}

// X^a on one polynomial of degree D (polyMulWithXK, trgsw.zig:442-466), 0 <= a <= 2D
U mul_xk(const U &x, size_t a) {
    const size_t D = x.size();
    U y(D);
    for (size_t i = 0; i < D; i++) {
        const size_t at = (i + a) % (2 * D);
        y[at % D] = at < D ? x[i] : 0u - x[i];
    }
    return y;
}
}  // namespace

int main() {
    const tfhe_params p = uint4();
    const size_t N = p.N;
    {
        const char *T = "generate_ext";
        for (uint32_t eta = 0; eta <= TFHE_LUT_EXT_MAX_LOG; eta++) {
            const size_t E = (size_t)1 << eta;
            for (uint32_t m : {2u, 16u, 32u, 64u, 128u}) {
                U f(m), enc(m), out(E * 2 * N, 7u);
                for (uint32_t x = 0; x < m; x++) {
                    f[x] = (7 * x + 3) % m;
                    // Encoder.new(m).encode: f / (2m) of the torus, exact for a power of two
                    enc[x] = (uint32_t)(((uint64_t)f[x] << 32) / (2 * m));
                }
                expect(tfhe_lut_generate_ext(&p, eta, m, f.data(), out.data()) == TFHE_OK, T, "status");
                const U b = generator_b(N * E, m, enc);
                bool a_zero = true, split = true;
                for (size_t j = 0; j < E; j++)
                    for (size_t k = 0; k < N; k++) {
                        a_zero = a_zero && out[j * 2 * N + k] == 0;
                        split = split && out[j * 2 * N + N + k] == b[k * E + j];
                    }
                expect(a_zero, T, "a = 0 in every component");
                expect(split, T, "tv_j.b[k] = TV.b[k E + j]");
                if (eta == 0) {
                    U tv(2 * N);
                    expect(tfhe_lut_generate(&p, m, f.data(), tv.data()) == TFHE_OK && tv == out, T, "eta = 0 is tfhe_lut_generate");
                }
            }
        }
        U f(4, 1u), out(8 * 2 * N);
        expect(tfhe_lut_generate_ext(&p, 3, 4, f.data(), out.data()) == TFHE_ERR_INVALID, T, "eta = 3 is refused");
        expect(tfhe_lut_generate_ext(&p, 1, 0, f.data(), out.data()) == TFHE_ERR_INVALID, T, "m = 0 is refused");
        expect(tfhe_lut_generate_ext(&p, 1, 4, nullptr, out.data()) == TFHE_ERR_INVALID, T, "null table");
    }
    {
        const char *T = "ext_rotate";
        uint32_t s = 11;
        for (uint32_t eta = 0; eta <= TFHE_LUT_EXT_MAX_LOG; eta++) {
            const size_t E = (size_t)1 << eta, D = N * E;
            U in(E * 2 * N), out(E * 2 * N);
            for (auto &v : in) v = lcg(s);
            U half[2] = {U(D), U(D)};  // the interleaved polynomials: coefficient k E + j = component j's k
            for (size_t j = 0; j < E; j++)
                for (size_t h = 0; h < 2; h++)
                    for (size_t k = 0; k < N; k++) half[h][k * E + j] = in[j * 2 * N + h * N + k];
            std::vector<size_t> as = {0, 1, E - 1, E, D - 1, D, D + 1, 2 * D - 1, 2 * D};
            for (int r = 0; r < 8; r++) as.push_back(lcg(s) % (2 * D + 1));
            for (size_t a : as) {
                expect(tfhe_lut_ext_rotate(&p, eta, in.data(), (uint32_t)a, out.data()) == TFHE_OK, T, "status");
                bool same = true;
                for (size_t h = 0; h < 2; h++) {
                    const U want = mul_xk(half[h], a);
                    for (size_t j = 0; j < E; j++)
                        for (size_t k = 0; k < N; k++) same = same && out[j * 2 * N + h * N + k] == want[k * E + j];
                }
                expect(same, T, "the rotation of the interleaved polynomial, de-interleaved");
            }
            expect(tfhe_lut_ext_rotate(&p, eta, in.data(), (uint32_t)(2 * D), out.data()) == TFHE_OK && out == in, T,
                   "a = 2N E is the identity");
            expect(tfhe_lut_ext_rotate(&p, eta, in.data(), (uint32_t)(2 * D + 1), out.data()) == TFHE_ERR_INVALID, T,
                   "a > 2N E is refused");
            expect(tfhe_lut_ext_rotate(&p, eta, in.data(), 0, in.data()) == TFHE_ERR_INVALID, T, "in == out is refused");
        }
        U in(8 * 2 * N), out(8 * 2 * N);
        expect(tfhe_lut_ext_rotate(&p, 3, in.data(), 0, out.data()) == TFHE_ERR_INVALID, T, "eta = 3 is refused");
    }
    {
        const char *T = "mod_switch";
        for (uint32_t eta = 0; eta <= TFHE_LUT_EXT_MAX_LOG; eta++) {
            const uint32_t sh = 21 - eta, top = 2048u << eta;
            expect(tfhe_lut_ext_mod_switch(&p, eta, 0) == 0, T, "0 -> 0");
            expect(tfhe_lut_ext_mod_switch(&p, eta, 0xFFFFFFFFu) == (int)top, T, "0xFFFFFFFF -> 2N E (the add is 64 bits wide)");
            expect(tfhe_lut_ext_mod_switch(&p, eta, (1u << (sh - 1)) - 1) == 0, T, "just below half rounds down");
            expect(tfhe_lut_ext_mod_switch(&p, eta, 1u << (sh - 1)) == 1, T, "half rounds up");
            expect(tfhe_lut_ext_mod_switch(&p, eta, 0x80000000u) == (int)(top / 2), T, "1/2 -> N E");
        }
        expect(tfhe_lut_ext_mod_switch(&p, 3, 0) == TFHE_ERR_INVALID, T, "eta = 3 is refused");
        expect(tfhe_lut_ext_mod_switch(nullptr, 1, 0) == TFHE_ERR_INVALID, T, "null params");
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
