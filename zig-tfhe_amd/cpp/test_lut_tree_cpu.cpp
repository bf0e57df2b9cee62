// Stand-alone test of the bivariate LUT bootstrap's host half (csrc/tfhe_cpu.cpp): tfhe_lut_spread
// against a restatement through polyMulWithXK, the generator's table from the trivial slot TRLWE for
// m = 4, 16, 32, the identity, in-place use and the argument checks.  Links tfhe_cpu.o only — no HIP,
// no libtfhe_gpu.so — and builds and runs under the host sanitizers too (make cpu-check).
// Exit status 0 = all passed.
#include "tfhe_cpu.hpp"

#include <algorithm>
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
// polyMulWithXK (trgsw.zig:442-466), 0 <= k <= 2N
U mulxk(const U &a, size_t k) {
    const size_t N = a.size();
    U r(N);
    if (k < N) {
        for (size_t i = 0; i < N - k; i++) r[i + k] = a[i];
        for (size_t i = N - k; i < N; i++) r[i + k - N] = 0u - a[i];
    } else {
        for (size_t i = 0; i < 2 * N - k; i++) r[i + k - N] = 0u - a[i];
        for (size_t i = 2 * N - k; i < N; i++) r[i - (2 * N - k)] = a[i];
    }
    return r;
}
}  // namespace

int main() {
    const tfhe_params p = uint4();
    const size_t N = p.N;
    {
        const char *T = "spread";
        uint32_t s = 11;
        for (uint32_t w : {1u, 2u, 64u, 256u, 1024u})
            for (uint32_t rot : {0u, 1u, 1024u, 2048u - 32u, 2048u})
                for (size_t B : {(size_t)1, (size_t)3}) {
                    U in(B * 2 * N), out(B * 2 * N, 1), want(B * 2 * N);
                    for (auto &v : in) v = lcg(s);
                    for (size_t h = 0; h < 2 * B; h++) {
                        const U x(in.begin() + h * N, in.begin() + (h + 1) * N);
                        U S(N, 0u);
                        for (uint32_t j = 0; j < w; j++) {
                            const U r = mulxk(x, j);
                            for (size_t i = 0; i < N; i++) S[i] += r[i];
                        }
                        const U y = mulxk(S, rot);
                        std::copy(y.begin(), y.end(), want.begin() + h * N);
                    }
                    expect(tfhe_lut_spread(&p, in.data(), w, rot, out.data(), B) == TFHE_OK, T, "status");
                    expect(out == want, T, "differs from the restatement");
                    if (w == 1 && (rot == 0 || rot == 2048)) expect(out == in, T, "w = 1 with X^0 or X^2N is the identity");
                    U same = in;
                    expect(tfhe_lut_spread(&p, same.data(), w, rot, same.data(), B) == TFHE_OK && same == want, T, "in place");
                }
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "generator";
        for (uint32_t m : {4u, 16u, 32u}) {
            const uint32_t w = (uint32_t)N / m, off = (uint32_t)N / (2 * m);
            U f(m), slots(2 * N, 0u), tv(2 * N), out(2 * N, 1);
            for (uint32_t x = 0; x < m; x++) f[x] = (5 * x + 3) % m;
            expect(tfhe_lut_generate(&p, m, f.data(), tv.data()) == TFHE_OK, T, "lut_generate");
            // Encoder.new(m).encode(v) = v / (2m) of the torus, exact for these m
            for (uint32_t x = 0; x < m; x++) slots[N + x * w] = f[x] * (uint32_t)(0x100000000ull / (2 * m));
            expect(tfhe_lut_spread(&p, slots.data(), w, 2 * (uint32_t)N - off, out.data(), 1) == TFHE_OK && out == tv, T,
                   "spread of the slots is the generator's table");
        }
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "arguments";
        U in(2 * N, 7), out(2 * N);
        expect(tfhe_lut_spread(&p, in.data(), 0, 0, out.data(), 1) == TFHE_ERR_INVALID, T, "w = 0");
        expect(tfhe_lut_spread(&p, in.data(), 1025, 0, out.data(), 1) == TFHE_ERR_INVALID, T, "w > N");
        expect(tfhe_lut_spread(&p, in.data(), 4, 2049, out.data(), 1) == TFHE_ERR_INVALID, T, "rot > 2N");
        expect(tfhe_lut_spread(nullptr, in.data(), 4, 0, out.data(), 1) == TFHE_ERR_INVALID, T, "null params");
        expect(tfhe_lut_spread(&p, nullptr, 4, 0, out.data(), 1) == TFHE_ERR_INVALID, T, "null input");
        expect(tfhe_lut_spread(&p, in.data(), 4, 0, nullptr, 1) == TFHE_ERR_INVALID, T, "null output");
        expect(tfhe_lut_spread(&p, nullptr, 4, 0, nullptr, 0) == TFHE_OK, T, "B = 0");
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
