// Stand-alone test of the packing key switch's GPU-free part (csrc/tfhe_cpu.cpp):
// tfhe_pack_tlwe against a direct restatement of its definition, and its argument
// checks.  Links tfhe_cpu.o only (no HIP, no libtfhe_gpu.so) and builds and runs
// under the host sanitizers too (make cpu-check).  Exit status 0 = all passed.
#include "tfhe_gpu.h"

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
uint64_t state = 0x9E3779B97F4A7C15ull;
uint32_t next() {  // xorshift64*: key rows and inputs are arbitrary words
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return (uint32_t)((state * 0x2545F4914F6CDD1Dull) >> 32);
}
}  // namespace

int main() {
    const size_t N = 1024;
    struct Shape {
        tfhe_params P;
        uint32_t basebit, t;
    };
    const Shape shapes[] = {
        {{20, 1024, 10, 3, 6, 2, 9, 0, 2.0e-5, 2.0e-8, 2.0e-5, 2.0e-8}, 2, 8},
        {{36, 1024, 10, 3, 6, 2, 9, 0, 2.0e-5, 2.0e-8, 2.0e-5, 2.0e-8}, 2, 7},
        {{18, 1024, 10, 1, 22, 5, 3, 0, 2.5e-6, 2.2e-16, 2.5e-6, 0.0}, 5, 3},
        {{18, 1024, 10, 1, 22, 5, 3, 0, 2.5e-6, 2.2e-16, 2.5e-6, 0.0}, 5, 2},
    };
    {
        const char *T = "pack_tlwe";
        for (const Shape &sh : shapes) {
            const size_t n = sh.P.n, base = (size_t)1 << sh.basebit, B = 2, C = 5;
            const uint32_t coef[C] = {1023, 0, 7, 512, 300};
            // exactly the documented sizes, so a read or write past one is the sanitizer's to catch
            std::vector<uint32_t> rows(n * sh.t * base * 2 * N), in(B * C * (n + 1)), out(B * 2 * N, 0xDEADBEEFu);
            for (uint32_t &w : rows) w = next();
            for (uint32_t &w : in) w = next();
            const uint32_t prec = 1u << (32 - (1 + sh.basebit * sh.t));
            for (size_t i = 0; i < n; i++) in[i] = i & 1 ? 0xFFFFFFFFu : prec;  // item 0: edge digits
            expect(tfhe_pack_tlwe(&sh.P, rows.data(), sh.basebit, sh.t, in.data(), coef, C, out.data(), B) == TFHE_OK, T,
                   "status");
            std::vector<uint32_t> want(B * 2 * N, 0u), R(2 * N);
            for (size_t g = 0; g < B * C; g++) {
                const uint32_t *x = in.data() + g * (n + 1);
                for (size_t w = 0; w < 2 * N; w++) R[w] = 0;
                R[N] = x[n];
                for (size_t i = 0; i < n; i++)
                    for (uint32_t j = 0; j < sh.t; j++) {
                        const uint32_t d = ((x[i] + prec) >> (32 - (j + 1) * sh.basebit)) & (uint32_t)(base - 1);
                        const uint32_t *row = rows.data() + (base * sh.t * i + base * j + d) * 2 * N;
                        for (size_t w = 0; w < 2 * N; w++) R[w] -= row[w];
                    }
                const size_t k = coef[g % C];
                uint32_t *o = want.data() + (g / C) * 2 * N;
                for (size_t half = 0; half < 2; half++)
                    for (size_t p = 0; p < N; p++)  // polyMulWithXK: res[p] = a[p - k], negated where it wraps
                        o[half * N + p] += p >= k ? R[half * N + p - k] : 0u - R[half * N + p - k + N];
            }
            expect(out == want, T, "out[b] = sum_c X^coef[c] R_{b,c}");
        }
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "pack_tlwe argument checks";
        const Shape &sh = shapes[0];
        const size_t n = sh.P.n;
        std::vector<uint32_t> rows(n * 8 * 4 * 2 * N), in(3 * (n + 1)), out(2 * N), many(N + 1);
        for (size_t i = 0; i <= N; i++) many[i] = (uint32_t)i;
        const uint32_t ok[3] = {3, 0, 1023}, big[3] = {3, 0, 1024}, dup[3] = {3, 0, 3};
        auto call = [&](const tfhe_params *p, const uint32_t *r, uint32_t bb, uint32_t t, const uint32_t *i, const uint32_t *c,
                        size_t C, uint32_t *o) { return tfhe_pack_tlwe(p, r, bb, t, i, c, C, o, 1); };
        expect(call(&sh.P, rows.data(), 2, 8, in.data(), ok, 3, out.data()) == TFHE_OK, T, "a good call");
        expect(call(nullptr, rows.data(), 2, 8, in.data(), ok, 3, out.data()) == TFHE_ERR_INVALID, T, "null params");
        expect(call(&sh.P, nullptr, 2, 8, in.data(), ok, 3, out.data()) == TFHE_ERR_INVALID, T, "null rows");
        expect(call(&sh.P, rows.data(), 2, 8, nullptr, ok, 3, out.data()) == TFHE_ERR_INVALID, T, "null in");
        expect(call(&sh.P, rows.data(), 2, 8, in.data(), nullptr, 3, out.data()) == TFHE_ERR_INVALID, T, "null coef");
        expect(call(&sh.P, rows.data(), 2, 8, in.data(), ok, 3, nullptr) == TFHE_ERR_INVALID, T, "null out");
        expect(call(&sh.P, rows.data(), 2, 8, in.data(), ok, 0, out.data()) == TFHE_ERR_INVALID, T, "C = 0");
        expect(call(&sh.P, rows.data(), 2, 8, in.data(), many.data(), N + 1, out.data()) == TFHE_ERR_INVALID, T, "C = N + 1");
        expect(call(&sh.P, rows.data(), 2, 8, in.data(), big, 3, out.data()) == TFHE_ERR_INVALID, T, "coef = N");
        expect(call(&sh.P, rows.data(), 2, 8, in.data(), dup, 3, out.data()) == TFHE_ERR_INVALID, T, "a duplicate coef");
        expect(call(&sh.P, rows.data(), 4, 3, in.data(), ok, 3, out.data()) == TFHE_ERR_INVALID, T, "shape (4, 3)");
        expect(call(&sh.P, rows.data(), 2, 6, in.data(), ok, 3, out.data()) == TFHE_ERR_INVALID, T, "shape (2, 6)");
        expect(tfhe_pack_tlwe(&sh.P, rows.data(), 2, 8, nullptr, ok, 3, nullptr, 0) == TFHE_OK, T, "B = 0");
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
