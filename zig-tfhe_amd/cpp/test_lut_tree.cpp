// The bivariate LUT bootstrap on this engine, through the host-side mirror (tfhe.hpp: lutGenerate2,
// lutApply2, lutSpread, bootstrapLutEach): the product of two 4-bit digits under the UINT4 set at its
// full message modulus 16, low and high nibble as F = 2 functions.  Per output digit 16 level-1
// bootstraps of y, one pack into the slots i * 64, the spread into a test vector, one bootstrap of x.
// The fused call is also rebuilt from the separate entries and compared word for word.
// Runs on one MI355X; exit status 0 = all passed.
#include "tfhe.hpp"

#include <cstdio>

namespace {
int failures = 0;
void expect(bool ok, const char *test, const char *what) {
    if (!ok) {
        std::printf("FAIL %s: %s\n", test, what);
        failures++;
    }
}
}  // namespace

int main() {
    using namespace tfhe;
    const tfhe_params P = params::SECURITY_UINT4();
    constexpr uint32_t M = 16;
    const uint32_t W = P.N / M, ROT = 2 * P.N - P.N / (2 * M);
    auto [sk, ck] = CloudKey::generate(P, 42, 43);
    const PackingKey key = PackingKey::generate(ck, sk, 9000, P.alpha_lv1, 5, 3);
    std::vector<uint32_t> lo(M * M), hi(M * M);
    for (uint32_t x = 0; x < M; x++)
        for (uint32_t y = 0; y < M; y++) lo[x * M + y] = (x * y) % M, hi[x * M + y] = (x * y) / M;
    std::vector<std::vector<Torus>> tables = lutGenerate2(P, M, lo);
    for (const std::vector<Torus> &t : lutGenerate2(P, M, hi)) tables.push_back(t);
    const LutSet set(ck, tables);
    expect(set.size() == 2 * M, "lutGenerate2", "F * m tables");

    // spread of the trivial slot TRLWE is the generator's table
    std::vector<uint32_t> f(M);
    for (uint32_t x = 0; x < M; x++) f[x] = (5 * x + 3) % M;
    TRLWELv1 slots;
    for (uint32_t x = 0; x < M; x++) slots.p[P.N + x * W] = f[x] << 27;  // Encoder.new(16): f / 32 of the torus
    expect(lutSpread(ck, {slots}, W, ROT)[0].p == lutGenerate(P, f), "lutSpread", "the generator's words");

    const uint32_t pairs[5][2] = {{0, 0}, {15, 15}, {7, 9}, {12, 3}, {1, 14}};
    std::vector<TLWELv0> pool;
    std::vector<Lut2Node> nodes;
    uint64_t seed = 2000;
    for (const auto &pr : pairs) {
        pool.push_back(sk.encryptLweMessage(pr[0], M, seed++));
        pool.push_back(sk.encryptLweMessage(pr[1], M, seed++));
        const uint32_t at = (uint32_t)pool.size() - 2;
        nodes.push_back({0, at, at + 1});
        nodes.push_back({1, at, at + 1});
    }
    const std::vector<TLWELv0> out = lutApply2(ck, set, key, M, pool, nodes);
    for (size_t k = 0; k < 5; k++) {
        const uint32_t x = pairs[k][0], y = pairs[k][1];
        const uint32_t got = sk.decryptLweMessage(out[2 * k], M) | sk.decryptLweMessage(out[2 * k + 1], M) << 4;
        expect(got == x * y, "lutApply2", "decrypted product differs");
        std::printf("     %2u * %2u = %3u\n", x, y, got);
    }

    // node 5 (7 * 9, high nibble) from the separate entries: the same words
    {
        const Lut2Node nd = nodes[5];
        LutCircuit c;
        const LutCircuit::Wire yw = c.input();
        for (uint32_t i = 0; i < M; i++) c.output(c.node(nd.fn * M + i, {{yw, 1}}));
        const std::vector<TLWELv0> g = c.run(ck, set, {pool[nd.y_src]});
        std::vector<uint32_t> coef(M);
        for (uint32_t i = 0; i < M; i++) coef[i] = i * W;
        const std::vector<TRLWELv1> tv = lutSpread(ck, packTlwe(ck, key, g, coef), W, ROT);
        expect(bootstrapLutEach(ck, {pool[nd.x_src]}, tv)[0].p == out[5].p, "lutApply2", "the composition's words");
    }
    std::printf("ok   bivariate LUT bootstrap: 4-bit x 4-bit products\n");
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
