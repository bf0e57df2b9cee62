// The extended LUT bootstrap on this engine, through the host-side mirror (tfhe.hpp: lutGenerateExt,
// blindRotateExt, lutApplyExt): a random 6-bit-to-4-bit table (an S-box of the DES kind) looked up in
// one bootstrap under the UINT4 set, at the message modulus m = 64 with eta = 2, i.e. the blind
// rotation on E = 4 accumulator components, whose mod switch rounds to 2N E = 8192 positions.  Every
// 6-bit message is looked up; one item is also rebuilt from the stage entry (acc_0, extracted at
// coefficient 0 and key-switched) and compared word for word.
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
    constexpr uint32_t M = 64, ETA = 2, E = 1u << ETA;
    auto [sk, ck] = CloudKey::generate(P, 42, 43);
    std::vector<uint32_t> sbox(M);
    uint32_t s = 2024;
    for (uint32_t x = 0; x < M; x++) sbox[x] = ((s = s * 1664525u + 1013904223u) >> 28) & 15u;  // 4 bits out
    const std::vector<std::vector<Torus>> tv = lutGenerateExt(P, ETA, sbox);
    expect(tv.size() == E, "lutGenerateExt", "2^eta components");
    expect(lutGenerateExt(P, 0, sbox)[0] == lutGenerate(P, sbox), "lutGenerateExt", "eta = 0 is lutGenerate");
    const LutSet set(ck, tv);

    std::vector<TLWELv0> pool;
    std::vector<LutExtNode> nodes;
    for (uint32_t x = 0; x < M; x++) {
        pool.push_back(sk.encryptLweMessage(x, M, 3000 + x));
        nodes.push_back({0, {{x, 1}}});
    }
    const std::vector<TLWELv0> out = lutApplyExt(ck, set, ETA, pool, nodes);
    uint32_t wrong = 0;
    for (uint32_t x = 0; x < M; x++) wrong += sk.decryptLweMessage(out[x], M) != sbox[x];
    expect(wrong == 0, "lutApplyExt", "a decrypted S-box value differs");
    std::printf("     S(%2u) = %2u, S(%2u) = %2u, S(%2u) = %2u\n", 0u, sk.decryptLweMessage(out[0], M), 37u,
                sk.decryptLweMessage(out[37], M), 63u, sk.decryptLweMessage(out[63], M));

    // item 37 from the stage entry: acc_0 of the extended blind rotation, extracted and key-switched
    const std::vector<TRLWELv1> acc = blindRotateExt(ck, ETA, {pool[37]}, tv);
    expect(acc.size() == E, "blindRotateExt", "E accumulators per item");
    expect(TableLookup::extractBits(ck, acc[0], {0})[0].p == out[37].p, "lutApplyExt", "the composition's words");
    std::printf("ok   extended LUT bootstrap: 6-bit to 4-bit table, m = 64, eta = 2\n");
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
