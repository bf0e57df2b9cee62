// A radix adder as a LUT circuit on this engine, through the host-side mirror
// (tfhe.hpp: LutSet, LutCircuit): 8-bit + 8-bit as four base-4 digits under the
// UINT4 set with message modulus 16 (2 message bits, 2 bits of carry room); per
// digit s = a_i + b_i + carry, message = s mod 4, carry = s div 4.
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
    constexpr uint32_t M = 16, DIGITS = 4;
    auto [sk, ck] = CloudKey::generate(P, 42, 43);
    std::vector<uint32_t> f_msg(M), f_carry(M);
    for (uint32_t x = 0; x < M; x++) {
        f_msg[x] = x % 4;
        f_carry[x] = x / 4;
    }
    const LutSet set(ck, {lutGenerate(P, f_msg), lutGenerate(P, f_carry)});

    LutCircuit c;
    std::vector<LutCircuit::Wire> a, b;
    for (uint32_t i = 0; i < DIGITS; i++) a.push_back(c.input());
    for (uint32_t i = 0; i < DIGITS; i++) b.push_back(c.input());
    for (LutCircuit::Wire w : c.radixAdd(a, b, 0, 1)) c.output(w);
    uint32_t depth = 0;
    const std::vector<uint32_t> levels = c.schedule(&depth);
    expect(c.numNodes() == 2 * DIGITS && depth == DIGITS, "radix add", "4 digits are 8 nodes at depth 4");
    expect(levels.front() == 1 && levels.back() == DIGITS, "radix add", "levels follow the carry chain");

    const uint32_t pairs[3][2] = {{0xB7, 0x5E}, {0xFF, 0xFF}, {0, 0}};
    uint64_t seed = 1000;
    for (const auto &pr : pairs) {
        std::vector<TLWELv0> in;
        for (uint32_t v : {pr[0], pr[1]})
            for (uint32_t i = 0; i < DIGITS; i++) in.push_back(sk.encryptLweMessage((v >> (2 * i)) & 3, M, seed++));
        uint32_t ran = 0;
        const std::vector<TLWELv0> out = c.run(ck, set, in, &ran);
        uint32_t sum = 0;
        for (size_t i = 0; i < out.size(); i++) sum |= sk.decryptLweMessage(out[i], M) << (2 * i);
        expect(ran == DIGITS, "radix add", "bootstrap depth");
        expect(sum == pr[0] + pr[1], "radix add", "decrypted sum differs");
        std::printf("     0x%02X + 0x%02X = 0x%03X\n", pr[0], pr[1], sum);
    }
    std::printf("ok   radix add as a LUT circuit\n");
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
