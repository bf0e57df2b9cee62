// The fused radix adder on this engine, through the host-side mirror (tfhe.hpp:
// lutInterleave, LutCircuit::radixAddFused): 8-bit + 8-bit as four base-4 digits under
// the UINT4 set with message modulus 8 (2 message bits, 1 bit of carry room, 1 bit paid
// for the second output); per digit ONE node whose interleaved table gives message =
// s mod 4 at coefficient 0 and carry = s div 4 at coefficient 1 of one blind rotation.
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
    constexpr uint32_t M = 8, DIGITS = 4;
    auto [sk, ck] = CloudKey::generate(P, 42, 43);
    std::vector<uint32_t> f_msg(M), f_carry(M);
    for (uint32_t x = 0; x < M; x++) {
        f_msg[x] = x % 4;
        f_carry[x] = x / 4;
    }
    const LutSet set(ck, {lutInterleave(P, {lutGenerate(P, f_msg), lutGenerate(P, f_carry)})});

    LutCircuit c;
    std::vector<LutCircuit::Wire> a, b;
    for (uint32_t i = 0; i < DIGITS; i++) a.push_back(c.input());
    for (uint32_t i = 0; i < DIGITS; i++) b.push_back(c.input());
    const std::vector<LutCircuit::Wire> sum_wires = c.radixAddFused(a, b, 0);
    for (LutCircuit::Wire w : sum_wires) c.output(w);
    uint32_t depth = 0;
    const std::vector<uint32_t> levels = c.schedule(&depth);
    expect(c.numNodes() == DIGITS && depth == DIGITS, "fused radix add", "4 digits are 4 nodes at depth 4");
    expect(levels.front() == 1 && levels.back() == DIGITS, "fused radix add", "levels follow the carry chain");
    expect(sum_wires == std::vector<LutCircuit::Wire>{8, 10, 12, 14, 15}, "fused radix add", "message wires, then the last carry");

    const TLWELv0 probe = sk.encryptLweMessage(5, M, 77), rounded = lutRoundTlwe(P, 1, probe);
    bool multiples = true;
    for (Torus w : rounded.p) multiples = multiples && w % (1u << 22) == 0;
    expect(multiples, "lutRoundTlwe", "words are multiples of 2^22 at theta = 1");

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
        expect(ran == DIGITS, "fused radix add", "bootstrap depth");
        expect(sum == pr[0] + pr[1], "fused radix add", "decrypted sum differs");
        std::printf("     0x%02X + 0x%02X = 0x%03X\n", pr[0], pr[1], sum);
    }
    std::printf("ok   fused radix add: one two-output node per digit\n");
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
