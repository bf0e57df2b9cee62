// Select nodes on this engine, through the host-side mirror (tfhe.hpp: LutCircuit::select / node2,
// lutSelect): the AES S-box after a key addition, S[x ^ k], on bytes held as two 4-bit digits under the
// UINT4 set at its full message modulus 16.  One circuit call per batch of bytes: the nibble XORs by two
// node2, then the S-box's two output nibbles by two node2 over the XORed nibbles: depth 4.  The flat
// lutSelect reads a table of constants and a table of pool ciphertexts by an encrypted index.
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
// The AES S-box: the inverse in GF(2^8) mod x^8 + x^4 + x^3 + x + 1, then the affine map (FIPS 197, 5.1.1).
std::vector<uint32_t> aesSbox() {
    auto mul = [](uint32_t a, uint32_t b) {
        uint32_t r = 0;
        for (; b; b >>= 1, a = (a << 1) ^ (a & 0x80 ? 0x11B : 0))
            if (b & 1) r ^= a;
        return r & 0xFF;
    };
    std::vector<uint32_t> S(256);
    for (uint32_t x = 0; x < 256; x++) {
        uint32_t inv = 0;
        for (uint32_t y = 1; y < 256 && x; y++)
            if (mul(x, y) == 1) inv = y;
        uint32_t s = inv;
        for (int r = 1; r <= 4; r++) s ^= ((inv << r) | (inv >> (8 - r))) & 0xFF;
        S[x] = s ^ 0x63;
    }
    return S;
}
}  // namespace

int main() {
    using namespace tfhe;
    using Wire = LutCircuit::Wire;
    const tfhe_params P = params::SECURITY_UINT4();
    constexpr uint32_t M = 16;
    auto [sk, ck] = CloudKey::generate(P, 42, 43);
    const PackingKey key = PackingKey::generate(ck, sk, 9100, P.alpha_lv1, 5, 3);
    const std::vector<uint32_t> S = aesSbox();
    expect(S[0x00] == 0x63 && S[0x53] == 0xED && S[0xFF] == 0x16, "sbox", "FIPS 197's values");

    // tables 0..15: a ^ b; 16..31: the S-box's high nibble of (h, l); 32..47: its low nibble
    std::vector<uint32_t> fx(M * M), fh(M * M), fl(M * M);
    for (uint32_t a = 0; a < M; a++)
        for (uint32_t b = 0; b < M; b++) fx[a * M + b] = a ^ b, fh[a * M + b] = S[a << 4 | b] >> 4, fl[a * M + b] = S[a << 4 | b] & 15;
    std::vector<std::vector<Torus>> tables = lutGenerate2(P, M, fx);
    for (const std::vector<Torus> &t : lutGenerate2(P, M, fh)) tables.push_back(t);
    for (const std::vector<Torus> &t : lutGenerate2(P, M, fl)) tables.push_back(t);
    const LutSet set(ck, tables);

    const uint32_t pairs[4][2] = {{0x00, 0x00}, {0x53, 0x00}, {0xA7, 0x5C}, {0xFF, 0x0F}};
    LutCircuit c;
    std::vector<Wire> in;
    for (int k = 0; k < 16; k++) in.push_back(c.input());  // per pair: x high, x low, k high, k low
    for (int k = 0; k < 4; k++) {
        const Wire xh = in[4 * k], xl = in[4 * k + 1], kh = in[4 * k + 2], kl = in[4 * k + 3];
        const Wire th = c.node2(0, {{xh, 1}}, {{kh, 1}}, M), tl = c.node2(0, {{xl, 1}}, {{kl, 1}}, M);
        c.output(c.node2(16, {{th, 1}}, {{tl, 1}}, M));
        c.output(c.node2(32, {{th, 1}}, {{tl, 1}}, M));
    }
    uint32_t depth = 0;
    c.schedule(&depth);
    expect(depth == 4 && c.numNodes() == 4 * 4 * 17, "schedule", "depth 4, 17 nodes per node2");
    std::vector<TLWELv0> cts;
    uint64_t seed = 3000;
    for (const auto &pr : pairs)
        for (uint32_t nib : {pr[0] >> 4, pr[0] & 15, pr[1] >> 4, pr[1] & 15}) cts.push_back(sk.encryptLweMessage(nib, M, seed++));
    uint32_t levels = 0;
    const std::vector<TLWELv0> out = c.run(ck, set, cts, &levels, &key);
    expect(levels == 4, "run", "four bootstrap levels");
    for (int k = 0; k < 4; k++) {
        const uint32_t got = sk.decryptLweMessage(out[2 * k], M) << 4 | sk.decryptLweMessage(out[2 * k + 1], M);
        expect(got == S[pairs[k][0] ^ pairs[k][1]], "sbox circuit", "decrypted byte differs");
        std::printf("     S[%02X ^ %02X] = %02X\n", pairs[k][0], pairs[k][1], got);
    }
    bool refused = false;
    try {
        c.run(ck, set, cts);
    } catch (const Error &) {
        refused = true;
    }
    expect(refused, "run", "select nodes without a packing key");

    // the flat form: entries that are constants (Encoder.new(16): v / 32 of the torus), and entries from the pool
    {
        std::vector<TLWELv0> pool;
        for (uint32_t v : {11u, 2u, 5u, 14u}) pool.push_back(sk.encryptLweMessage(v, M, seed++));
        for (uint32_t idx : {1u, 3u}) pool.push_back(sk.encryptLweMessage(idx, M, seed++));
        LutSelectNode consts, wires;
        for (uint32_t i = 0; i < M; i++) {
            consts.entries.push_back(LutCircuit::Entry::constant(((7 * i + 2) % M) << 27));
            wires.entries.push_back(LutCircuit::Entry(i % 4));
        }
        consts.terms = {{4, 1}, {5, 1}};  // 1 + 3
        wires.terms = {{5, 1}};           // 3
        const std::vector<TLWELv0> r = lutSelect(ck, key, M, pool, {consts, wires});
        expect(sk.decryptLweMessage(r[0], M) == (7 * 4 + 2) % M, "lutSelect", "constant entries");
        expect(sk.decryptLweMessage(r[1], M) == 14, "lutSelect", "pool entries");
    }
    std::printf("ok   select nodes: S[x ^ k] on nibbles in one circuit\n");
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
