// Extended nodes on this engine, through the host-side mirror (tfhe.hpp: LutCircuit's eta arguments, lutSelectExt,
// bootstrapLutEachExt): a 64-word memory of 6-bit values, client-encrypted under the UINT4 set at message modulus
// 64, read at base + offset with both operands encrypted (a carry-free sum below 64: the bootstrap is negacyclic).
// The address is the select node's own linear combination and the read is ONE extended select node (m = 64,
// eta = 2) per address; the flat lutSelectExt gives the same words, and bootstrapLutEachExt with a plaintext table
// in every component reads the same table.
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
    using Wire = LutCircuit::Wire;
    const tfhe_params P = params::SECURITY_UINT4();
    constexpr uint32_t M = 64, ETA = 2;
    auto [sk, ck] = CloudKey::generate(P, 42, 43);
    const PackingKey key = PackingKey::generate(ck, sk, 9300, P.alpha_lv1, 5, 3);

    std::vector<uint32_t> mem(M);
    for (uint32_t i = 0; i < M; i++) mem[i] = (37 * i + 11) % M;
    const uint32_t reads[4][2] = {{0, 0}, {17, 5}, {40, 23}, {20, 43}};  // (base, offset), sums 0, 22, 63, 63

    // one table for the extended ordinary node below: x -> x + 1 mod 64, its four components the set's entries 0..3
    std::vector<uint32_t> inc(M);
    for (uint32_t i = 0; i < M; i++) inc[i] = (i + 1) % M;
    const LutSet set(ck, lutGenerateExt(P, ETA, inc));

    LutCircuit c;
    std::vector<Wire> words, ops;
    for (uint32_t i = 0; i < M; i++) words.push_back(c.input());
    for (int k = 0; k < 8; k++) ops.push_back(c.input());
    std::vector<LutCircuit::Entry> entries(words.begin(), words.end());
    for (int k = 0; k < 4; k++) c.output(c.select({{ops[2 * k], 1}, {ops[2 * k + 1], 1}}, entries, 0, ETA));
    c.output(c.node(0, {{ops[2], 1}}, 0, 0, ETA));  // 17 + 1
    std::vector<uint32_t> groups;
    uint32_t depth = 0;
    c.scheduleExt(groups, &depth);
    expect(depth == 1 && groups == std::vector<uint32_t>({0, 0, 5}), "schedule", "one level, five eta = 2 nodes");

    std::vector<TLWELv0> cts;
    uint64_t seed = 5000;
    for (uint32_t v : mem) cts.push_back(sk.encryptLweMessage(v, M, seed++));
    for (const auto &r : reads)
        for (uint32_t v : r) cts.push_back(sk.encryptLweMessage(v, M, seed++));
    uint32_t levels = 0;
    const std::vector<TLWELv0> out = c.run(ck, set, cts, &levels, &key);
    expect(levels == 1, "run", "one bootstrap level");
    for (int k = 0; k < 4; k++) {
        const uint32_t got = sk.decryptLweMessage(out[k], M), want = mem[reads[k][0] + reads[k][1]];
        expect(got == want, "memory read", "decrypted word differs");
        std::printf("     mem[%u + %u] = %u\n", reads[k][0], reads[k][1], got);
    }
    expect(sk.decryptLweMessage(out[4], M) == 18, "extended node", "17 + 1");

    // the flat form gives the circuit's words
    {
        std::vector<LutSelectNode> nodes(4);
        for (int k = 0; k < 4; k++) {
            nodes[k].terms = {{M + 2 * k, 1}, {M + 2 * k + 1, 1}};
            for (uint32_t i = 0; i < M; i++) nodes[k].entries.push_back(LutCircuit::Entry(i));
        }
        const std::vector<TLWELv0> flat = lutSelectExt(ck, key, M, ETA, cts, nodes);
        bool same = true;
        for (int k = 0; k < 4; k++) same = same && flat[k].p == out[k].p;
        expect(same, "lutSelectExt", "words differ from the circuit's");
    }
    // one plaintext table in every component: the E-copies identity
    {
        const std::vector<std::vector<Torus>> one = lutGenerateExt(P, 0, mem);
        TRLWELv1 tv;
        std::copy(one[0].begin(), one[0].end(), tv.p.begin());
        const std::vector<TLWELv0> in{cts[M + 2], cts[M + 7]};  // 17, 43
        const std::vector<TLWELv0> r = bootstrapLutEachExt(ck, ETA, in, {tv, tv});
        expect(sk.decryptLweMessage(r[0], M) == mem[17] && sk.decryptLweMessage(r[1], M) == mem[43], "bootstrapLutEachExt",
               "a plaintext table in every component");
    }
    std::printf("ok   extended nodes: a 64-word encrypted memory read by one select node per address\n");
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
