// Encrypted writes into a packed table through the host-side mirror (tfhe.hpp): a 16-entry
// table of 4-bit words in one TRLWE, three entries set by encrypted addresses with
// packedWrite (lookup, extract, bootstrap, new - old', packTlwe, packedScatterAdd), then all
// 16 entries read back by encrypted addresses; they decrypt to the plaintext model.  A
// second table of 4 whole TRLWEs (width N: the demux tree alone) takes one scatter-add.
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
    const tfhe_params P = params::SECURITY_128_BIT();
    auto [sk, ck] = CloudKey::generate(P, 42, 43);
    uint64_t seed = 800;
    const PackingKey key = PackingKey::generate(ck, sk, 9000, P.alpha_lv1, 2, 8);

    // selectors 0 .. 63: bit j of address e at 4 e + j, shared by the writes and the reads
    std::vector<double> fft;
    for (uint32_t e = 0; e < 16; e++)
        for (uint32_t j = 0; j < 4; j++) {
            const TRGSWLv1FFT bit = TRGSWLv1FFT::encryptTorus((e >> j) & 1, P.alpha_bsk, sk.key_lv1, ck, seed++);
            fft.insert(fft.end(), bit.fft.begin(), bit.fft.end());
        }
    const TrgswSet set(ck, fft, 64);
    auto address = [](std::vector<uint32_t> &addr, uint32_t e) {
        for (uint32_t j = 0; j < 4; j++) addr.push_back(4 * e + j);
    };

    {
        const char *T = "packedWrite: 16 x 4 bits";
        std::vector<uint64_t> model(16);
        for (uint32_t e = 0; e < 16; e++) model[e] = (e * 5 + 1) & 0xF;
        PackedTableLookup tl = PackedTableLookup::fromBits(P, model, 4);
        expect(tl.plan.trlwes == 1 && tl.plan.h == 4 && tl.plan.v == 0, T, "plan: one TRLWE, 16 slots");
        const uint32_t where[3] = {3, 12, 6}, what[3] = {0x9, 0x0, 0xF};
        std::vector<uint32_t> addr;
        std::vector<TLWELv0> in;
        for (int q = 0; q < 3; q++) {
            address(addr, where[q]);
            for (uint32_t c = 0; c < 4; c++) in.push_back(sk.encryptBool((what[q] >> c) & 1, seed++));
            model[where[q]] = what[q];
        }
        packedWrite(ck, set, key, addr, in, tl);
        std::vector<uint32_t> all;
        for (uint32_t e = 0; e < 16; e++) address(all, e);
        const std::vector<TRLWELv1> out = tl.lookup(ck, set, all);
        for (uint32_t e = 0; e < 16; e++) {
            const std::vector<TLWELv0> bits = TableLookup::extractBits(ck, out[e], {0, 1, 2, 3});
            uint32_t v = 0;
            for (size_t c = 0; c < 4; c++) v |= (uint32_t)sk.decryptBool(bits[c]) << c;
            expect(v == model[e], T, "an entry read back differs from the model");
        }
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "packedScatterAdd: 4 whole TRLWEs";
        // 4 entries of N bits, every bit 0: trivial TRLWEs with -1/8 in every coefficient (fromBits packs
        // at most 64 bits per entry)
        PackedTableLookup tl;
        tl.k = 2;
        tl.width = P.N;
        check(tfhe_packed_lookup_plan(&P, tl.k, tl.width, &tl.plan), "packed_lookup_plan");
        tl.table.assign(4 * 2 * (size_t)P.N, 0u);
        for (uint32_t e = 0; e < 4; e++)
            std::fill(tl.table.begin() + (2 * e + 1) * (size_t)P.N, tl.table.begin() + (2 * e + 2) * (size_t)P.N, 0xE0000000u);
        expect(tl.plan.trlwes == 4 && tl.plan.h == 0 && tl.plan.v == 2, T, "plan: the tree alone");
        // +1/4 on coefficients 0 .. 7 of entry 2 turns those bits to 1
        std::vector<double> mu(P.N, 0.0);
        for (int c = 0; c < 8; c++) mu[c] = 0.25;
        const std::vector<TRLWELv1> delta = {TRLWELv1::encryptF64(mu, P.alpha_lv1, sk.key_lv1, ck, seed++)};
        const std::vector<uint32_t> addr = {4 * 2 + 0, 4 * 2 + 1};  // bits 0, 1 of address 2
        packedScatterAdd(ck, set, addr, delta, tl);
        for (uint32_t e = 0; e < 4; e++) {
            TRLWELv1 x;
            std::copy(tl.table.begin() + e * 2 * (size_t)P.N, tl.table.begin() + (e + 1) * 2 * (size_t)P.N, x.p.begin());
            const std::vector<bool> dec = x.decryptBool(sk.key_lv1, ck);
            bool ok = true;
            for (uint32_t c = 0; c < (uint32_t)P.N; c++) ok = ok && dec[c] == (e == 2 && c < 8);
            expect(ok, T, "a table TRLWE decrypts to other bits than the model's");
        }
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
