// A table computed on the server, then looked up by an encrypted address, through the
// host-side mirror (tfhe.hpp): 16 encrypted 4-bit values are XORed with an encrypted
// 4-bit mask (64 gates), the gate outputs are packed into one TRLWE by the packing key
// switch (PackingKey, PackedTableLookup::fromCiphertexts), the table is addressed by 4
// TRGSW-encrypted bits, and the extracted result decrypts to value[addr] ^ mask.
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
    uint64_t seed = 700;
    const char *T = "computed table -> packed lookup";
    const PackingKey key = PackingKey::generate(ck, sk, 9000, P.alpha_lv1, 2, 8);
    uint32_t value[16];
    const uint32_t mask = 0x6;
    std::vector<uint8_t> ops(64, TFHE_GATE_XOR);
    std::vector<TLWELv0> a, b;
    for (uint32_t e = 0; e < 16; e++) {
        value[e] = (e * 7 + 3) & 0xF;
        for (uint32_t c = 0; c < 4; c++) {
            a.push_back(sk.encryptBool((value[e] >> c) & 1, seed++));
            b.push_back(sk.encryptBool((mask >> c) & 1, seed++));
        }
    }
    const std::vector<TLWELv0> gates = Gates().gateBatch(ops, a, b, ck);
    const PackedTableLookup tl = PackedTableLookup::fromCiphertexts(ck, key, gates, 4, 4);
    expect(tl.plan.trlwes == 1 && tl.plan.stride == 4 && tl.plan.h == 4 && tl.table.size() == 2 * (size_t)P.N, T,
           "plan: one TRLWE, 16 slots of 4 coefficients");
    {
        TRLWELv1 t0;
        std::copy(tl.table.begin(), tl.table.end(), t0.p.begin());
        const std::vector<bool> dec = t0.decryptBool(sk.key_lv1, ck);
        bool ok = true;
        for (uint32_t e = 0; e < 16; e++)
            for (uint32_t c = 0; c < 4; c++) ok = ok && dec[e * 4 + c] == (((value[e] ^ mask) >> c) & 1);
        expect(ok, T, "the packed slots decrypt to value ^ mask");
    }
    const uint32_t queries[5] = {0, 15, 5, 10, 9};
    std::vector<double> fft;
    std::vector<uint32_t> addr;
    for (uint32_t q : queries)
        for (uint32_t j = 0; j < 4; j++) {
            const TRGSWLv1FFT bit = TRGSWLv1FFT::encryptTorus((q >> j) & 1, P.alpha_bsk, sk.key_lv1, ck, seed++);
            fft.insert(fft.end(), bit.fft.begin(), bit.fft.end());
            addr.push_back((uint32_t)addr.size());
        }
    const TrgswSet set(ck, fft, addr.size());
    const std::vector<TRLWELv1> out = tl.lookup(ck, set, addr);
    for (size_t q = 0; q < 5; q++) {
        const std::vector<TLWELv0> bits = TableLookup::extractBits(ck, out[q], {0, 1, 2, 3});
        uint32_t v = 0;
        for (size_t c = 0; c < 4; c++) v |= (uint32_t)sk.decryptBool(bits[c]) << c;
        expect(v == (value[queries[q]] ^ mask), T, "decrypted nibble differs from value[addr] ^ mask");
    }
    std::printf("ok   %s\n", T);
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
