// The reference's own CMUX test (src/trgsw.zig:637-692, "trgsw cmux") on this
// engine, through the host-side mirror (tfhe.hpp): random TRLWE plaintexts,
// TRGSW encryptions of 1 and 0, cmux under each, decrypt and compare; then a
// table lookup by encrypted address bits whose extracted outputs feed a gate.
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
// splitmix64: the plaintext bits of the test (the reference draws them from DefaultPrng(42))
uint64_t next(uint64_t &s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
}  // namespace

int main() {
    using namespace tfhe;
    const tfhe_params P = params::SECURITY_128_BIT();
    const SecretKey sk = SecretKey::newWithSeed(P, 42);
    {  // trgsw.zig:637-692
        const CloudKey ck = CloudKey::newNoKsk(P);
        const size_t N = P.N;
        const double ALPHA = P.alpha_lv1;  // trgsw_lv1.ALPHA
        uint64_t rng = 42, seed = 100;
        for (int t = 0; t < 5; t++) {
            std::vector<bool> pt1(N), pt2(N);
            for (size_t i = 0; i < N; i++) {
                pt1[i] = next(rng) & 1;
                pt2[i] = next(rng) & 1;
            }
            const TRLWELv1 c1 = TRLWELv1::encryptBool(pt1, ALPHA, sk.key_lv1, ck, seed++);
            const TRLWELv1 c2 = TRLWELv1::encryptBool(pt2, ALPHA, sk.key_lv1, ck, seed++);
            const TRGSWLv1FFT trgsw_true = TRGSWLv1FFT::encryptTorus(1, ALPHA, sk.key_lv1, ck, seed++);
            const TRGSWLv1FFT trgsw_false = TRGSWLv1FFT::encryptTorus(0, ALPHA, sk.key_lv1, ck, seed++);
            const std::vector<bool> dec1 = cmux(c1, c2, trgsw_false, ck).decryptBool(sk.key_lv1, ck);
            const std::vector<bool> dec2 = cmux(c1, c2, trgsw_true, ck).decryptBool(sk.key_lv1, ck);
            expect(dec1 == pt1, "trgsw cmux", "cond = 0 must give in1");
            expect(dec2 == pt2, "trgsw cmux", "cond = 1 must give in2");
        }
        std::printf("ok   trgsw cmux\n");
    }
    {  // a 16-entry byte table addressed by 4 encrypted bits; the outputs are gate inputs
        const tfhe_params P80 = params::SECURITY_80_BIT();
        auto [sk80, ck] = CloudKey::generate(P80, 42, 43);
        std::vector<uint64_t> values(16);
        for (size_t e = 0; e < 16; e++) values[e] = (e * 37 + 11) & 0xFF;
        const TableLookup tl = TableLookup::fromBits(P80, values, 8);
        const uint32_t queries[3] = {0, 15, 9};
        std::vector<double> fft;
        std::vector<uint32_t> addr;
        uint64_t seed = 500;
        for (uint32_t q : queries)
            for (uint32_t j = 0; j < 4; j++) {
                const TRGSWLv1FFT b = TRGSWLv1FFT::encryptTorus((q >> j) & 1, P80.alpha_bsk, sk80.key_lv1, ck, seed++);
                fft.insert(fft.end(), b.fft.begin(), b.fft.end());
                addr.push_back((uint32_t)addr.size());
            }
        const TrgswSet set(ck, fft, addr.size());
        const std::vector<TRLWELv1> out = tl.lookup(ck, set, addr);
        const Gates gates;
        for (size_t q = 0; q < 3; q++) {
            const std::vector<TLWELv0> bits = TableLookup::extractBits(ck, out[q], {0, 1, 2, 3, 4, 5, 6, 7});
            uint64_t v = 0;
            for (size_t c = 0; c < 8; c++) v |= (uint64_t)sk80.decryptBool(bits[c]) << c;
            expect(v == values[queries[q]], "table lookup", "decrypted byte differs from the table entry");
            const TLWELv0 r = gates.andGate(bits[0], sk80.encryptBool(true, seed++), ck);
            expect(sk80.decryptBool(r) == bool(values[queries[q]] & 1), "table lookup", "AND of an output bit");
        }
        std::printf("ok   table lookup -> extract -> gate\n");
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
