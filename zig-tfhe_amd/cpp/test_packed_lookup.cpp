// The packed table lookup on this engine, through the host-side mirror (tfhe.hpp): a
// 256-entry byte table (an S-box) as 2 TRLWEs, addressed by 8 TRGSW-encrypted bits
// per query with 1 + 7 = 8 CMUXes where the CMUX tree alone takes 255; the extracted
// outputs decrypt to the table's entries.  Then rotateByBits on an encrypted
// polynomial.  Runs on one MI355X; exit status 0 = all passed.
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
    uint64_t seed = 500;
    {
        const char *T = "packed S-box lookup";
        std::vector<uint64_t> sbox(256);
        for (size_t e = 0; e < 256; e++) sbox[e] = (e * 167 + 13) & 0xFF;  // 167 is odd: a permutation of 0..255
        const PackedTableLookup tl = PackedTableLookup::fromBits(P, sbox, 8);
        expect(tl.plan.stride == 8 && tl.plan.h == 7 && tl.plan.v == 1 && tl.plan.trlwes == 2 && tl.plan.cmuxes == 8, T,
               "plan: 2 TRLWEs, 8 CMUXes");
        const uint32_t queries[4] = {0, 255, 0x5A, 0xA7};
        std::vector<double> fft;
        std::vector<uint32_t> addr;
        for (uint32_t q : queries)
            for (uint32_t j = 0; j < 8; j++) {
                const TRGSWLv1FFT b = TRGSWLv1FFT::encryptTorus((q >> j) & 1, P.alpha_bsk, sk.key_lv1, ck, seed++);
                fft.insert(fft.end(), b.fft.begin(), b.fft.end());
                addr.push_back((uint32_t)addr.size());
            }
        const TrgswSet set(ck, fft, addr.size());
        const std::vector<TRLWELv1> out = tl.lookup(ck, set, addr);
        for (size_t q = 0; q < 4; q++) {
            const std::vector<TLWELv0> bits = TableLookup::extractBits(ck, out[q], {0, 1, 2, 3, 4, 5, 6, 7});
            uint64_t v = 0;
            for (size_t c = 0; c < 8; c++) v |= (uint64_t)sk.decryptBool(bits[c]) << c;
            expect(v == sbox[queries[q]], T, "decrypted byte differs from the table entry");
        }
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "rotateByBits";
        const size_t N = P.N;
        std::vector<bool> pt(N);
        for (size_t i = 0; i < N; i++) pt[i] = (i * i + i / 7) & 1;
        const TRLWELv1 c = TRLWELv1::encryptBool(pt, P.alpha_lv1, sk.key_lv1, ck, seed++);
        // bits 1, 0, 1 under X^-1, X^-2, X^-4: X^-5 in all, coefficient i of the result is coefficient i + 5
        std::vector<double> fft;
        for (uint32_t bit : {1u, 0u, 1u}) {
            const TRGSWLv1FFT b = TRGSWLv1FFT::encryptTorus(bit, P.alpha_bsk, sk.key_lv1, ck, seed++);
            fft.insert(fft.end(), b.fft.begin(), b.fft.end());
        }
        const TrgswSet set(ck, fft, 3);
        const uint32_t M = 2 * (uint32_t)N;
        const std::vector<bool> dec = rotateByBits(c, {M - 1, M - 2, M - 4}, set, {0, 1, 2}, ck).decryptBool(sk.key_lv1, ck);
        bool ok = true;
        for (size_t i = 0; i < N; i++) ok = ok && dec[i] == (i + 5 < N ? pt[i + 5] : !pt[i + 5 - N]);
        expect(ok, T, "X^-5: coefficient i + 5, negated past N");
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
