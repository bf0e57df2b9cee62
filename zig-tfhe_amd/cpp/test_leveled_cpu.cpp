// Stand-alone test of the leveled operations' GPU-free part (csrc/tfhe_cpu.cpp):
// tfhe_lookup_table_pack_bits, the table entries of tfhe_gpu_table_lookup_*, and
// its argument checks.  Links tfhe_cpu.o only — no HIP, no libtfhe_gpu.so — and
// builds and runs under the host sanitizers too (make cpu-check).  Exit status
// 0 = all passed.
#include "tfhe_gpu.h"

#include <cstdio>
#include <vector>

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
    const tfhe_params P{700, 1024, 10, 3, 6, 2, 9, 0, 2.0e-5, 2.0e-8, 2.0e-5, 2.0e-8};
    const uint32_t PLUS = 0x20000000u, MINUS = 0xE0000000u;  // f64ToTorus(+-0.125)
    const size_t N = P.N;
    {
        const char *T = "pack_bits";
        const std::vector<uint64_t> values{0x00, 0xFF, 0xA5, 0x8000000000000001ull};
        for (uint32_t width : {0u, 1u, 8u, 64u, 65u, 1024u}) {
            // exactly entries * 2N words, so a write past the table is the sanitizer's to catch
            std::vector<uint32_t> table(values.size() * 2 * N, 0xDEADBEEFu);
            expect(tfhe_lookup_table_pack_bits(&P, values.data(), values.size(), width, table.data()) == TFHE_OK, T,
                   "status");
            bool ok = true;
            for (size_t e = 0; e < values.size(); e++)
                for (size_t c = 0; c < N; c++) {
                    const bool bit = c < 64 && ((values[e] >> c) & 1);
                    const uint32_t want = c < width ? (bit ? PLUS : MINUS) : 0u;
                    ok = ok && table[e * 2 * N + c] == 0u && table[e * 2 * N + N + c] == want;
                }
            expect(ok, T, "a = 0, b = +-1/8 below width and 0 from width on");
        }
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "pack_bits argument checks";
        std::vector<uint32_t> table(2 * N);
        const uint64_t v = 1;
        tfhe_params bad = P;
        bad.N = 512;
        expect(tfhe_lookup_table_pack_bits(nullptr, &v, 1, 8, table.data()) == TFHE_ERR_INVALID, T, "null params");
        expect(tfhe_lookup_table_pack_bits(&bad, &v, 1, 8, table.data()) == TFHE_ERR_INVALID, T, "unsupported params");
        expect(tfhe_lookup_table_pack_bits(&P, nullptr, 1, 8, table.data()) == TFHE_ERR_INVALID, T, "null values");
        expect(tfhe_lookup_table_pack_bits(&P, &v, 1, 8, nullptr) == TFHE_ERR_INVALID, T, "null table");
        expect(tfhe_lookup_table_pack_bits(&P, &v, 1, 1025, table.data()) == TFHE_ERR_INVALID, T, "width > N");
        expect(tfhe_lookup_table_pack_bits(&P, nullptr, 0, 8, nullptr) == TFHE_OK, T, "no entries");
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
