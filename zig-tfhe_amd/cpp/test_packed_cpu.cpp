// Stand-alone test of the packed lookup's GPU-free part (csrc/tfhe_cpu.cpp):
// tfhe_packed_lookup_plan and tfhe_lookup_table_pack_slots with their argument
// checks.  Links tfhe_cpu.o only (no HIP, no libtfhe_gpu.so) and builds and runs
// under the host sanitizers too (make cpu-check).  Exit status 0 = all passed.
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
        const char *T = "packed_lookup_plan";
        for (uint32_t k : {1u, 5u, 7u, 8u, 22u, 23u})
            for (uint32_t width : {1u, 3u, 8u, 64u, 1000u, 1024u}) {
                uint32_t stride = 1, bits = 0;
                while (stride < width) stride *= 2;
                while ((stride << bits) < N) bits++;
                const uint32_t h = k < bits ? k : bits, v = k - h;
                tfhe_packed_plan pl{};
                const int rc = tfhe_packed_lookup_plan(&P, k, width, &pl);
                if (v > 12) {
                    expect(rc == TFHE_ERR_INVALID, T, "more than 12 bits left to the tree");
                    continue;
                }
                expect(rc == TFHE_OK, T, "status");
                expect(pl.stride == stride && pl.slots == N / stride && pl.h == h && pl.v == v, T, "stride, slots, h, v");
                expect(pl.trlwes == 1u << v && pl.cmuxes == (1u << v) - 1 + h, T, "trlwes, cmuxes");
                bool ok = true;
                for (uint32_t j = 0; j < 10; j++) ok = ok && pl.rot[j] == (j < h ? 2 * N - (stride << j) : 0u);
                expect(ok, T, "rot[j] = 2N - stride 2^j, 0 from h on");
            }
        tfhe_packed_plan pl{};
        tfhe_params bad = P;
        bad.N = 512;
        expect(tfhe_packed_lookup_plan(nullptr, 8, 8, &pl) == TFHE_ERR_INVALID, T, "null params");
        expect(tfhe_packed_lookup_plan(&bad, 8, 8, &pl) == TFHE_ERR_INVALID, T, "unsupported params");
        expect(tfhe_packed_lookup_plan(&P, 8, 8, nullptr) == TFHE_ERR_INVALID, T, "null plan");
        expect(tfhe_packed_lookup_plan(&P, 0, 8, &pl) == TFHE_ERR_INVALID, T, "k = 0");
        expect(tfhe_packed_lookup_plan(&P, 8, 0, &pl) == TFHE_ERR_INVALID, T, "width = 0");
        expect(tfhe_packed_lookup_plan(&P, 8, 1025, &pl) == TFHE_ERR_INVALID, T, "width > N");
        expect(tfhe_packed_lookup_plan(&P, 0xFFFFFFFFu, 8, &pl) == TFHE_ERR_INVALID, T, "k = 2^32 - 1");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "pack_slots";
        const uint32_t shapes[][2] = {{1, 1}, {5, 8}, {8, 8}, {7, 3}, {3, 64}, {11, 1}, {4, 33}};
        for (const auto &kw : shapes) {
            const uint32_t k = kw[0], width = kw[1];
            tfhe_packed_plan pl{};
            expect(tfhe_packed_lookup_plan(&P, k, width, &pl) == TFHE_OK, T, "plan");
            std::vector<uint64_t> values((size_t)1 << k);
            for (size_t e = 0; e < values.size(); e++) values[e] = e * 0x9E3779B97F4A7C15ull + 0x8000000000000001ull;
            // exactly trlwes * 2N words, so a write past the table is the sanitizer's to catch
            std::vector<uint32_t> table((size_t)pl.trlwes * 2 * N, 0xDEADBEEFu);
            expect(tfhe_lookup_table_pack_slots(&P, values.data(), k, width, table.data()) == TFHE_OK, T, "status");
            std::vector<uint32_t> want(table.size(), 0u);
            for (size_t e = 0; e < values.size(); e++)
                for (uint32_t c = 0; c < width; c++)
                    want[(e >> pl.h) * 2 * N + N + (e & ((1u << pl.h) - 1)) * pl.stride + c] = (values[e] >> c) & 1 ? PLUS : MINUS;
            expect(table == want, T, "entry e in TRLWE e >> h at slot e & (2^h - 1); a = 0; unused coefficients 0");
        }
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "pack_slots argument checks";
        std::vector<uint32_t> table(2 * N);
        std::vector<uint64_t> v(256, 1);
        expect(tfhe_lookup_table_pack_slots(nullptr, v.data(), 8, 1, table.data()) == TFHE_ERR_INVALID, T, "null params");
        expect(tfhe_lookup_table_pack_slots(&P, nullptr, 8, 1, table.data()) == TFHE_ERR_INVALID, T, "null values");
        expect(tfhe_lookup_table_pack_slots(&P, v.data(), 8, 1, nullptr) == TFHE_ERR_INVALID, T, "null table");
        expect(tfhe_lookup_table_pack_slots(&P, v.data(), 8, 65, table.data()) == TFHE_ERR_INVALID, T, "width > 64");
        expect(tfhe_lookup_table_pack_slots(&P, v.data(), 8, 0, table.data()) == TFHE_ERR_INVALID, T, "width = 0");
        expect(tfhe_lookup_table_pack_slots(&P, v.data(), 0, 1, table.data()) == TFHE_ERR_INVALID, T, "k = 0");
        expect(tfhe_lookup_table_pack_slots(&P, v.data(), 23, 1, table.data()) == TFHE_ERR_INVALID, T, "v > 12");
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
