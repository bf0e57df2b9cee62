// A 16-bit "a < b" on TRGSW-encrypted bits through the host-side mirror (tfhe.hpp: CmuxGraph,
// cmuxGraph): the comparator's decision diagram of 47 CMUXes over the trivial leaves false / true,
// one call for all pairs, the results extracted and key-switched; they decrypt to a < b and go
// into a gate like any other TLWELv0.  Runs on one MI355X; exit status 0 = all passed.
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
    uint64_t seed = 1200;
    const uint32_t nbits = 16;
    const uint32_t pairs[4][2] = {{0x1234, 0x1235}, {0xBEEF, 0xBEEF}, {0x8000, 0x7FFF}, {0x0000, 0xFFFF}};

    const CmuxGraph g = CmuxGraph::lessThan(nbits);
    const CmuxGraph::Plan plan = g.plan(P.N);
    {
        const char *T = "lessThan(16): plan";
        expect(g.var.size() == 3 * nbits - 1 && g.roots.size() == 1, T, "3 nodes per bit pair, less one");
        expect(plan.depth == 2 * nbits, T, "two levels per bit pair");
        expect(plan.nSlots <= 8, T, "slots by the diagram's width, not its size");
        std::printf("ok   %s: %zu nodes, depth %u, %u slots\n", T, g.var.size(), plan.depth, plan.nSlots);
    }
    // selector 32 q + 2 i encrypts bit 15 - i of a_q, selector 32 q + 2 i + 1 that bit of b_q
    std::vector<double> fft;
    std::vector<uint32_t> addr;
    for (uint32_t q = 0; q < 4; q++)
        for (uint32_t i = 0; i < nbits; i++)
            for (uint32_t side = 0; side < 2; side++) {
                const Torus bit = (pairs[q][side] >> (nbits - 1 - i)) & 1;
                const TRGSWLv1FFT t = TRGSWLv1FFT::encryptTorus(bit, P.alpha_bsk, sk.key_lv1, ck, seed++);
                fft.insert(fft.end(), t.fft.begin(), t.fft.end());
                addr.push_back((uint32_t)addr.size());
            }
    const TrgswSet set(ck, fft, 4 * 2 * nbits);
    {
        const char *T = "lessThan(16): 4 pairs";
        const std::vector<TLWELv0> lt = cmuxGraph(ck, set, addr, g, CmuxGraph::boolLeaves(P));
        expect(lt.size() == 4, T, "one result per pair");
        for (uint32_t q = 0; q < 4 && q < lt.size(); q++)
            expect(sk.decryptBool(lt[q]) == (pairs[q][0] < pairs[q][1]), T, "a result decrypts to something else than a < b");
        // gate inputs: (a0 < b0) AND (a3 < b3) = 1, (a0 < b0) AND (a1 < b1) = 0
        const Gates gates;
        expect(sk.decryptBool(gates.andGate(lt[0], lt[3], ck)), T, "AND of two true results");
        expect(!sk.decryptBool(gates.andGate(lt[0], lt[1], ck)), T, "AND of a true and a false result");
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
