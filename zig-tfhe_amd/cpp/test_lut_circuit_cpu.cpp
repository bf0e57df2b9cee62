// Stand-alone test of the LUT-circuit planner (csrc/tfhe_cpu.cpp): ASAP levels,
// slot assignment in level order, the per-level CSR descriptors rewritten to slots,
// and the descriptor checks of the batch entry.  Links tfhe_cpu.o only — no HIP, no
// libtfhe_gpu.so — and builds and runs under the host sanitizers too (make
// cpu-check).  Exit status 0 = all passed.
#include "tfhe_cpu.hpp"

#include <cstdio>
#include <string>
#include <vector>

namespace {
int failures = 0;
void expect(bool ok, const char *test, const char *what) {
    if (!ok) {
        std::printf("FAIL %s: %s\n", test, what);
        failures++;
    }
}
using U = std::vector<uint32_t>;
using I = std::vector<int32_t>;
}  // namespace

int main() {
    using namespace tfhe;
    {
        // 2 inputs (wires 0, 1); nodes (wires 2..6):
        //   n0 = f(w0 + 2 w1)          level 1
        //   n1 = f(n0 - w0)            level 2
        //   n2 = f(konst)              level 1  (no terms)
        //   n3 = f(n1 + n1 + 3 n2)     level 3  (a wire used twice by one node)
        //   n4 = f(w1)                 level 1
        const char *T = "plan";
        const U off{0, 2, 4, 4, 7, 8}, wire{0, 1, 2, 0, 3, 3, 4, 1}, konst{0, 5, 77, 0, 9}, lut{0, 1, 2, 1, 0};
        const I coef{1, 2, 1, -1, 1, 1, 3, 1};
        const U outs{6, 1, 5, 2};  // a node, an input wire, the deepest node, a level-1 node
        LutCircuitPlan pl;
        const char *why = plan_lut_circuit(2, 5, off.data(), wire.data(), coef.data(), konst.data(), lut.data(), 3,
                                           outs.size(), outs.data(), pl);
        expect(why == nullptr, T, why ? why : "");
        expect(pl.depth == 3 && pl.level == U{1, 2, 1, 3, 1}, T, "ASAP levels");
        expect(pl.first == U{0, 3, 4, 5}, T, "level boundaries");
        expect(pl.order == U{0, 2, 4, 1, 3}, T, "evaluation order: by level, node order inside a level");
        expect(pl.slot == U{0, 1, 2, 5, 3, 6, 4}, T, "slots: inputs, then the nodes in evaluation order");
        // level 1: n0 (w0, w1), n2 (), n4 (w1); level 2: n1 (n0 -> slot 2, w0); level 3: n3 (n1 -> 5, 5, n2 -> 3)
        expect(pl.off == U{0, 2, 2, 3, 3, 5, 5, 8}, T, "per-level CSR offsets, one more entry than nodes per level");
        expect(pl.src == U{0, 1, 1, 2, 0, 5, 5, 3}, T, "sources rewritten to slots");
        expect(pl.coef == I{1, 2, 1, 1, -1, 1, 1, 3}, T, "coefficients follow their terms");
        expect(pl.konst == U{0, 77, 9, 5, 0} && pl.lut == U{0, 2, 0, 1, 1}, T, "konst / lut in evaluation order");
        expect(pl.out_slots == U{4, 1, 6, 2}, T, "output slots (an input wire keeps its own)");
        // every source of a level lies below that level's first slot: a launch never reads what it writes
        bool below = true;
        for (uint32_t lv = 1; lv <= pl.depth; lv++) {
            const uint32_t *o = pl.off.data() + pl.first[lv - 1] + (lv - 1);
            const uint32_t nb = pl.first[lv] - pl.first[lv - 1];
            for (uint32_t k = o[0]; k < o[nb]; k++) below = below && pl.src[k] < 2 + pl.first[lv - 1];
        }
        expect(below, T, "a level reads earlier slots only");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "plan edge cases";
        LutCircuitPlan pl;
        const U outs{0, 0};
        expect(plan_lut_circuit(1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 2, outs.data(), pl) == nullptr, T,
               "no nodes");
        expect(pl.depth == 0 && pl.off.empty() && pl.out_slots == U{0, 0} && pl.first == U{0}, T, "empty plan");
        const U off{0, 1}, wire{0}, konst{0}, lut{2};
        const I coef{1};
        expect(plan_lut_circuit(1, 1, off.data(), wire.data(), coef.data(), konst.data(), lut.data(), 2, 0, nullptr, pl) !=
                   nullptr,
               T, "table index >= T");
        const U lut_ok{1}, bad_out{2};
        expect(plan_lut_circuit(1, 1, off.data(), wire.data(), coef.data(), konst.data(), lut_ok.data(), 2, 1,
                                bad_out.data(), pl) != nullptr,
               T, "output wire out of range");
        const U self{1};
        expect(plan_lut_circuit(1, 1, off.data(), self.data(), coef.data(), konst.data(), lut_ok.data(), 2, 0, nullptr,
                                pl) != nullptr,
               T, "self reference");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "schedule";
        uint32_t depth = 99;
        U levels(3, 99);
        const U off{0, 1, 2, 3}, chain{0, 1, 2};
        expect(tfhe_lut_circuit_schedule(1, 3, off.data(), chain.data(), levels.data(), &depth) == TFHE_OK, T, "chain");
        expect(levels == U{1, 2, 3} && depth == 3, T, "chain levels");
        const U fwd{0, 3, 2};  // node 1 reads wire 3 = node 2
        expect(tfhe_lut_circuit_schedule(1, 3, off.data(), fwd.data(), levels.data(), &depth) == TFHE_ERR_INVALID, T,
               "forward reference");
        const U off1{1, 1, 2, 3}, down{0, 2, 1, 3};
        expect(tfhe_lut_circuit_schedule(1, 3, off1.data(), chain.data(), levels.data(), &depth) == TFHE_ERR_INVALID, T,
               "term_off[0] != 0");
        expect(tfhe_lut_circuit_schedule(1, 3, down.data(), chain.data(), levels.data(), &depth) == TFHE_ERR_INVALID, T,
               "term_off not monotone");
        expect(tfhe_lut_circuit_schedule(4, 0, nullptr, nullptr, nullptr, &depth) == TFHE_OK && depth == 0, T, "empty");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "batch descriptor checks";
        const U off{0, 2, 2, 3}, src{0, 7, 3}, lut{0, 4, 1};
        expect(check_lut_nodes(3, 8, 5, off.data(), src.data(), lut.data()) == nullptr, T, "valid");
        expect(check_lut_nodes(3, 7, 5, off.data(), src.data(), lut.data()) != nullptr, T, "source >= P");
        expect(check_lut_nodes(3, 8, 4, off.data(), src.data(), lut.data()) != nullptr, T, "lut >= T");
        const U off1{1, 2, 2, 3}, down{0, 2, 1, 3};
        expect(check_lut_nodes(3, 8, 5, off1.data(), src.data(), lut.data()) != nullptr, T, "term_off[0] != 0");
        expect(check_lut_nodes(3, 8, 5, down.data(), src.data(), lut.data()) != nullptr, T, "term_off not monotone");
        expect(check_lut_nodes(0, 0, 1, nullptr, nullptr, nullptr) == nullptr, T, "empty batch");
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
