// Stand-alone test of the multi-output LUT bootstrap's host half (csrc/tfhe_cpu.cpp):
// round_theta (tfhe_lut_round_tlwe), the interleaved test vector (tfhe_lut_interleave)
// and the planner's multi-output form (wire numbering over sum 2^theta outputs, levels,
// slots, fan-out pairs).  Links tfhe_cpu.o only — no HIP, no libtfhe_gpu.so — and builds
// and runs under the host sanitizers too (make cpu-check).  Exit status 0 = all passed.
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
// UINT4 (n = 820) as far as these host entries read it
tfhe_params uint4() {
    tfhe_params p{};
    p.n = 820, p.N = 1024, p.nbit = 10, p.L = 1, p.bgbit = 22, p.basebit = 5, p.iks_t = 3;
    return p;
}
uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
}  // namespace

int main() {
    using namespace tfhe;
    const tfhe_params p = uint4();
    {
        const char *T = "round";
        const size_t B = 3, w = p.n + 1;
        U in(B * w), out(B * w, 1);
        uint32_t s = 7;
        for (auto &v : in) v = lcg(s);
        in[0] = 0xFFFFFFFFu, in[1] = 0, in[2] = (1u << 21) - 1, in[3] = 1u << 21, in[4] = 0xFFDFFFFFu;
        for (uint32_t theta = 1; theta <= TFHE_LUT_MULTI_MAX_LOG; theta++) {
            expect(tfhe_lut_round_tlwe(&p, theta, in.data(), out.data(), B) == TFHE_OK, T, "status");
            const uint32_t sh = 21 + theta;
            expect(lut_round_shift(p, theta) == sh, T, "s = 32 - (nbit + 1) + theta");
            bool multiple = true, switched = true, nearest = true;
            for (size_t i = 0; i < in.size(); i++) {
                multiple = multiple && out[i] % (1u << sh) == 0;
                switched = switched && ((out[i] + (1u << 20)) >> 21) == (out[i] >> 21) && (out[i] >> 21) % (1u << theta) == 0;
                const uint32_t d = out[i] - in[i], e = in[i] - out[i];  // wrapping distance either way
                nearest = nearest && (d <= (1u << (sh - 1)) || e < (1u << (sh - 1)));
            }
            expect(multiple, T, "every word a multiple of 2^(21 + theta)");
            expect(switched, T, "the mod switch returns w >> 21, a multiple of 2^theta");
            expect(nearest, T, "the nearest multiple");
            expect(out[0] == 0 && out[1] == 0, T, "0xFFFFFFFF wraps to 0");
        }
        expect(lut_round_shift(p, 0) == 0, T, "theta = 0: no shift");
        expect(tfhe_lut_round_tlwe(&p, 0, in.data(), out.data(), B) == TFHE_OK && out == in, T, "theta = 0 is the identity");
        expect(tfhe_lut_round_tlwe(&p, 4, in.data(), out.data(), B) == TFHE_ERR_INVALID, T, "theta = 4 is refused");
        expect(tfhe_lut_round_tlwe(&p, 1, nullptr, out.data(), B) == TFHE_ERR_INVALID, T, "null input");
        U same = in;
        expect(tfhe_lut_round_tlwe(&p, 2, same.data(), same.data(), B) == TFHE_OK, T, "in place");
        tfhe_lut_round_tlwe(&p, 2, in.data(), out.data(), B);
        expect(same == out, T, "in place gives the same words");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "interleave";
        const size_t N = p.N;
        for (uint32_t theta = 0; theta <= TFHE_LUT_MULTI_MAX_LOG; theta++) {
            const size_t nu = (size_t)1 << theta;
            U tv(nu * 2 * N), out(2 * N, 0);
            uint32_t s = 11 + theta;
            for (auto &v : tv) v = lcg(s);
            expect(tfhe_lut_interleave(&p, tv.data(), theta, out.data()) == TFHE_OK, T, "status");
            bool ok = true;
            for (size_t h = 0; h < 2; h++)
                for (size_t q = 0; q < N; q++) ok = ok && out[h * N + q] == tv[(q % nu) * 2 * N + h * N + (q - q % nu)];
            expect(ok, T, "TV[h][q] = tv_{q mod nu}[h][q - q mod nu]");
            if (theta == 0) expect(out == tv, T, "theta = 0 copies the table");
        }
        U tv(2 * N), out(2 * N);
        expect(tfhe_lut_interleave(&p, tv.data(), 4, out.data()) == TFHE_ERR_INVALID, T, "theta = 4 is refused");
        std::printf("ok   %s\n", T);
    }
    // 2 inputs (wires 0, 1); thetas (0, 1, 0, 2, 1) -> 1, 2, 1, 4, 2 outputs, first wires 2, 3, 5, 6, 10:
    //   n0 = f(w0 + w1)       wire 2        level 1
    //   n1 = f(n0)            wires 3, 4    level 2
    //   n2 = f(w0)            wire 5        level 1
    //   n3 = f(n1[1] + n2)    wires 6..9    level 3
    //   n4 = f(n0 - w1)       wires 10, 11  level 2
    const U off{0, 2, 3, 4, 6, 8}, wire{0, 1, 2, 0, 4, 5, 2, 1}, konst{0, 5, 77, 0, 9}, lut{0, 1, 2, 1, 0};
    const I coef{1, 1, 1, 1, 1, 1, 1, -1};
    const U theta{0, 1, 0, 2, 1};
    {
        const char *T = "multi-output plan";
        const U outs{11, 1, 6, 9, 3, 5};
        LutCircuitPlan pl;
        const char *why = plan_lut_circuit(2, 5, off.data(), wire.data(), coef.data(), konst.data(), lut.data(), 3,
                                           outs.size(), outs.data(), pl, theta.data());
        expect(why == nullptr, T, why ? why : "");
        expect(pl.depth == 3 && pl.level == U{1, 2, 1, 3, 2}, T, "levels: a wire's level is its node's");
        expect(pl.first == U{0, 2, 4, 5}, T, "node boundaries of the levels");
        expect(pl.ofirst == U{0, 2, 6, 10}, T, "output-slot boundaries of the levels");
        expect(pl.order == U{0, 2, 1, 4, 3}, T, "evaluation order");
        expect(pl.slot == U{0, 1, 2, 4, 5, 3, 8, 9, 10, 11, 6, 7}, T, "wire -> slot over the sum of outputs");
        expect(pl.theta == U{0, 0, 1, 1, 2}, T, "theta in evaluation order");
        expect(pl.fan == U{0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 2, 0, 3}, T,
               "(node in level, coefficient) per output slot");
        expect(pl.off == U{0, 2, 3, 3, 4, 6, 6, 8}, T, "per-level CSR offsets");
        expect(pl.src == U{0, 1, 0, 2, 2, 1, 5, 3}, T, "sources rewritten to slots");
        expect(pl.coef == I{1, 1, 1, 1, 1, -1, 1, 1}, T, "coefficients follow their terms");
        expect(pl.konst == U{0, 77, 5, 9, 0} && pl.lut == U{0, 2, 1, 0, 1}, T, "konst / lut in evaluation order");
        expect(pl.out_slots == U{7, 1, 8, 11, 4, 3}, T, "output slots");
        bool below = true;  // a level reads slots below its own run of outputs only
        for (uint32_t lv = 1; lv <= pl.depth; lv++) {
            const uint32_t *o = pl.off.data() + pl.first[lv - 1] + (lv - 1);
            const uint32_t nb = pl.first[lv] - pl.first[lv - 1];
            for (uint32_t k = o[0]; k < o[nb]; k++) below = below && pl.src[k] < 2 + pl.ofirst[lv - 1];
        }
        expect(below, T, "a level reads earlier slots only");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "multi-output checks";
        LutCircuitPlan pl;
        auto plan = [&](const U &w, const U &th) {
            return plan_lut_circuit(2, 5, off.data(), w.data(), coef.data(), konst.data(), lut.data(), 3, 0, nullptr, pl,
                                    th.data());
        };
        U own = wire;
        own[2] = 3;  // n1 reads its own first output wire
        expect(plan(own, theta) != nullptr, T, "a node reading its own first wire");
        own[2] = 4;  // ... its second
        expect(plan(own, theta) != nullptr, T, "a node reading its own second wire");
        own = wire, own[4] = 9;  // n3 reads its own last wire
        expect(plan(own, theta) != nullptr, T, "a node reading its own last wire");
        own = wire, own[4] = 10;  // n3 reads n4's wire: forward
        expect(plan(own, theta) != nullptr, T, "a forward reference");
        own = wire, own[4] = 3;  // n3 reads n1's first wire: fine
        expect(plan(own, theta) == nullptr, T, "an earlier node's other output");
        U big = theta;
        big[2] = 4;
        expect(plan(wire, big) != nullptr, T, "theta = 4");
        uint32_t depth = 0;
        U levels(5, 99);
        expect(tfhe_lut_circuit_schedule_multi(2, 5, off.data(), wire.data(), theta.data(), levels.data(), &depth) == TFHE_OK &&
                   levels == U{1, 2, 1, 3, 2} && depth == 3,
               T, "schedule_multi");
        expect(tfhe_lut_circuit_schedule_multi(2, 5, off.data(), wire.data(), big.data(), levels.data(), &depth) ==
                   TFHE_ERR_INVALID,
               T, "schedule_multi refuses theta = 4");
        std::printf("ok   %s\n", T);
    }
    {
        // theta = NULL and all-zero thetas give the single-output plan
        const char *T = "theta = NULL";
        const U off1{0, 2, 4, 4, 7, 8}, wire1{0, 1, 2, 0, 3, 3, 4, 1}, outs{6, 1, 5, 2}, zero(5, 0);
        const I coef1{1, 2, 1, -1, 1, 1, 3, 1};
        LutCircuitPlan a, b, c;
        expect(plan_lut_circuit(2, 5, off1.data(), wire1.data(), coef1.data(), konst.data(), lut.data(), 3, outs.size(),
                                outs.data(), a) == nullptr, T, "existing signature");
        expect(plan_lut_circuit(2, 5, off1.data(), wire1.data(), coef1.data(), konst.data(), lut.data(), 3, outs.size(),
                                outs.data(), b, nullptr) == nullptr, T, "NULL");
        expect(plan_lut_circuit(2, 5, off1.data(), wire1.data(), coef1.data(), konst.data(), lut.data(), 3, outs.size(),
                                outs.data(), c, zero.data()) == nullptr, T, "all zero");
        for (const LutCircuitPlan *q : {&b, &c})
            expect(q->depth == a.depth && q->level == a.level && q->first == a.first && q->order == a.order &&
                       q->slot == a.slot && q->off == a.off && q->src == a.src && q->coef == a.coef && q->konst == a.konst &&
                       q->lut == a.lut && q->out_slots == a.out_slots && q->ofirst == a.first && q->theta == zero,
                   T, "the same plan");
        expect(a.slot == U{0, 1, 2, 5, 3, 6, 4} && a.ofirst == a.first, T, "the existing plan's slots");
        uint32_t d0 = 0, d1 = 0;
        U l0(5), l1(5);
        expect(tfhe_lut_circuit_schedule(2, 5, off1.data(), wire1.data(), l0.data(), &d0) == TFHE_OK &&
                   tfhe_lut_circuit_schedule_multi(2, 5, off1.data(), wire1.data(), nullptr, l1.data(), &d1) == TFHE_OK &&
                   l0 == l1 && d0 == d1,
               T, "schedule_multi(NULL) is schedule");
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
