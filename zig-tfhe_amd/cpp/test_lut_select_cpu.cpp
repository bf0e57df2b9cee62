// Stand-alone test of the select nodes' host half (csrc/tfhe_cpu.cpp): plan_lut_circuit with select
// nodes (levels, the ordinary-then-select order of a level, consecutive output slots, the entry
// descriptors in pack order, where each item's test vector comes from), every refusal of the planner,
// tfhe_lut_circuit_schedule_select, and the identity the definition rests on: tfhe_pack_tlwe of trivial
// ciphertexts leaves a = 0 and b[i*w] = c_i, so tfhe_lut_spread of it is tfhe_lut_generate's table.
// Links tfhe_cpu.o only — no HIP, no libtfhe_gpu.so — and builds and runs under the host sanitizers
// too (make cpu-check).  Exit status 0 = all passed.
#include "tfhe_cpu.hpp"

#include <cstdio>
#include <cstring>
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
constexpr uint32_t K = TFHE_LUT_ENTRY_CONST, E = tfhe::LUT_TV_EACH;
// UINT4 (n = 820) as far as these host entries read it
tfhe_params uint4() {
    tfhe_params p{};
    p.n = 820, p.N = 1024, p.nbit = 10, p.L = 1, p.bgbit = 22, p.basebit = 5, p.iks_t = 3;
    return p;
}
uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

// A circuit in the C ABI's arrays; plan() is nullptr or the planner's reason.
struct Circuit {
    size_t n_inputs;
    U term_off, term_wire, konst, lut, theta, sel_off, sel_wire, sel_konst, out_wires;
    uint32_t m;
    const char *plan(tfhe::LutCircuitPlan &pl, size_t T = 8) const {
        const std::vector<int32_t> coef(term_wire.size(), 1);
        const tfhe::LutSelect sel{m, sel_off.data(), sel_wire.data(), sel_konst.data()};
        return tfhe::plan_lut_circuit(n_inputs, lut.size(), term_off.data(), term_wire.data(), coef.data(), konst.data(),
                                      lut.data(), T, out_wires.size(), out_wires.data(), pl,
                                      theta.empty() ? nullptr : theta.data(), sel_off.empty() ? nullptr : &sel);
    }
};

// 2 inputs (wires 0, 1), m = 2.  Nodes: 0 ordinary over w0 (lut 3) -> w2; 1 select, x = w1, entries (w0, const 9)
// -> w3; 2 ordinary over w1 (lut 5) -> w4; 3 select, x = w2 + w4, entries (w4, w3) -> w5; 4 ordinary over w5
// (lut 1) -> w6; 5 select, x = w0, entries (const 4, w2) -> w7.  Levels 1 1 1 2 3 2.
Circuit mixed() {
    Circuit c;
    c.n_inputs = 2, c.m = 2;
    c.term_off = {0, 1, 2, 3, 5, 6, 7};
    c.term_wire = {0, 1, 1, 2, 4, 5, 0};
    c.konst = {10, 11, 12, 13, 14, 15};
    c.lut = {3, 0, 5, 0, 1, 0};
    c.sel_off = {0, 0, 2, 2, 4, 4, 6};
    c.sel_wire = {0, K, 4, 3, K, 2};
    c.sel_konst = {0, 9, 0, 0, 4, 0};
    c.out_wires = {7, 6, 0};
    return c;
}
}  // namespace

int main() {
    {
        const char *T = "plan";
        tfhe::LutCircuitPlan pl;
        const Circuit c = mixed();
        const char *why = c.plan(pl);
        expect(!why, T, why ? why : "");
        expect(pl.depth == 3 && pl.level == U({1, 1, 1, 2, 3, 2}), T, "levels");
        // a level's ordinary nodes ahead of its select nodes, node order inside either group
        expect(pl.order == U({0, 2, 1, 3, 5, 4}), T, "evaluation order");
        expect(pl.first == U({0, 3, 5, 6}) && pl.ofirst == pl.first, T, "level starts");
        expect(pl.nsel == U({1, 2, 0}) && pl.sfirst == U({0, 1, 3, 3}), T, "select counts");
        // wires 0..7 -> slots: inputs, then w2 w4 | w3, then w5 w7, then w6
        expect(pl.slot == U({0, 1, 2, 4, 3, 5, 7, 6}), T, "consecutive output slots per level");
        expect(pl.lut == U({3, 5, 0, 0, 0, 1}) && pl.konst == U({10, 12, 11, 13, 15, 14}), T, "per-node descriptors");
        expect(pl.tv_sel == U({3, 5, E | 0, E | 0, E | 1, 1}), T, "where each item's test vector comes from");
        // x terms over slots, per level: (w0) (w1) (w1) | (w2 + w4) (w0) | (w5)
        expect(pl.off == U({0, 1, 2, 3, 3, 5, 6, 6, 7}) && pl.src == U({0, 1, 1, 2, 3, 0, 5}), T, "x terms");
        // entries in pack order, select nodes 1, 3, 5: (w0, 9) (w4, w3) (4, w2) over slots
        expect(pl.e_off == U({0, 1, 1, 2, 3, 3, 4}) && pl.e_src == U({0, 3, 4, 2}) && pl.e_konst == U({0, 9, 0, 0, 4, 0}), T,
               "entry descriptors");
        expect(pl.out_slots == U({6, 7, 0}), T, "output slots");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "plan with a multi-output node";
        // 1 input; node 0 theta 1 -> w1 w2; node 1 select x = w0, entries (w1, w2) -> w3; node 2 theta 1 over w0 -> w4 w5;
        // node 3 select x = w0, entries (const, const) -> w6: level 1 holds nodes 0, 2, 3 (ordinary first), level 2 node 1
        Circuit c;
        c.n_inputs = 1, c.m = 2;
        c.term_off = {0, 1, 2, 3, 4};
        c.term_wire = {0, 0, 0, 0};
        c.konst = {0, 0, 0, 0};
        c.lut = {2, 0, 2, 0};
        c.theta = {1, 0, 1, 0};
        c.sel_off = {0, 0, 2, 2, 4};
        c.sel_wire = {1, 2, K, K};
        c.sel_konst = {0, 0, 7, 8};
        c.out_wires = {3, 6};
        tfhe::LutCircuitPlan pl;
        const char *why = c.plan(pl);
        expect(!why, T, why ? why : "");
        expect(pl.level == U({1, 2, 1, 1}) && pl.order == U({0, 2, 3, 1}), T, "order");
        expect(pl.ofirst == U({0, 5, 6}) && pl.nsel == U({1, 1}), T, "output runs");
        expect(pl.slot == U({0, 1, 2, 6, 3, 4, 5}), T, "slots: the level's select outputs behind its fan-outs");
        expect(pl.fan == U({0, 0, 0, 1, 1, 0, 1, 1, 2, 0, 0, 0}), T, "fan-out pairs");
        expect(pl.tv_sel == U({2, 2, E | 0, E | 0}), T, "test vector sources");
        expect(pl.e_off == U({0, 0, 0, 1, 2}) && pl.e_src == U({1, 2}) && pl.e_konst == U({7, 8, 0, 0}), T, "entries");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "no select nodes is the old plan";
        Circuit c = mixed();
        tfhe::LutCircuitPlan with, without;
        c.sel_off.assign(c.lut.size() + 1, 0), c.sel_wire.clear(), c.sel_konst.clear();
        expect(!c.plan(with), T, "empty descriptors");
        c.sel_off.clear();
        expect(!c.plan(without), T, "no descriptors");
        expect(with.order == without.order && with.slot == without.slot && with.off == without.off &&
                   with.tv_sel == without.lut && without.tv_sel == without.lut && with.nsel == U({0, 0, 0}),
               T, "plans differ");
        expect(without.order == U({0, 1, 2, 5, 3, 4}), T, "node order inside a level");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "refusals";
        tfhe::LutCircuitPlan pl;
        auto refused = [&](void (*edit)(Circuit &), const char *what, size_t Tset = 8) {
            Circuit c = mixed();
            edit(c);
            expect(c.plan(pl, Tset) != nullptr, T, what);
        };
        expect(mixed().plan(pl) == nullptr, T, "the unedited circuit");
        refused([](Circuit &c) { c.sel_off = {0, 0, 1, 1, 3, 3, 5}, c.sel_wire.pop_back(), c.sel_konst.pop_back(); },
                "an entry count of 1");
        refused([](Circuit &c) { c.sel_off = {0, 0, 4, 4, 4, 4, 6}; }, "an entry count of 2m");
        refused([](Circuit &c) { c.sel_wire[0] = 3; }, "a select node's own wire as its entry");
        refused([](Circuit &c) { c.sel_wire[0] = 6; }, "a forward entry wire");
        refused([](Circuit &c) { c.sel_wire[0] = 8; }, "an entry wire past the last");
        refused([](Circuit &c) { c.theta = {0, 1, 0, 0, 0, 0}; }, "theta on a select node");
        refused([](Circuit &c) { c.lut[1] = 2; }, "lut on a select node");
        refused([](Circuit &c) { c.sel_off[0] = 1; }, "sel_off not from 0");
        refused([](Circuit &c) { c.sel_off = {0, 0, 2, 2, 4, 2, 4}; }, "sel_off not monotone");
        refused([](Circuit &c) { c.m = 3; }, "m = 3");
        refused([](Circuit &c) { c.m = 1; }, "m = 1");
        refused([](Circuit &c) { c.term_wire[3] = 5; }, "a forward term wire");
        refused([](Circuit &c) { c.lut[0] = 8; }, "a table index past the set");
        refused([](Circuit &c) { c.out_wires[0] = 8; }, "an output wire out of range");
        refused([](Circuit &) {}, "a set of 2^31 tables", (size_t)1 << 31);
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "schedule entry";
        const Circuit c = mixed();
        U levels(6), multi(6);
        uint32_t depth = 0, mdepth = 0;
        expect(tfhe_lut_circuit_schedule_select(2, 6, c.term_off.data(), c.term_wire.data(), nullptr, 2, c.sel_off.data(),
                                                c.sel_wire.data(), levels.data(), &depth) == TFHE_OK &&
                   levels == U({1, 1, 1, 2, 3, 2}) && depth == 3,
               T, "levels");
        expect(tfhe_lut_circuit_schedule_select(2, 6, c.term_off.data(), c.term_wire.data(), nullptr, 4, c.sel_off.data(),
                                                c.sel_wire.data(), levels.data(), &depth) == TFHE_ERR_INVALID,
               T, "counts against another m");
        const U theta(6, 0);
        expect(tfhe_lut_circuit_schedule_select(2, 6, c.term_off.data(), c.term_wire.data(), theta.data(), 0, nullptr,
                                                nullptr, levels.data(), &depth) == TFHE_OK &&
                   tfhe_lut_circuit_schedule_multi(2, 6, c.term_off.data(), c.term_wire.data(), theta.data(), multi.data(),
                                                   &mdepth) == TFHE_OK &&
                   levels == multi && depth == mdepth,
               T, "sel_off = NULL is the multi schedule");
        expect(tfhe_lut_circuit_schedule_select(2, 0, nullptr, nullptr, nullptr, 2, c.sel_off.data(), nullptr, nullptr,
                                                nullptr) == TFHE_OK,
               T, "zero nodes");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "trivial pack";
        const tfhe_params p = uint4();
        const size_t N = p.N, n1 = p.n + 1;
        const uint32_t basebit = 5, t = 3;
        // a packing key's shape with seeded words in every row but the k = 0 rows, which are zero in every key
        U rows((size_t)p.n * t * (1u << basebit) * 2 * N);
        uint32_t s = 77;
        for (size_t r = 0; r < rows.size() / (2 * N); r++)
            for (size_t i = 0; i < 2 * N; i++) rows[r * 2 * N + i] = r % (1u << basebit) ? lcg(s) : 0u;
        for (uint32_t m : {2u, 4u, 16u}) {
            const uint32_t w = (uint32_t)N / m, off = (uint32_t)N / (2 * m);
            U f(m), in(m * n1, 0u), coef(m), packed(2 * N, 1), want(2 * N, 0u), tv(2 * N), gen(2 * N);
            for (uint32_t i = 0; i < m; i++) {
                f[i] = (7 * i * i + 3 * i + 1) % m;  // non-monotone
                coef[i] = i * w;
                // Encoder.new(m).encode(v) = v / (2m) of the torus, exact for these m
                in[i * n1 + p.n] = want[N + i * w] = f[i] * (uint32_t)(0x100000000ull / (2 * m));
            }
            expect(tfhe_pack_tlwe(&p, rows.data(), basebit, t, in.data(), coef.data(), m, packed.data(), 1) == TFHE_OK, T,
                   "pack status");
            expect(packed == want, T, "the pack of trivial inputs is not (a = 0, b[i*w] = c_i)");
            expect(tfhe_lut_spread(&p, packed.data(), w, 2 * (uint32_t)N - off, tv.data(), 1) == TFHE_OK &&
                       tfhe_lut_generate(&p, m, f.data(), gen.data()) == TFHE_OK && tv == gen,
                   T, "spread of the pack is not the generator's table");
        }
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
