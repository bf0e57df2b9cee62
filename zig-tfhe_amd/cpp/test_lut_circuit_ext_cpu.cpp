// Stand-alone test of the extended nodes' host half (csrc/tfhe_cpu.cpp): plan_lut_circuit with an eta per
// node (a level's run grouped by eta, ordinary nodes ahead of select nodes inside each group, one numbering of
// the level's select nodes across the groups, consecutive output slots), that a plan without eta is the plan it
// was, every refusal, tfhe_lut_circuit_schedule_ext with its per-level group counts, and the identity the
// extended select node rests on: for 2m <= N every component of tfhe_lut_generate_ext is tfhe_lut_generate.
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
tfhe_params uint4() {
    tfhe_params p{};
    p.n = 820, p.N = 1024, p.nbit = 10, p.L = 1, p.bgbit = 22, p.basebit = 5, p.iks_t = 3;
    return p;
}

struct Circuit {
    size_t n_inputs;
    U term_off, term_wire, konst, lut, theta, sel_off, sel_wire, sel_konst, eta, out_wires;
    uint32_t m;
    const char *plan(tfhe::LutCircuitPlan &pl, size_t T = 8) const {
        const std::vector<int32_t> coef(term_wire.size(), 1);
        const tfhe::LutSelect sel{m, sel_off.data(), sel_wire.data(), sel_konst.data()};
        return tfhe::plan_lut_circuit(n_inputs, lut.size(), term_off.data(), term_wire.data(), coef.data(), konst.data(),
                                      lut.data(), T, out_wires.size(), out_wires.data(), pl,
                                      theta.empty() ? nullptr : theta.data(), sel_off.empty() ? nullptr : &sel,
                                      eta.empty() ? nullptr : eta.data());
    }
    int schedule(U &levels, uint32_t &depth, U &groups) const {
        levels.assign(lut.size(), 0), groups.assign(3 * lut.size(), 99);
        return tfhe_lut_circuit_schedule_ext(n_inputs, lut.size(), term_off.data(), term_wire.data(),
                                             theta.empty() ? nullptr : theta.data(), m,
                                             sel_off.empty() ? nullptr : sel_off.data(), sel_wire.data(),
                                             eta.empty() ? nullptr : eta.data(), levels.data(), &depth, groups.data());
    }
};

// 3 inputs (wires 0..2), m = 2, a set of 8 tables.
//   level 1: nodes 0, 1 ordinary eta = 2 (w3, w4); node 2 select eta = 2, entries (w0, const 9) (w5)
//   level 2: node 3 theta = 1 (w6, w7), node 4 select eta = 1, entries (w5, const 4) (w8), node 5 ordinary eta = 0 (w9),
//            node 6 select eta = 0, entries (w3, w4) (w10), node 7 ordinary eta = 1 (w11), node 8 ordinary eta = 2 (w12)
//   level 3: node 9 select eta = 1 over w7 + w11, entries an extended node's wire and an input wire (w12, w1) (w13)
Circuit mixed() {
    Circuit c;
    c.n_inputs = 3, c.m = 2;
    c.term_off = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11};
    c.term_wire = {0, 1, 2, 3, 4, 5, 3, 4, 5, 7, 11};
    c.konst = {10, 11, 12, 13, 14, 15, 16, 17, 18, 19};
    c.lut = {1, 0, 0, 7, 0, 5, 0, 3, 1, 0};
    c.theta = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0};
    c.sel_off = {0, 0, 0, 2, 2, 4, 4, 6, 6, 6, 8};
    c.sel_wire = {0, K, 5, K, 3, 4, 12, 1};
    c.sel_konst = {0, 9, 0, 4, 0, 0, 0, 0};
    c.eta = {2, 2, 2, 0, 1, 0, 0, 1, 2, 1};
    c.out_wires = {13, 6, 0};
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
        expect(pl.depth == 3 && pl.level == U({1, 1, 1, 2, 2, 2, 2, 2, 2, 3}), T, "levels");
        // level 2: eta 0 (ordinary 3, 5, select 6), eta 1 (ordinary 7, select 4), eta 2 (8)
        expect(pl.order == U({0, 1, 2, 3, 5, 6, 7, 4, 8, 9}), T, "evaluation order");
        expect(pl.first == U({0, 3, 9, 10}) && pl.ofirst == U({0, 3, 10, 11}), T, "level starts");
        expect(pl.neta == U({0, 0, 3, 3, 2, 1, 0, 1, 0}) && pl.nsel_eta == U({0, 0, 1, 1, 1, 0, 0, 1, 0}), T, "group counts");
        expect(pl.nsel == U({1, 2, 1}) && pl.sfirst == U({0, 1, 3, 4}), T, "select counts");
        expect(pl.eta == U({2, 2, 2, 0, 0, 0, 1, 1, 2, 1}) && pl.theta == U({0, 0, 0, 1, 0, 0, 0, 0, 0, 0}), T,
               "eta and theta in evaluation order");
        // wires 0..13 -> slots: inputs | w3 w4 w5 | w6 w7 w9 w10 w11 w8 w12 | w13
        expect(pl.slot == U({0, 1, 2, 3, 4, 5, 6, 7, 11, 8, 9, 10, 12, 13}), T, "consecutive output slots per level");
        // the level's select nodes are numbered in evaluation order across the groups: node 6 is 0, node 4 is 1
        expect(pl.tv_sel == U({1, 0, E | 0, 7, 5, E | 0, 3, E | 1, 1, E | 0}), T, "where each item's test vector comes from");
        // entries in pack order, select nodes 2 | 6, 4 | 9 over slots
        expect(pl.e_off == U({0, 1, 1, 2, 3, 4, 4, 5, 6}) && pl.e_src == U({0, 3, 4, 5, 12, 1}) &&
                   pl.e_konst == U({0, 9, 0, 0, 0, 4, 0, 0}),
               T, "entry descriptors");
        // the fan-out pairs of level 2 name the eta = 0 part only, by the node's index in its level
        expect(pl.fan == U({0, 0, 1, 0, 2, 0, 0, 0, 0, 1, 1, 0, 2, 0, 3, 0, 4, 0, 5, 0, 0, 0}), T, "fan-out pairs");
        expect(pl.out_slots == U({13, 6, 0}), T, "output slots");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "no eta is the old plan";
        Circuit c = mixed();
        c.eta.assign(c.lut.size(), 0);
        tfhe::LutCircuitPlan zero, none;
        expect(!c.plan(zero), T, "all-zero eta");
        c.eta.clear();
        expect(!c.plan(none), T, "no eta");
        expect(zero.order == none.order && zero.slot == none.slot && zero.off == none.off && zero.src == none.src &&
                   zero.tv_sel == none.tv_sel && zero.e_off == none.e_off && zero.e_src == none.e_src &&
                   zero.fan == none.fan && zero.nsel == none.nsel && zero.sfirst == none.sfirst && zero.neta == none.neta,
               T, "plans differ");
        // ordinary nodes, then select nodes, node order inside either: what the planner gave before
        expect(none.order == U({0, 1, 2, 3, 5, 7, 8, 4, 6, 9}), T, "a level's order without eta");
        expect(none.neta == U({3, 0, 0, 6, 0, 0, 1, 0, 0}) && none.nsel_eta == U({1, 0, 0, 2, 0, 0, 1, 0, 0}), T, "one group");
        expect(none.eta == U(10, 0u), T, "eta per node");
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
        refused([](Circuit &c) { c.eta[0] = 3; }, "eta = 3 on an ordinary node");
        refused([](Circuit &c) { c.eta[9] = 3; }, "eta = 3 on a select node");
        refused([](Circuit &c) { c.eta[3] = 1; }, "eta on a theta > 0 node");
        refused([](Circuit &c) { c.theta[7] = 1; }, "theta on an extended node");
        refused([](Circuit &c) { c.lut[0] = 2; }, "lut * 4 + 4 = 12 beyond a set of 8");
        refused([](Circuit &c) { c.lut[7] = 4; }, "lut * 2 + 2 = 10 beyond a set of 8");
        refused([](Circuit &c) { c.lut[3] = 0; }, "lut 1 at eta = 2 in a set of 7", 7);
        {
            Circuit c = mixed();
            c.lut[7] = 3, c.lut[3] = 6;
            expect(c.plan(pl, 8) == nullptr, T, "lut * 2 + 2 = 8: the last extended table of a set of 8");
        }
        // what the planner refused before
        refused([](Circuit &c) { c.lut[4] = 1; }, "lut on an extended select node");
        refused([](Circuit &c) { c.theta[2] = 1; }, "theta on a select node");
        refused([](Circuit &c) { c.sel_wire[6] = 13; }, "a select node's own wire as its entry");
        refused([](Circuit &c) { c.sel_off = {0, 0, 0, 1, 1, 3, 3, 5, 5, 5, 7}, c.sel_wire.pop_back(), c.sel_konst.pop_back(); },
                "an entry count of 1");
        refused([](Circuit &c) { c.m = 3; }, "m = 3");
        refused([](Circuit &c) { c.term_wire[10] = 13; }, "a forward term wire");
        refused([](Circuit &c) { c.lut[5] = 8; }, "a table index past the set");
        refused([](Circuit &c) { c.out_wires[0] = 14; }, "an output wire out of range");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "schedule entry";
        Circuit c = mixed();
        U levels, groups, sel_levels(10);
        uint32_t depth = 0, sdepth = 0;
        expect(c.schedule(levels, depth, groups) == TFHE_OK && depth == 3 && levels == U({1, 1, 1, 2, 2, 2, 2, 2, 2, 3}), T,
               "levels");
        groups.resize(9);
        expect(groups == U({0, 0, 3, 3, 2, 1, 0, 1, 0}), T, "group counts");
        // a level with only eta = 2 nodes and a theta > 0 node beside extended ones are levels 1 and 2 above
        Circuit n = c;
        n.eta.clear();
        expect(n.schedule(levels, depth, groups) == TFHE_OK &&
                   tfhe_lut_circuit_schedule_select(3, 10, c.term_off.data(), c.term_wire.data(), c.theta.data(), 2,
                                                    c.sel_off.data(), c.sel_wire.data(), sel_levels.data(), &sdepth) == TFHE_OK &&
                   levels == sel_levels && depth == sdepth,
               T, "eta = NULL is the select schedule");
        groups.resize(9);
        expect(groups == U({3, 0, 0, 6, 0, 0, 1, 0, 0}), T, "eta = NULL: one group per level");
        auto refused = [&](void (*edit)(Circuit &), const char *what) {
            Circuit e = mixed();
            edit(e);
            expect(e.schedule(levels, depth, groups) == TFHE_ERR_INVALID, T, what);
        };
        refused([](Circuit &e) { e.eta[1] = 3; }, "eta = 3");
        refused([](Circuit &e) { e.eta[3] = 2; }, "eta with theta");
        refused([](Circuit &e) { e.m = 4; }, "counts against another m");
        refused([](Circuit &e) { e.sel_wire[6] = 13; }, "an entry wire that is not earlier");
        expect(tfhe_lut_circuit_schedule_ext(3, 0, nullptr, nullptr, nullptr, 2, c.sel_off.data(), nullptr, nullptr, nullptr,
                                             nullptr, nullptr) == TFHE_OK,
               T, "zero nodes");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "E copies";
        const tfhe_params p = uint4();
        const size_t N = p.N;
        for (uint32_t eta : {1u, 2u})
            for (uint32_t m : {2u, 16u, 32u, 64u, 512u, 1024u, 2048u}) {
                const size_t Ec = (size_t)1 << eta;
                U f(m), ext(Ec * 2 * N), one(2 * N);
                for (uint32_t i = 0; i < m; i++) f[i] = (7 * i * i + 3 * i + 1) % m;
                expect(tfhe_lut_generate_ext(&p, eta, m, f.data(), ext.data()) == TFHE_OK &&
                           tfhe_lut_generate(&p, m, f.data(), one.data()) == TFHE_OK,
                       T, "status");
                bool all = true;
                for (size_t j = 0; j < Ec; j++) all &= !std::memcmp(ext.data() + j * 2 * N, one.data(), 2 * N * sizeof(uint32_t));
                expect(all == (2 * (size_t)m <= N), T, "every component equals the ordinary table exactly when 2m <= N");
            }
        expect(TFHE_GPU_ABI_VERSION == 7, T, "ABI version");
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
