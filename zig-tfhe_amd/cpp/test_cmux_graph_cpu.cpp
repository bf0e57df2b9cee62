// Stand-alone test of the CMUX graphs' host half (csrc/tfhe_cpu.cpp): tfhe_cmux_graph_plan on
// pseudo-random graphs (levels against the longest path, the slot assignment replayed level by
// level), the comparator's footprint, and every refusal.  Links tfhe_cpu.o only — no HIP, no
// libtfhe_gpu.so — and builds and runs under the host sanitizers too (make cpu-check).
// Exit status 0 = all passed.
#include "tfhe_cpu.hpp"

#include <algorithm>
#include <cstdio>
#include <set>
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
constexpr uint32_t N = 1024;
uint32_t lcg(uint32_t &s) { return (s = s * 1664525u + 1013904223u) >> 8; }

struct Graph {
    uint32_t nL = 1, k = 1;
    U var, lo, hi, rlo, rhi, roots;
    uint32_t V() const { return (uint32_t)var.size(); }
    void node(uint32_t v, uint32_t l, uint32_t h, uint32_t rl = 0, uint32_t rh = 0) {
        var.push_back(v), lo.push_back(l), hi.push_back(h), rlo.push_back(rl), rhi.push_back(rh);
    }
    int plan(U &level, U &slot, uint32_t &depth, uint32_t &n_slots) const {
        level.assign(V() + 1, 0xABABABABu), slot.assign(V() + 1, 0xABABABABu);  // one word more: nothing is written past V
        return tfhe_cmux_graph_plan(nL, V(), k, var.data(), lo.data(), hi.data(), rlo.data(), rhi.data(), (uint32_t)roots.size(),
                                    roots.data(), N, level.data(), slot.data(), &depth, &n_slots);
    }
};

Graph random_graph(uint32_t seed) {
    uint32_t s = seed * 2654435761u + 1;
    Graph g;
    g.nL = 1 + lcg(s) % 4, g.k = 1 + lcg(s) % 6;
    const uint32_t V = lcg(s) % 41;
    for (uint32_t v = 0; v < V; v++) {
        const uint32_t ids = g.nL + v;
        // even seeds: children among the last few values (deep graphs); odd: anywhere (wide ones)
        auto pick = [&] { return seed % 2 ? lcg(s) % ids : ids - 1 - std::min(lcg(s) % 4, ids - 1); };
        g.node(lcg(s) % g.k, pick(), pick(), lcg(s) % (2 * N + 1), lcg(s) % (2 * N + 1));
    }
    for (uint32_t r = lcg(s) % 5; r > 0; r--) g.roots.push_back(lcg(s) % (g.nL + V));
    return g;
}

// The level-by-level schedule with the slots' occupants: a level reads its children (each still in its slot),
// then writes; no slot is written in a level that reads it, and the roots are in their slots at the end.
bool replay(const Graph &g, const U &level, const U &slot, uint32_t depth, uint32_t n_slots) {
    std::vector<int64_t> held(n_slots, -1);
    for (uint32_t l = 1; l <= depth; l++) {
        std::set<uint32_t> read, written;
        bool any = false;
        for (uint32_t v = 0; v < g.V(); v++) {
            if (level[v] != l) continue;
            any = true;
            for (uint32_t c : {g.lo[v], g.hi[v]}) {
                if (c < g.nL) continue;
                if (slot[c - g.nL] >= n_slots || held[slot[c - g.nL]] != (int64_t)(c - g.nL)) return false;
                read.insert(slot[c - g.nL]);
            }
        }
        if (!any) return false;
        for (uint32_t v = 0; v < g.V(); v++) {
            if (level[v] != l) continue;
            if (slot[v] >= n_slots || read.count(slot[v]) || !written.insert(slot[v]).second) return false;
            held[slot[v]] = v;
        }
    }
    for (uint32_t r : g.roots)
        if (r >= g.nL && held[slot[r - g.nL]] != (int64_t)(r - g.nL)) return false;
    return true;
}
}  // namespace

int main() {
    {
        const char *T = "plan: 200 graphs";
        for (uint32_t seed = 0; seed < 200; seed++) {
            const Graph g = random_graph(seed);
            U level, slot;
            uint32_t depth = 99, n_slots = 99;
            expect(g.plan(level, slot, depth, n_slots) == TFHE_OK, T, "a valid graph is refused");
            uint32_t deepest = 0, top = 0;
            bool ok = true;
            for (uint32_t v = 0; v < g.V(); v++) {
                uint32_t l = 0;
                for (uint32_t c : {g.lo[v], g.hi[v]})
                    if (c >= g.nL) l = std::max(l, level[c - g.nL]);
                ok = ok && level[v] == l + 1;
                deepest = std::max(deepest, level[v]);
                top = std::max(top, slot[v] + 1);
            }
            expect(ok, T, "a level is not 1 + the deepest non-leaf child's");
            expect(depth == deepest && n_slots == top, T, "depth or n_slots");
            expect(level[g.V()] == 0xABABABABu && slot[g.V()] == 0xABABABABu, T, "written past V entries");
            expect(replay(g, level, slot, depth, n_slots), T, "the replayed schedule loses a value");
        }
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "plan: the comparator's footprint";
        for (uint32_t nbits : {8u, 32u}) {
            Graph g;
            g.nL = 2, g.k = 2 * nbits;
            uint32_t rest = 0;
            auto mux = [&](uint32_t v, uint32_t l, uint32_t h) {
                if (l == h) return l;
                g.node(v, l, h);
                return g.nL + g.V() - 1;
            };
            for (uint32_t i = nbits; i-- > 0;) {
                const uint32_t a0 = mux(2 * i + 1, rest, 1), a1 = mux(2 * i + 1, 0, rest);
                rest = mux(2 * i, a0, a1);
            }
            g.roots = {rest};
            U level, slot;
            uint32_t depth = 0, n_slots = 0;
            expect(g.plan(level, slot, depth, n_slots) == TFHE_OK, T, "refused");
            expect(g.V() == 3 * nbits - 1 && depth == 2 * nbits && n_slots <= 8, T, "nodes, depth or slots");
            expect(replay(g, level, slot, depth, n_slots), T, "replay");
        }
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "plan: refusals";
        U level, slot;
        uint32_t depth = 7, n_slots = 7;
        Graph ok;
        ok.nL = 2, ok.k = 2;
        ok.node(0, 0, 1), ok.node(1, 2, 0, 5, 2 * N);
        ok.roots = {3, 0};
        expect(ok.plan(level, slot, depth, n_slots) == TFHE_OK && depth == 2 && n_slots == 2, T, "the valid graph");
        auto refused = [&](const char *what, auto change) {
            Graph g = ok;
            change(g);
            depth = n_slots = 7;
            expect(g.plan(level, slot, depth, n_slots) == TFHE_ERR_INVALID, T, what);
            expect(depth == 7 && n_slots == 7 && level[0] == 0xABABABABu, T, "something was written on a refusal");
        };
        refused("nL = 0", [](Graph &g) { g.nL = 0; });
        refused("lo = the node itself", [](Graph &g) { g.lo[1] = 3; });
        refused("hi = a later value", [](Graph &g) { g.hi[0] = 3; });
        refused("var >= k", [](Graph &g) { g.var[1] = 2; });
        refused("rlo > 2N", [](Graph &g) { g.rlo[0] = 2 * N + 1; });
        refused("rhi > 2N", [](Graph &g) { g.rhi[1] = 2 * N + 1; });
        refused("root >= nL + V", [](Graph &g) { g.roots[1] = 4; });
        const uint32_t *v = ok.var.data(), *r = ok.roots.data();
        uint32_t *lv = level.data(), *sl = slot.data();
        expect(tfhe_cmux_graph_plan(2, 2, 2, nullptr, v, v, v, v, 2, r, N, lv, sl, nullptr, nullptr) == TFHE_ERR_INVALID, T, "null var");
        expect(tfhe_cmux_graph_plan(2, 2, 2, v, v, v, v, nullptr, 2, r, N, lv, sl, nullptr, nullptr) == TFHE_ERR_INVALID, T, "null rhi");
        expect(tfhe_cmux_graph_plan(2, 2, 2, ok.var.data(), ok.lo.data(), ok.hi.data(), ok.rlo.data(), ok.rhi.data(), 2, nullptr,
                                    N, lv, sl, nullptr, nullptr) == TFHE_ERR_INVALID, T, "null roots");
        expect(tfhe_cmux_graph_plan(2, 2, 2, ok.var.data(), ok.lo.data(), ok.hi.data(), ok.rlo.data(), ok.rhi.data(), 2, r, N,
                                    nullptr, sl, nullptr, nullptr) == TFHE_ERR_INVALID, T, "null level");
        expect(tfhe_cmux_graph_plan(2, 2, 2, ok.var.data(), ok.lo.data(), ok.hi.data(), ok.rlo.data(), ok.rhi.data(), 2, r, N,
                                    lv, sl, nullptr, nullptr) == TFHE_OK, T, "depth and n_slots may be null");
        expect(tfhe_cmux_graph_plan(3, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 1, r + 1, N, nullptr, nullptr, &depth,
                                    &n_slots) == TFHE_OK && depth == 0 && n_slots == 0, T, "V = 0: the roots are leaves");
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
