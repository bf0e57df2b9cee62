// tfhe_cpu.cpp — the GPU-free half of the C ABI (include/tfhe_gpu.h): the tfhe_*
// functions that take no context, and the circuit planner, partitioner and splitter
// whose plans tfhe_gpu.cpp and tfhe_multi.cpp evaluate.
// Plain C++17, no HIP: cpp/test_cpu.cpp runs it stand-alone, under the host sanitizers too.
#include "tfhe_cpu.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <numeric>

#include "host_math.hpp"

namespace tfhe {

bool params_ok(const tfhe_params *p, std::string &why) {
    if (!p) { why = "params is NULL"; return false; }
    if (p->N != 1024 || p->nbit != 10) { why = "only N=1024 (nbit=10) is supported"; return false; }
    if (p->n == 0 || p->n > 1024) { why = "n must be in [1, 1024]"; return false; }
    if (p->L < 1 || p->L > 3) { why = "L must be 1, 2 or 3"; return false; }
    // bgbit = 32 (L = 1) is no gadget this code can hold: Bg = 2^32 does not fit the 32-bit words the
    // offset, the digit mask and the device's bit-field extracts (width 32 reads as 0) work in
    if (p->bgbit < 1 || p->bgbit > 31) { why = "bgbit must be in [1, 31] (Bg = 2^bgbit must fit a 32-bit word)"; return false; }
    if (p->bgbit * p->L > 32) { why = "bgbit*L must be <= 32"; return false; }
    // the select form takes basebit 2 with t in [7, 9] (128/80-bit), the gather form
    // basebit 3..8 with t in [2, 4] (Uint sets); the shapes with faster forms are
    // listed once, in KS_SHAPES (tfhe_kernels.hip)
    const bool ks_sel = p->basebit == 2 && p->iks_t >= 7 && p->iks_t <= 9;
    const bool ks_gather = p->basebit >= 3 && p->basebit <= 8 && p->iks_t >= 2 && p->iks_t <= 4;
    if (!(ks_sel || ks_gather) || p->basebit * p->iks_t >= 31) {
        why = "unsupported key-switch base/levels";
        return false;
    }
    return true;
}

size_t bk_rows(const tfhe_params &p) { return (size_t)p.n * 2 * p.L; }
size_t ksk_rows(const tfhe_params &p) { return (size_t)p.N * p.iks_t * (1u << p.basebit); }
size_t ksk_words(const tfhe_params &p) { return ksk_rows(p) * (p.n + 1); }

// genDecompositionOffset (key.zig:121-131)
uint32_t decomposition_offset(const tfhe_params &p) {
    uint32_t offset = 0;
    for (uint32_t l = 0; l < p.L; l++) offset += ((1u << p.bgbit) / 2) * (1u << (32 - (l + 1) * p.bgbit));
    return offset;
}

// TLWELv0.encryptF64 (tlwe.zig:34-49) with DefaultPrng(seed).
void tlwe_encrypt(uint32_t n, double mu, double alpha, const uint32_t *key, uint64_t seed, uint32_t *out) {
    host::Rng r(seed);
    uint32_t inner = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t x = r.u32();
        inner += key[i] * x;
        out[i] = x;
    }
    host::NormalDist nd(0.0, alpha);
    uint32_t mu_t = host::f64_to_torus(mu);
    out[n] = inner + host::gaussian_torus(mu_t, nd, r);
}

// ---- Circuit evaluation with a level scheduler -------------
// Round packing.  A bootstrapped gate whose consumers all sit at least two
// levels later, and that feeds no NOT, can run one level later without
// changing the depth.  Levels are visited in ascending order; each moves to
// the next level the number of such gates that minimises the modelled
// blind-rotation time of the two levels (blind_rotate_cost: whole rounds of
// 4 x #CUs gates, a ragged tail in the latency form).  Example: a level of
// 10,256 gates hands 16 of them to the next level instead of running a
// 16-gate tail.  Moved gates may move again from their new level.
// TFHE_OPT_CIRCUIT_PACK = 0 turns packing off (A/B runs and tests).
static void pack_levels(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                        const uint32_t *in_b, size_t cus, CostModel model, std::vector<uint32_t> &level,
                        std::vector<std::vector<uint32_t>> &bs) {
    const size_t W = n_inputs + n_gates;
    const uint32_t max_level = (uint32_t)bs.size() - 1;
    // earliest level among each wire's bootstrapped consumers; NOT consumers pin it
    constexpr uint32_t PINNED = 0, FREE = 0xFFFFFFFFu;
    // (kept from the ASAP levels: moving a gate later only raises its inputs'
    // true first use, so the values stay safe)
    std::vector<uint32_t> first_use(W, FREE);
    for (size_t g = 0; g < n_gates; g++) {
        const bool two = ops[g] <= TFHE_GATE_ORYN;
        for (int k = 0; k < (two ? 2 : 1); k++) {
            const uint32_t src = k ? in_b[g] : in_a[g];
            if (ops[g] == TFHE_GATE_NOT) first_use[src] = PINNED;
            else if (first_use[src] != PINNED) first_use[src] = std::min(first_use[src], level[n_inputs + g]);
        }
    }
    const size_t R = 4 * cus;
    const size_t J = (512 + cus - 1) / cus + 1;  // tail breakpoints per round (multiples of #CUs)
    auto cost = [&](size_t b) { return model(b, cus); };
    std::vector<uint32_t> cand;
    for (uint32_t lv = 1; lv < max_level; lv++) {
        cand.clear();
        for (uint32_t g : bs[lv]) {
            const uint32_t u = first_use[n_inputs + g];
            if (u != PINNED && (u == FREE || u >= lv + 2)) cand.push_back(g);
        }
        if (cand.empty()) continue;
        const size_t c0 = bs[lv].size(), c1 = bs[lv + 1].size(), k = cand.size();
        // blind_rotate_cost(c0 - d) only drops where c0 - d reaches a breakpoint
        // m*R + j*#CUs, so those d (and d = 0) are the only candidates
        size_t best_d = 0;
        double best = cost(c0) + cost(c1);
        for (size_t m = (c0 - k) / R; m <= c0 / R; m++)
            for (size_t j = 0; j <= J; j++) {
                const size_t bp = m * R + j * cus;
                if (bp > c0 || bp + k < c0) continue;
                const size_t d = c0 - bp;
                const double cd = cost(bp) + cost(c1 + d);
                if (cd < best - 1e-9 || (cd < best + 1e-9 && d < best_d)) {
                    best = cd;
                    best_d = d;
                }
            }
        if (best_d == 0) continue;
        // move the last best_d candidates (those of the latest gates); their
        // consumers are at lv + 2 or later, their inputs only gain slack
        for (size_t x = k - best_d; x < k; x++) {
            level[n_inputs + cand[x]] = lv + 1;
            bs[lv + 1].push_back(cand[x]);
        }
        std::vector<uint32_t> keep;
        keep.reserve(c0 - best_d);
        for (uint32_t g : bs[lv])
            if (level[n_inputs + g] == lv) keep.push_back(g);
        bs[lv].swap(keep);
    }
}

// Wire w < n_inputs is input w; gate g drives wire n_inputs + g.  A
// bootstrapped gate is ready one level after the later of its inputs; a NOT
// (negation) is ready with its input.  Fills level[] (per wire), the depth and
// the bootstrapped / NOT gates of every level (packed unless `pack` is false);
// returns nullptr, or the reason the graph is invalid.
const char *schedule_levels(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                            const uint32_t *in_b, bool pack, size_t cus, CostModel cost, std::vector<uint32_t> &level,
                            uint32_t &max_level, std::vector<std::vector<uint32_t>> &bs,
                            std::vector<std::vector<uint32_t>> &nots) {
    level.assign(n_inputs + n_gates, 0);
    max_level = 0;
    for (size_t g = 0; g < n_gates; g++) {
        const size_t w = n_inputs + g;
        const int op = ops[g];
        const bool bootstrapped = op <= TFHE_GATE_ORYN || op == TFHE_GATE_COPY;
        if (!bootstrapped && op != TFHE_GATE_NOT) return "unknown gate op";
        if (in_a[g] >= w) return "gate input a is not an earlier wire";
        const bool two = op <= TFHE_GATE_ORYN;
        if (two && in_b[g] >= w) return "gate input b is not an earlier wire";
        uint32_t r = level[in_a[g]];
        if (two) r = std::max(r, level[in_b[g]]);
        level[w] = bootstrapped ? r + 1 : r;
        max_level = std::max(max_level, level[w]);
    }
    // groups in evaluation order: NOT(0), BS(1), NOT(1), ..., BS(max), NOT(max)
    bs.assign(max_level + 1, {});
    nots.assign(max_level + 1, {});
    for (size_t g = 0; g < n_gates; g++) {
        const uint32_t lv = level[n_inputs + g];
        (ops[g] == TFHE_GATE_NOT ? nots[lv] : bs[lv]).push_back((uint32_t)g);
    }
    if (pack && max_level > 1) pack_levels(n_inputs, n_gates, ops, in_a, in_b, cus, cost, level, bs);
    return nullptr;
}

const char *plan_circuit(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                         const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires, bool pack, size_t cus,
                         CostModel cost, CircuitPlan &pl) {
    const size_t W = n_inputs + n_gates;
    if (W > 0xFFFFFFFFull) return "too many wires";
    std::vector<uint32_t> ready;
    if (const char *why = schedule_levels(n_inputs, n_gates, ops, in_a, in_b, pack, cus, cost, ready, pl.max_level,
                                          pl.bs, pl.nots))
        return why;
    for (size_t o = 0; o < n_outputs; o++)
        if (out_wires[o] >= W) return "output wire out of range";
    // A NOT of a NOT is in its input's group, which one gather launch evaluates: it may not read a
    // slot that launch writes.  It equals its input's input, so it shares that wire's slot and
    // leaves the group (pl.nots); every gather index is then below its group's first slot.
    std::vector<uint32_t> same_as(W);
    std::iota(same_as.begin(), same_as.end(), 0u);
    for (size_t g = 0; g < n_gates; g++)
        if (ops[g] == TFHE_GATE_NOT && in_a[g] >= n_inputs && ops[in_a[g] - n_inputs] == TFHE_GATE_NOT)
            same_as[n_inputs + g] = same_as[in_a[in_a[g] - n_inputs]];
    for (std::vector<uint32_t> &group : pl.nots)
        group.erase(std::remove_if(group.begin(), group.end(),
                                   [&](uint32_t g) { return same_as[n_inputs + g] != n_inputs + g; }),
                    group.end());
    std::vector<uint32_t> slot(W);
    for (size_t w = 0; w < n_inputs; w++) slot[w] = (uint32_t)w;
    uint32_t next = (uint32_t)n_inputs;
    for (uint32_t lv = 0; lv <= pl.max_level; lv++) {
        for (uint32_t g : pl.bs[lv]) slot[n_inputs + g] = next++;
        for (uint32_t g : pl.nots[lv]) slot[n_inputs + g] = next++;
    }
    for (size_t w = n_inputs; w < W; w++) slot[w] = slot[same_as[w]];
    pl.idx.clear();
    pl.cops.clear();
    pl.idx.reserve(2 * n_gates + n_outputs);
    for (uint32_t lv = 0; lv <= pl.max_level; lv++) {
        for (uint32_t g : pl.bs[lv]) {
            const bool two = ops[g] <= TFHE_GATE_ORYN;
            pl.idx.push_back(slot[in_a[g]]);
            pl.idx.push_back(two ? slot[in_b[g]] : slot[in_a[g]]);
            pl.cops.push_back(ops[g]);
        }
        for (uint32_t g : pl.nots[lv]) pl.idx.push_back(slot[in_a[g]]);
    }
    for (size_t o = 0; o < n_outputs; o++) pl.idx.push_back(slot[out_wires[o]]);
    return nullptr;
}

// The graph's validation without a plan (before a partition): nullptr, or plan_circuit's
// reason for a graph of at most 2^32 - 1 wires.
const char *check_circuit(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                          const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires) {
    std::vector<uint32_t> level;
    std::vector<std::vector<uint32_t>> bs, nots;
    uint32_t ml = 0;
    if (const char *why = schedule_levels(n_inputs, n_gates, ops, in_a, in_b, false, 256, nullptr, level, ml, bs, nots))
        return why;
    for (size_t o = 0; o < n_outputs; o++)
        if (out_wires[o] >= n_inputs + n_gates) return "output wire out of range";
    return nullptr;
}

namespace {
struct Dsu {
    std::vector<uint32_t> p;
    explicit Dsu(size_t n) : p(n) { std::iota(p.begin(), p.end(), 0u); }
    uint32_t find(uint32_t x) {
        while (p[x] != x) x = p[x] = p[p[x]];
        return x;
    }
    void unite(uint32_t a, uint32_t b) { p[find(a)] = find(b); }
};
}  // namespace

// Device of every gate (dev_of_gate[g] < D) for circuit_eval_multi: the
// connected components of the gate DAG under gate-to-gate wires (primary
// inputs do not join gates: they are replicated), largest first (by
// bootstrapped gates) onto the least-loaded device.
void partition_gates(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a, const uint32_t *in_b,
                     size_t D, std::vector<uint32_t> &dev_of_gate) {
    Dsu dsu(std::max<size_t>(n_gates, 1));
    auto join = [&](size_t g, uint32_t w) {
        if (w >= n_inputs) dsu.unite((uint32_t)g, (uint32_t)(w - n_inputs));
    };
    for (size_t g = 0; g < n_gates; g++) {
        join(g, in_a[g]);
        if (ops[g] <= TFHE_GATE_ORYN) join(g, in_b[g]);
    }
    std::vector<uint64_t> weight(n_gates, 0);
    for (size_t g = 0; g < n_gates; g++)
        if (ops[g] != TFHE_GATE_NOT) weight[dsu.find((uint32_t)g)]++;
    std::vector<uint32_t> roots;
    for (size_t g = 0; g < n_gates; g++)
        if (dsu.find((uint32_t)g) == g) roots.push_back((uint32_t)g);
    std::stable_sort(roots.begin(), roots.end(), [&](uint32_t a, uint32_t b) { return weight[a] > weight[b]; });
    std::vector<uint32_t> dev_of_root(n_gates, 0);
    std::vector<uint64_t> load(D, 0);
    for (uint32_t r : roots) {
        const size_t d = std::min_element(load.begin(), load.end()) - load.begin();
        dev_of_root[r] = (uint32_t)d;
        load[d] += weight[r];
    }
    dev_of_gate.resize(n_gates);
    for (size_t g = 0; g < n_gates; g++) dev_of_gate[g] = dev_of_root[dsu.find((uint32_t)g)];
}

// The D sub-circuits of a placement (dev_of_gate: partition_gates' devices, no
// gate-to-gate wire crossing them; the whole graph passed check_circuit).
// Primary inputs are read-only, so each device gets its own copy of the ones
// it reads.  Wires are renumbered: the device's inputs first (in the order it
// first reads them), then its gates in the whole circuit's order.  An output
// that is a primary input is copied out by device 0.
std::vector<SubCircuit> split_circuit(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                                      const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires,
                                      const std::vector<uint32_t> &dev_of_gate, size_t D) {
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    std::vector<SubCircuit> sub(D);
    std::vector<std::vector<uint32_t>> input_id(D);  // per device: global input -> local id (or none)
    auto wire_dev = [&](uint32_t w) { return w < n_inputs ? 0u : dev_of_gate[w - n_inputs]; };
    auto use_input = [&](uint32_t d, uint32_t w) {
        if (w >= n_inputs) return;
        if (input_id[d].empty()) input_id[d].assign(n_inputs, NONE);
        if (input_id[d][w] == NONE) {
            input_id[d][w] = (uint32_t)sub[d].inputs.size();
            sub[d].inputs.push_back(w);
        }
    };
    for (size_t g = 0; g < n_gates; g++) {
        use_input(dev_of_gate[g], in_a[g]);
        if (ops[g] <= TFHE_GATE_ORYN) use_input(dev_of_gate[g], in_b[g]);
    }
    for (size_t o = 0; o < n_outputs; o++) use_input(wire_dev(out_wires[o]), out_wires[o]);
    std::vector<uint32_t> local_gate(n_gates), gate_count(D, 0);
    for (size_t g = 0; g < n_gates; g++) local_gate[g] = gate_count[dev_of_gate[g]]++;
    auto id = [&](uint32_t d, uint32_t w) {
        return w < n_inputs ? input_id[d][w] : (uint32_t)sub[d].inputs.size() + local_gate[w - n_inputs];
    };
    for (size_t g = 0; g < n_gates; g++) {
        const uint32_t d = dev_of_gate[g];
        sub[d].ops.push_back(ops[g]);
        sub[d].in_a.push_back(id(d, in_a[g]));
        sub[d].in_b.push_back(ops[g] <= TFHE_GATE_ORYN ? id(d, in_b[g]) : 0u);
    }
    for (size_t o = 0; o < n_outputs; o++) {
        const uint32_t d = wire_dev(out_wires[o]);
        sub[d].out_wires.push_back(id(d, out_wires[o]));
        sub[d].out_index.push_back((uint32_t)o);
    }
    return sub;
}

// ---- LUT circuits ---------------------------------------------------------
const char *check_lut_nodes(size_t B, size_t P, size_t T, const uint32_t *term_off, const uint32_t *term_src,
                            const uint32_t *lut) {
    if (B == 0) return nullptr;
    if (term_off[0] != 0) return "term_off[0] is not 0";
    for (size_t i = 0; i < B; i++) {
        if (term_off[i + 1] < term_off[i]) return "term_off is not monotone";
        if (lut && lut[i] >= T) return "table index >= the set's size";
    }
    for (size_t k = 0; k < term_off[B]; k++)
        if (term_src[k] >= P) return "term source is not a ciphertext of the pool";
    return nullptr;
}

// Node g's first output wire, relative to n_inputs (n_nodes + 1 entries: the last is the wire count).
static const char *lut_output_offsets(size_t n_nodes, const uint32_t *theta, std::vector<size_t> &o) {
    o.assign(n_nodes + 1, 0);
    for (size_t g = 0; g < n_nodes; g++) {
        if (theta && theta[g] > TFHE_LUT_MULTI_MAX_LOG) return "theta > TFHE_LUT_MULTI_MAX_LOG";
        o[g + 1] = o[g] + ((size_t)1 << (theta ? theta[g] : 0));
    }
    return nullptr;
}

uint32_t lut_round_shift(const tfhe_params &p, uint32_t theta) { return theta ? 32 - (p.nbit + 1) + theta : 0; }

// nullptr, or what is wrong with the select descriptors themselves (m, the offsets, a theta on a select node)
static const char *check_lut_select(size_t n_nodes, const uint32_t *theta, const LutSelect &sel) {
    if (sel.m < 2 || (sel.m & (sel.m - 1))) return "m must be a power of two >= 2";
    if (!sel.off) return "null select offsets";
    if (sel.off[0] != 0) return "sel_off[0] is not 0";
    for (size_t g = 0; g < n_nodes; g++) {
        if (sel.off[g + 1] < sel.off[g]) return "sel_off is not monotone";
        const uint32_t cnt = sel.off[g + 1] - sel.off[g];
        if (cnt != 0 && cnt != sel.m) return "a node's entry count is neither 0 nor m";
        if (cnt && theta && theta[g] != 0) return "a select node has theta != 0";
    }
    if (sel.off[n_nodes] && !sel.wire) return "null select entries";
    return nullptr;
}

const char *schedule_lut_levels(size_t n_inputs, size_t n_nodes, const uint32_t *term_off, const uint32_t *term_wire,
                                std::vector<uint32_t> &level, uint32_t &depth, const uint32_t *theta,
                                const LutSelect *sel) {
    level.assign(n_nodes, 0);
    depth = 0;
    if (n_nodes == 0) return nullptr;
    std::vector<size_t> o;
    if (const char *why = lut_output_offsets(n_nodes, theta, o)) return why;
    if (n_inputs + o[n_nodes] > 0xFFFFFFFFull) return "too many wires";
    if (term_off[0] != 0) return "term_off[0] is not 0";
    if (sel)
        if (const char *why = check_lut_select(n_nodes, theta, *sel)) return why;
    const bool by_node = theta || sel;  // both entries number the wires through theta (NULL: one wire per node)
    std::vector<uint32_t> node_of;      // multi-output form: the node that drives a wire
    if (by_node) node_of.resize(o[n_nodes]);
    for (size_t g = 0; g < n_nodes; g++) {
        if (term_off[g + 1] < term_off[g]) return "term_off is not monotone";
        uint32_t r = 0;
        for (size_t k = term_off[g]; k < term_off[g + 1]; k++) {
            const size_t w = term_wire[k];
            if (w >= n_inputs + o[g]) return "term wire is not an earlier wire";
            if (w >= n_inputs) r = std::max(r, level[by_node ? node_of[w - n_inputs] : w - n_inputs]);
        }
        for (size_t j = sel ? sel->off[g] : 0; sel && j < sel->off[g + 1]; j++) {
            const size_t w = sel->wire[j];
            if (w == TFHE_LUT_ENTRY_CONST) continue;
            if (w >= n_inputs + o[g]) return "entry wire is not an earlier wire";
            if (w >= n_inputs) r = std::max(r, level[node_of[w - n_inputs]]);
        }
        level[g] = r + 1;
        depth = std::max(depth, level[g]);
        if (by_node) std::fill(node_of.begin() + o[g], node_of.begin() + o[g + 1], (uint32_t)g);
    }
    return nullptr;
}

const char *check_lut_eta(size_t n_nodes, const uint32_t *theta, const uint32_t *eta) {
    for (size_t g = 0; eta && g < n_nodes; g++) {
        if (eta[g] > TFHE_LUT_EXT_MAX_LOG) return "eta > TFHE_LUT_EXT_MAX_LOG";
        if (eta[g] && theta && theta[g]) return "a node has eta > 0 and theta > 0";
    }
    return nullptr;
}

const char *plan_lut_circuit(size_t n_inputs, size_t n_nodes, const uint32_t *term_off, const uint32_t *term_wire,
                             const int32_t *term_coef, const uint32_t *konst, const uint32_t *lut, size_t T,
                             size_t n_outputs, const uint32_t *out_wires, LutCircuitPlan &pl, const uint32_t *theta,
                             const LutSelect *sel, const uint32_t *eta) {
    std::vector<size_t> fo;  // node g's first output wire, relative to n_inputs
    if (const char *why = lut_output_offsets(n_nodes, theta, fo)) return why;
    const size_t W = n_inputs + fo[n_nodes];
    if (W > 0xFFFFFFFFull) return "too many wires";
    if (T >= LUT_TV_EACH) return "the set has 2^31 tables or more";  // the selector's top bit names the other base
    if (const char *why = schedule_lut_levels(n_inputs, n_nodes, term_off, term_wire, pl.level, pl.depth, theta, sel))
        return why;
    if (sel && n_nodes && sel->off[n_nodes] && !sel->konst) return "null select constants";
    if (const char *why = check_lut_eta(n_nodes, theta, eta)) return why;
    auto is_sel = [&](size_t g) { return sel && sel->off[g + 1] != sel->off[g]; };
    auto eta_of = [&](size_t g) { return eta ? eta[g] : 0u; };
    for (size_t g = 0; g < n_nodes; g++) {
        if (is_sel(g) && lut[g] != 0) return "a select node has lut != 0";
        if (lut[g] >= T) return "table index >= the set's size";
        // the extended table t is the entries t E .. t E + E - 1
        if (!is_sel(g) && (((uint64_t)lut[g] + 1) << eta_of(g)) > T) return "extended table index E + E exceeds the set";
    }
    for (size_t o = 0; o < n_outputs; o++)
        if (out_wires[o] >= W) return "output wire out of range";
    // slots in level order (a counting sort of the nodes by level, then eta, a group's ordinary nodes ahead of
    // its select nodes, keeps node order inside each)
    const uint32_t m = sel ? sel->m : 0;
    pl.first.assign((size_t)pl.depth + 1, 0);
    pl.ofirst.assign((size_t)pl.depth + 1, 0);
    pl.sfirst.assign((size_t)pl.depth + 1, 0);
    pl.nsel.assign(pl.depth, 0);
    pl.neta.assign(3 * (size_t)pl.depth, 0);
    pl.nsel_eta.assign(3 * (size_t)pl.depth, 0);
    for (size_t g = 0; g < n_nodes; g++) {
        pl.first[pl.level[g]]++;  // level lv's count at [lv]
        pl.ofirst[pl.level[g]] += (uint32_t)(fo[g + 1] - fo[g]);
        pl.neta[3 * (pl.level[g] - 1) + eta_of(g)]++;
        if (is_sel(g)) pl.sfirst[pl.level[g]]++, pl.nsel[pl.level[g] - 1]++, pl.nsel_eta[3 * (pl.level[g] - 1) + eta_of(g)]++;
    }
    for (uint32_t lv = 1; lv <= pl.depth; lv++) {  // -> its end, its start at [lv - 1]
        pl.first[lv] += pl.first[lv - 1];
        pl.ofirst[lv] += pl.ofirst[lv - 1];
        pl.sfirst[lv] += pl.sfirst[lv - 1];
    }
    pl.order.assign(n_nodes, 0);
    pl.slot.assign(W, 0);
    for (size_t w = 0; w < n_inputs; w++) pl.slot[w] = (uint32_t)w;
    {
        // next[6 (lv-1) + 2 e + s]: where the next node of level lv, group e, kind s (1: select) goes
        std::vector<uint32_t> next(6 * (size_t)pl.depth);
        for (uint32_t lv = 1; lv <= pl.depth; lv++)
            for (uint32_t e = 0, at = pl.first[lv - 1]; e < 3; e++) {
                const uint32_t ne = pl.neta[3 * (lv - 1) + e], ns = pl.nsel_eta[3 * (lv - 1) + e];
                next[6 * (lv - 1) + 2 * e] = at;
                next[6 * (lv - 1) + 2 * e + 1] = at + ne - ns;
                at += ne;
            }
        for (size_t g = 0; g < n_nodes; g++)
            pl.order[next[6 * (pl.level[g] - 1) + 2 * eta_of(g) + (is_sel(g) ? 1 : 0)]++] = (uint32_t)g;
        size_t out_slot = n_inputs;  // the levels are consecutive in `order`, and so are their output slots
        for (size_t at = 0; at < n_nodes; at++)
            for (size_t j = fo[pl.order[at]]; j < fo[pl.order[at] + 1]; j++) pl.slot[n_inputs + j] = (uint32_t)out_slot++;
    }
    // per-level CSR descriptors over slots, concatenated in evaluation order
    const size_t terms = n_nodes ? term_off[n_nodes] : 0;
    pl.off.clear();
    pl.src.clear();
    pl.coef.clear();
    pl.konst.clear();
    pl.lut.clear();
    pl.theta.clear();
    pl.fan.clear();
    pl.tv_sel.clear();
    pl.eta.clear();
    pl.e_off.assign(1, 0);
    pl.e_src.clear();
    pl.e_konst.clear();
    pl.off.reserve(n_nodes + pl.depth);
    pl.src.reserve(terms);
    pl.coef.reserve(terms);
    pl.fan.reserve(2 * fo[n_nodes]);
    for (uint32_t lv = 1; lv <= pl.depth; lv++) {
        pl.off.push_back((uint32_t)pl.src.size());
        uint32_t k_sel = 0;
        for (uint32_t at = pl.first[lv - 1]; at < pl.first[lv]; at++) {
            const uint32_t g = pl.order[at];
            for (size_t k = term_off[g]; k < term_off[g + 1]; k++) {
                pl.src.push_back(pl.slot[term_wire[k]]);
                pl.coef.push_back(term_coef[k]);
            }
            pl.off.push_back((uint32_t)pl.src.size());
            pl.konst.push_back(konst[g]);
            pl.lut.push_back(lut[g]);
            pl.theta.push_back(theta ? theta[g] : 0u);
            pl.eta.push_back(eta_of(g));
            pl.tv_sel.push_back(is_sel(g) ? LUT_TV_EACH | k_sel++ : lut[g]);
            for (uint32_t j = 0; j < fo[g + 1] - fo[g]; j++) {
                pl.fan.push_back(at - pl.first[lv - 1]);
                pl.fan.push_back(j);
            }
            for (uint32_t i = 0; is_sel(g) && i < m; i++) {  // the node's entries, in pack order
                const uint32_t e = sel->wire[sel->off[g] + i];
                if (e != TFHE_LUT_ENTRY_CONST) pl.e_src.push_back(pl.slot[e]);
                pl.e_konst.push_back(e == TFHE_LUT_ENTRY_CONST ? sel->konst[sel->off[g] + i] : 0u);
                pl.e_off.push_back((uint32_t)pl.e_src.size());
            }
        }
    }
    pl.out_slots.resize(n_outputs);
    for (size_t o = 0; o < n_outputs; o++) pl.out_slots[o] = pl.slot[out_wires[o]];
    return nullptr;
}

// ---- Packing key switch: the argument checks shared with the device path ----
bool pack_shape_ok(uint32_t basebit, uint32_t t) {
    return (basebit == 2 && t >= 7 && t <= 9) || (basebit == 5 && t >= 2 && t <= 3);
}
size_t pack_key_words(const tfhe_params &p, uint32_t basebit, uint32_t t) {
    return (size_t)p.n * t * ((size_t)1 << basebit) * 2 * p.N;
}
const char *check_pack_args(const tfhe_params &p, uint32_t basebit, uint32_t t, const uint32_t *coef, size_t C) {
    if (!pack_shape_ok(basebit, t)) return "pack: (basebit, t) has no GEMM form (basebit 2: t 7..9, basebit 5: t 2..3)";
    if (C == 0 || C > p.N) return "pack: C outside 1..N";
    std::vector<bool> seen(p.N, false);
    for (size_t c = 0; c < C; c++) {
        if (coef[c] >= p.N) return "pack: coefficient index >= N";
        if (seen[coef[c]]) return "pack: a coefficient is listed twice";
        seen[coef[c]] = true;
    }
    return nullptr;
}

// ---- CMUX graphs: checks, levels and the per-query scratch slots ------------------------
// level[v] = 1 + the largest level among node v's children (leaves are level 0).  One level is one
// launch, inside which reads and writes are unordered: a node of level l takes the lowest slot whose
// occupant is out of use below l, that is, whose occupant and all of its readers have levels < l;
// a root's slot stays its own to the end.  Nodes are placed in (level, index) order, so the plan is
// a function of the graph alone.
const char *plan_cmux_graph(uint32_t nL, uint32_t V, uint32_t k, const uint32_t *var, const uint32_t *lo,
                            const uint32_t *hi, const uint32_t *rlo, const uint32_t *rhi, uint32_t R,
                            const uint32_t *roots, uint32_t N, CmuxGraphPlan &pl) {
    if (nL == 0) return "CMUX graph: no leaves";
    if (nL >= 0x80000000u || V >= 0x80000000u - nL) return "CMUX graph: more than 2^31 values";
    if (V && (!var || !lo || !hi || !rlo || !rhi)) return "CMUX graph: a null node array";
    if (R && !roots) return "CMUX graph: null roots";
    if (N == 0 || N > 0x40000000u) return "CMUX graph: N outside 1..2^30";
    for (uint32_t v = 0; v < V; v++) {
        if (var[v] >= k) return "CMUX graph: a node's variable >= k";
        if (lo[v] >= nL + v || hi[v] >= nL + v) return "CMUX graph: a node's child is not an earlier value";
        if (rlo[v] > 2 * N || rhi[v] > 2 * N) return "CMUX graph: a rotation > 2N";
    }
    for (uint32_t r = 0; r < R; r++)
        if (roots[r] >= nL + V) return "CMUX graph: a root >= nL + V";
    pl.level.assign(V, 0);
    pl.slot.assign(V, 0);
    pl.depth = pl.n_slots = 0;
    std::vector<uint32_t> last(V, 0);  // the largest level among a node's readers (0: none)
    std::vector<bool> is_root(V, false);
    for (uint32_t v = 0; v < V; v++) {
        uint32_t l = 0;
        for (const uint32_t c : {lo[v], hi[v]})
            if (c >= nL) l = std::max(l, pl.level[c - nL]);
        pl.level[v] = l + 1;
        pl.depth = std::max(pl.depth, l + 1);
        for (const uint32_t c : {lo[v], hi[v]})
            if (c >= nL) last[c - nL] = std::max(last[c - nL], l + 1);
    }
    for (uint32_t r = 0; r < R; r++)
        if (roots[r] >= nL) is_root[roots[r] - nL] = true;
    pl.first.assign(pl.depth + 1, 0);
    for (uint32_t v = 0; v < V; v++) pl.first[pl.level[v]]++;  // first[l]: nodes of level l, then the running sum
    for (uint32_t l = 1, sum = 0; l <= pl.depth; l++) {
        const uint32_t c = pl.first[l];
        pl.first[l - 1] = sum;
        sum += c;
        if (l == pl.depth) pl.first[l] = sum;
    }
    pl.order.assign(V, 0);
    {
        std::vector<uint32_t> at(pl.first.begin(), pl.first.end());
        for (uint32_t v = 0; v < V; v++) pl.order[at[pl.level[v] - 1]++] = v;
    }
    constexpr uint32_t NEVER = 0xFFFFFFFFu;
    std::vector<uint32_t> free_from;  // per slot: the first level whose nodes may take it
    for (const uint32_t v : pl.order) {
        uint32_t s = 0;
        while (s < free_from.size() && free_from[s] > pl.level[v]) s++;
        if (s == free_from.size()) free_from.push_back(0);
        pl.slot[v] = s;
        free_from[s] = is_root[v] ? NEVER : std::max(last[v], pl.level[v]) + 1;
    }
    pl.n_slots = (uint32_t)free_from.size();
    return nullptr;
}

}  // namespace tfhe

using namespace tfhe;

namespace {

uint32_t tlwe_phase(uint32_t n, const uint32_t *ct, const uint32_t *key) {
    uint32_t inner = 0;
    for (uint32_t i = 0; i < n; i++) inner += ct[i] * key[i];
    return ct[n] - inner;
}

// PublicKeyLv0.encryptF64 (proxy_reenc.zig:83-113): plaintext on b, each
// encryption of zero kept with probability 1/2 and added or subtracted with
// probability 1/2 (two booleans, the second only when kept), then fresh noise.
void pk_encrypt(uint32_t n, const uint32_t *pk, size_t pk_size, double plaintext, double alpha, uint64_t seed,
                uint32_t *out) {
    host::Rng r(seed);
    std::fill(out, out + n + 1, 0u);
    out[n] = host::f64_to_torus(plaintext);
    for (size_t e = 0; e < pk_size; e++) {
        if (!r.boolean()) continue;
        const uint32_t *enc = pk + e * (n + 1);
        if (r.boolean())
            for (uint32_t x = 0; x <= n; x++) out[x] += enc[x];
        else
            for (uint32_t x = 0; x <= n; x++) out[x] -= enc[x];
    }
    host::NormalDist nd(0.0, alpha);
    out[n] += host::gaussian_torus(0u, nd, r);
}

// ProxyReencryptionKey.new{Symmetric,Asymmetric}WithParams (proxy_reenc.zig:
// 150-256): entry (i, j, k != 0) encrypts k * key_from[i] / 2^((j+1)*basebit)
// under the target; the c-th encryption in (i, j, k) order uses seed0 + c.
template <class Enc>
void reenc_key_gen(uint32_t n, const uint32_t *key_from, uint32_t basebit, uint32_t t, uint64_t seed0,
                   uint32_t *out, Enc enc) {
    const uint32_t base = 1u << basebit;
    std::fill(out, out + (size_t)n * t * base * (n + 1), 0u);
    uint64_t c = 0;
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t j = 0; j < t; j++)
            for (uint32_t k = 1; k < base; k++) {
                const double p = ((double)k * (double)key_from[i]) / (double)(1u << ((j + 1) * basebit));
                enc(p, seed0 + c++, out + ((size_t)base * t * i + (size_t)base * j + k) * (n + 1));
            }
}

// ---- Cloud-key files (include/tfhe_gpu.h) ---------------
struct KeyFileHeader {
    char magic[8];
    uint32_t version, n, N, L, bgbit, basebit, iks_t, offset;
    uint64_t bsk_len, ksk_len, checksum;
};
static_assert(sizeof(KeyFileHeader) == 64, "key file header is 64 bytes");
constexpr char KEY_MAGIC[8] = {'Z', 'T', 'F', 'H', 'E', 'C', 'K', '1'};

// FNV-1a-64 over 8-byte little-endian words; a section's last < 8 bytes one by one
struct Fnv64 {
    uint64_t h = 0xcbf29ce484222325ull;
    void add(const void *p, size_t bytes) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        size_t k = 0;
        for (; k + 8 <= bytes; k += 8) {
            uint64_t w;
            std::memcpy(&w, b + k, 8);
            h = (h ^ w) * 0x100000001b3ull;
        }
        for (; k < bytes; k++) h = (h ^ b[k]) * 0x100000001b3ull;
    }
};

uint64_t key_checksum(const tfhe_params *p, const uint32_t *tv_a, const uint32_t *tv_b, const double *bsk,
                      size_t bsk_len, const uint32_t *ksk, size_t ksk_len) {
    Fnv64 f;
    f.add(tv_a, p->N * sizeof(uint32_t));
    f.add(tv_b, p->N * sizeof(uint32_t));
    f.add(bsk, bsk_len * sizeof(double));
    f.add(ksk, ksk_len * sizeof(uint32_t));
    return f.h;
}

bool key_shape_ok(const tfhe_params *p, size_t bsk_len, size_t ksk_len) {
    std::string why;
    return params_ok(p, why) && bsk_len == bk_rows(*p) * 2 * p->N && ksk_len == ksk_words(*p);
}

// generateLookupTableFullAssign (lut/generator.zig:155-191): message x's range
// [divRound(xN, m), divRound((x+1)N, m)) of the raw table holds values[x]; the
// table is rotated by divRound(N, 2m), its last divRound(N, 2m) entries negated,
// and stored as the b polynomial (a = 0).  divRound(a, b) = (a + b/2) / b
// (generator.zig:253-255).  Any m >= 1, as the reference (m > N leaves ranges empty).
void lut_from_values(size_t N, size_t m, const uint32_t *values, uint32_t *tv) {
    std::vector<uint32_t> raw(N, 0u);
    auto div_round = [](size_t a, size_t b) { return (a + b / 2) / b; };
    for (size_t x = 0; x < m; x++) {
        const size_t s = div_round(x * N, m), e = div_round((x + 1) * N, m);
        for (size_t i = s; i < e; i++) raw[i] = values[x];
    }
    const size_t off = div_round(N, 2 * m);
    for (size_t i = 0; i < N; i++) tv[N + i] = raw[(i + off) % N];
    for (size_t i = N - off; i < N; i++) tv[N + i] = ~tv[N + i] + 1u;
    for (size_t i = 0; i < N; i++) tv[i] = 0;
}

}  // namespace

extern "C" {

int tfhe_cloud_key_write(const char *path, const tfhe_params *p, uint32_t offset, const uint32_t *tv_a,
                         const uint32_t *tv_b, const double *bsk, size_t bsk_len, const uint32_t *ksk,
                         size_t ksk_len) {
    if (!path || !tv_a || !tv_b || !bsk || !ksk || !key_shape_ok(p, bsk_len, ksk_len)) return TFHE_ERR_INVALID;
    KeyFileHeader h{};
    std::memcpy(h.magic, KEY_MAGIC, 8);
    h.version = 1;
    h.n = p->n, h.N = p->N, h.L = p->L, h.bgbit = p->bgbit, h.basebit = p->basebit, h.iks_t = p->iks_t;
    h.offset = offset;
    h.bsk_len = bsk_len;
    h.ksk_len = ksk_len;
    h.checksum = key_checksum(p, tv_a, tv_b, bsk, bsk_len, ksk, ksk_len);
    FILE *fp = std::fopen(path, "wb");
    if (!fp) return TFHE_ERR_IO;
    bool ok = std::fwrite(&h, sizeof h, 1, fp) == 1 && std::fwrite(tv_a, 4, p->N, fp) == p->N &&
              std::fwrite(tv_b, 4, p->N, fp) == p->N && std::fwrite(bsk, 8, bsk_len, fp) == bsk_len &&
              std::fwrite(ksk, 4, ksk_len, fp) == ksk_len;
    ok = std::fclose(fp) == 0 && ok;
    return ok ? TFHE_OK : TFHE_ERR_IO;
}

int tfhe_cloud_key_read(const char *path, const tfhe_params *p, uint32_t *offset, uint32_t *tv_a, uint32_t *tv_b,
                        double *bsk, size_t bsk_len, uint32_t *ksk, size_t ksk_len) {
    if (!path || !offset || !tv_a || !tv_b || !bsk || !ksk || !key_shape_ok(p, bsk_len, ksk_len))
        return TFHE_ERR_INVALID;
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return TFHE_ERR_IO;
    KeyFileHeader h{};
    int rc = TFHE_OK;
    if (std::fread(&h, sizeof h, 1, fp) != 1)
        rc = TFHE_ERR_IO;
    else if (std::memcmp(h.magic, KEY_MAGIC, 8) != 0 || h.version != 1)
        rc = TFHE_ERR_INVALID;  // not a key file of this format
    else if (h.n != p->n || h.N != p->N || h.L != p->L || h.bgbit != p->bgbit || h.basebit != p->basebit ||
             h.iks_t != p->iks_t || h.bsk_len != bsk_len || h.ksk_len != ksk_len)
        rc = TFHE_ERR_INVALID;  // another parameter set
    else if (std::fread(tv_a, 4, p->N, fp) != p->N || std::fread(tv_b, 4, p->N, fp) != p->N ||
             std::fread(bsk, 8, bsk_len, fp) != bsk_len || std::fread(ksk, 4, ksk_len, fp) != ksk_len)
        rc = TFHE_ERR_IO;  // truncated
    std::fclose(fp);
    if (rc) return rc;
    if (key_checksum(p, tv_a, tv_b, bsk, bsk_len, ksk, ksk_len) != h.checksum) return TFHE_ERR_INVALID;
    *offset = h.offset;
    return TFHE_OK;
}

int tfhe_decomposition_offset(const tfhe_params *p, uint32_t *offset) {
    std::string why;
    if (!params_ok(p, why) || !offset) return TFHE_ERR_INVALID;
    *offset = decomposition_offset(*p);
    return TFHE_OK;
}

int tfhe_secret_key_new(const tfhe_params *p, uint64_t seed, uint32_t *key_lv0, uint32_t *key_lv1) {
    if (!p || !key_lv0 || !key_lv1) return TFHE_ERR_INVALID;
    host::Rng r(seed);  // SecretKey.new (key.zig:41-57)
    for (uint32_t i = 0; i < p->n; i++) key_lv0[i] = r.boolean() ? 1u : 0u;
    for (uint32_t i = 0; i < p->N; i++) key_lv1[i] = r.boolean() ? 1u : 0u;
    return TFHE_OK;
}

int tfhe_public_key_gen(const tfhe_params *p, const uint32_t *key, size_t size, double alpha, uint64_t seed0,
                        uint32_t *pk) {
    if (!p || !key || (size && !pk)) return TFHE_ERR_INVALID;
    for (size_t e = 0; e < size; e++) tlwe_encrypt(p->n, 0.0, alpha, key, seed0 + e, pk + e * (p->n + 1));
    return TFHE_OK;
}

int tfhe_public_key_encrypt_bool_batch(const tfhe_params *p, const uint32_t *pk, size_t pk_size, const uint8_t *bits,
                                       double alpha, uint64_t seed0, uint32_t *out, size_t B) {
    if (!p || (pk_size && !pk) || (B && (!bits || !out))) return TFHE_ERR_INVALID;
    for (size_t i = 0; i < B; i++)
        pk_encrypt(p->n, pk, pk_size, bits[i] ? 0.125 : -0.125, alpha, seed0 + i, out + i * (p->n + 1));
    return TFHE_OK;
}

int tfhe_reenc_key_gen_symmetric(const tfhe_params *p, const uint32_t *key_from, const uint32_t *key_to, double alpha,
                                 uint32_t basebit, uint32_t t, uint64_t seed0, uint32_t *out) {
    if (!p || !key_from || !key_to || !out || basebit < 1 || basebit > 8 || t < 1) return TFHE_ERR_INVALID;
    reenc_key_gen(p->n, key_from, basebit, t, seed0, out, [&](double v, uint64_t seed, uint32_t *o) {
        tlwe_encrypt(p->n, v, alpha, key_to, seed, o);
    });
    return TFHE_OK;
}

int tfhe_reenc_key_gen_asymmetric(const tfhe_params *p, const uint32_t *key_from, const uint32_t *pk, size_t pk_size,
                                  double alpha, uint32_t basebit, uint32_t t, uint64_t seed0, uint32_t *out) {
    if (!p || !key_from || !out || (pk_size && !pk) || basebit < 1 || basebit > 8 || t < 1) return TFHE_ERR_INVALID;
    reenc_key_gen(p->n, key_from, basebit, t, seed0, out, [&](double v, uint64_t seed, uint32_t *o) {
        pk_encrypt(p->n, pk, pk_size, v, alpha, seed, o);
    });
    return TFHE_OK;
}

int tfhe_circuit_partition(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                           const uint32_t *in_b, int num_devices, uint32_t *device_of_gate) {
    if ((n_gates && (!ops || !in_a || !in_b || !device_of_gate)) || num_devices < 1) return TFHE_ERR_INVALID;
    if (n_inputs + n_gates > 0xFFFFFFFFull) return TFHE_ERR_INVALID;
    if (check_circuit(n_inputs, n_gates, ops, in_a, in_b, 0, nullptr)) return TFHE_ERR_INVALID;
    std::vector<uint32_t> dev;
    partition_gates(n_inputs, n_gates, ops, in_a, in_b, (size_t)num_devices, dev);
    std::copy(dev.begin(), dev.end(), device_of_gate);
    return TFHE_OK;
}

int tfhe_lut_circuit_schedule(size_t n_inputs, size_t n_nodes, const uint32_t *term_off, const uint32_t *term_wire,
                              uint32_t *levels, uint32_t *depth) {
    if (n_nodes && (!term_off || !levels || (term_off[n_nodes] && !term_wire))) return TFHE_ERR_INVALID;
    std::vector<uint32_t> level;
    uint32_t d = 0;
    if (schedule_lut_levels(n_inputs, n_nodes, term_off, term_wire, level, d)) return TFHE_ERR_INVALID;
    std::copy(level.begin(), level.end(), levels);
    if (depth) *depth = d;
    return TFHE_OK;
}

int tfhe_lut_circuit_schedule_multi(size_t n_inputs, size_t n_nodes, const uint32_t *term_off, const uint32_t *term_wire,
                                    const uint32_t *theta, uint32_t *levels, uint32_t *depth) {
    if (n_nodes && (!term_off || !levels || (term_off[n_nodes] && !term_wire))) return TFHE_ERR_INVALID;
    std::vector<uint32_t> level;
    uint32_t d = 0;
    if (schedule_lut_levels(n_inputs, n_nodes, term_off, term_wire, level, d, theta)) return TFHE_ERR_INVALID;
    std::copy(level.begin(), level.end(), levels);
    if (depth) *depth = d;
    return TFHE_OK;
}

int tfhe_lut_circuit_schedule_select(size_t n_inputs, size_t n_nodes, const uint32_t *term_off,
                                     const uint32_t *term_wire, const uint32_t *theta, uint32_t m,
                                     const uint32_t *sel_off, const uint32_t *sel_wire, uint32_t *levels,
                                     uint32_t *depth) {
    if (!sel_off) return tfhe_lut_circuit_schedule_multi(n_inputs, n_nodes, term_off, term_wire, theta, levels, depth);
    if (n_nodes && (!term_off || !levels || (term_off[n_nodes] && !term_wire))) return TFHE_ERR_INVALID;
    const LutSelect sel{m, sel_off, sel_wire, nullptr};
    std::vector<uint32_t> level;
    uint32_t d = 0;
    if (schedule_lut_levels(n_inputs, n_nodes, term_off, term_wire, level, d, theta, &sel)) return TFHE_ERR_INVALID;
    std::copy(level.begin(), level.end(), levels);
    if (depth) *depth = d;
    return TFHE_OK;
}

int tfhe_lut_circuit_schedule_ext(size_t n_inputs, size_t n_nodes, const uint32_t *term_off, const uint32_t *term_wire,
                                  const uint32_t *theta, uint32_t m, const uint32_t *sel_off, const uint32_t *sel_wire,
                                  const uint32_t *eta, uint32_t *levels, uint32_t *depth, uint32_t *group_nodes) {
    if (n_nodes && !levels) return TFHE_ERR_INVALID;
    if (check_lut_eta(n_nodes, theta, eta)) return TFHE_ERR_INVALID;
    uint32_t d = 0;
    if (const int rc = tfhe_lut_circuit_schedule_select(n_inputs, n_nodes, term_off, term_wire, theta, m, sel_off,
                                                        sel_wire, levels, &d))
        return rc;
    if (depth) *depth = d;
    if (group_nodes) {
        std::fill(group_nodes, group_nodes + 3 * (size_t)d, 0u);
        for (size_t g = 0; g < n_nodes; g++) group_nodes[3 * (levels[g] - 1) + (eta ? eta[g] : 0u)]++;
    }
    return TFHE_OK;
}

// round_theta of the multi-output LUT bootstrap (include/tfhe_gpu.h): every word to the nearest
// multiple of 2^s, s = 32 - (log2 N + 1) + theta, in wrapping u32; theta = 0 is the identity.
int tfhe_lut_round_tlwe(const tfhe_params *p, uint32_t theta, const uint32_t *in, uint32_t *out, size_t B) {
    std::string why;
    if (!p || !params_ok(p, why) || theta > TFHE_LUT_MULTI_MAX_LOG || (B && (!in || !out))) return TFHE_ERR_INVALID;
    const uint32_t s = lut_round_shift(*p, theta);
    const size_t words = B * ((size_t)p->n + 1);
    for (size_t i = 0; i < words; i++) out[i] = s ? (in[i] + (1u << (s - 1))) & ~((1u << s) - 1) : in[i];
    return TFHE_OK;
}

// TV[h][q] = tv_{q mod nu}[h][q - (q mod nu)], nu = 2^theta, on both halves.
int tfhe_lut_interleave(const tfhe_params *p, const uint32_t *testvecs, uint32_t theta, uint32_t *out) {
    std::string why;
    if (!p || !params_ok(p, why) || theta > TFHE_LUT_MULTI_MAX_LOG || !testvecs || !out) return TFHE_ERR_INVALID;
    const size_t N = p->N, nu = (size_t)1 << theta;
    for (size_t h = 0; h < 2; h++)
        for (size_t q = 0; q < N; q++) out[h * N + q] = testvecs[(q % nu) * 2 * N + h * N + (q - q % nu)];
    return TFHE_OK;
}

// spread of the bivariate LUT bootstrap (include/tfhe_gpu.h), term by term as it is defined: on each
// half, S = sum_{j<w} polyMulWithXK(in, j) (trgsw.zig:442-466), then out = polyMulWithXK(S, rot).
int tfhe_lut_spread(const tfhe_params *p, const uint32_t *in, uint32_t w, uint32_t rot, uint32_t *out, size_t B) {
    std::string why;
    if (!p || !params_ok(p, why) || w == 0 || w > p->N || rot > 2 * p->N || (B && (!in || !out))) return TFHE_ERR_INVALID;
    const size_t N = p->N;
    std::vector<uint32_t> S(N);
    for (size_t h = 0; h < 2 * B; h++) {
        const uint32_t *x = in + h * N;
        uint32_t *y = out + h * N;
        for (size_t i = 0; i < N; i++) {
            uint32_t acc = 0;
            for (size_t j = 0; j < w; j++) acc += j <= i ? x[i - j] : 0u - x[N + i - j];
            S[i] = acc;
        }
        if (rot < N) {
            for (size_t i = 0; i < N - rot; i++) y[i + rot] = S[i];
            for (size_t i = N - rot; i < N; i++) y[i + rot - N] = 0u - S[i];
        } else {
            for (size_t i = 0; i < 2 * N - rot; i++) y[i + rot - N] = 0u - S[i];
            for (size_t i = 2 * N - rot; i < N; i++) y[i - (2 * N - rot)] = S[i];
        }
    }
    return TFHE_OK;
}

// ---- host-side TLWELv0 helpers ------------------------------------------
int tfhe_encrypt_bool_batch(const tfhe_params *p, const uint32_t *key, const uint8_t *bits, uint64_t seed0,
                            uint32_t *out, size_t B) {
    if (!p || !key || (B && (!bits || !out))) return TFHE_ERR_INVALID;
    for (size_t i = 0; i < B; i++)
        tlwe_encrypt(p->n, bits[i] ? 0.125 : -0.125, p->alpha_lv0, key, seed0 + i, out + i * (p->n + 1));
    return TFHE_OK;
}

int tfhe_decrypt_bool_batch(const tfhe_params *p, const uint32_t *key, const uint32_t *ct, uint8_t *bits, size_t B) {
    if (!p || !key || (B && (!bits || !ct))) return TFHE_ERR_INVALID;
    for (size_t i = 0; i < B; i++) bits[i] = (int32_t)tlwe_phase(p->n, ct + i * (p->n + 1), key) >= 0;
    return TFHE_OK;
}

int tfhe_encrypt_lwe_message_batch(const tfhe_params *p, const uint32_t *key, const uint32_t *msgs, uint32_t m,
                                   uint64_t seed0, uint32_t *out, size_t B) {
    if (!p || !key || m == 0 || (B && (!msgs || !out))) return TFHE_ERR_INVALID;
    const double scale = 1.0 / (2.0 * (double)m);
    for (size_t i = 0; i < B; i++)
        tlwe_encrypt(p->n, (double)(msgs[i] % m) * scale, p->alpha_lv0, key, seed0 + i, out + i * (p->n + 1));
    return TFHE_OK;
}

int tfhe_decrypt_lwe_message_batch(const tfhe_params *p, const uint32_t *key, const uint32_t *ct, uint32_t m,
                                   uint32_t *msgs, size_t B) {
    if (!p || !key || m == 0 || (B && (!msgs || !ct))) return TFHE_ERR_INVALID;
    const double scale = 1.0 / (2.0 * (double)m);
    for (size_t i = 0; i < B; i++) {
        double f = (double)tlwe_phase(p->n, ct + i * (p->n + 1), key) / 4294967296.0;
        msgs[i] = (uint32_t)((uint64_t)(f / scale + 0.5) % m);
    }
    return TFHE_OK;
}

int tfhe_lut_generate_scaled(const tfhe_params *p, uint32_t m, double scale, const uint32_t *f_table, uint32_t *tv) {
    if (!p || !f_table || !tv || m == 0 || m > TFHE_LUT_MAX_M) return TFHE_ERR_INVALID;
    try {
        std::vector<uint32_t> enc(m);
        for (uint32_t x = 0; x < m; x++)  // Encoder.encode (encoder.zig:66-74): (f(x) mod m) * scale -> torus
            enc[x] = host::f64_to_torus((double)(f_table[x] % m) * scale);
        lut_from_values(p->N, m, enc.data(), tv);
    } catch (const std::bad_alloc &) {  // never through the C ABI (std::terminate)
        return TFHE_ERR_OOM;
    }
    return TFHE_OK;
}

int tfhe_lut_generate(const tfhe_params *p, uint32_t m, const uint32_t *f_table, uint32_t *tv) {
    if (!p || m == 0 || m > TFHE_LUT_MAX_M) return TFHE_ERR_INVALID;
    return tfhe_lut_generate_scaled(p, m, 1.0 / (2.0 * (double)m), f_table, tv);  // Encoder.new (encoder.zig:29-42)
}

int tfhe_lut_generate_full(const tfhe_params *p, uint32_t m, const uint32_t *values, uint32_t *tv) {
    if (!p || !values || !tv || m == 0 || m > TFHE_LUT_MAX_M) return TFHE_ERR_INVALID;
    try {
        lut_from_values(p->N, m, values, tv);
    } catch (const std::bad_alloc &) {
        return TFHE_ERR_OOM;
    }
    return TFHE_OK;
}

// ---- Extended LUT bootstrap (include/tfhe_gpu.h): the host half ----
// The test vector of degree N * E, split into its E components over Z[Y]/(Y^N + 1), Y = X^E.
int tfhe_lut_generate_ext(const tfhe_params *p, uint32_t eta, uint32_t m, const uint32_t *f_table, uint32_t *out) {
    std::string why;
    if (!params_ok(p, why) || eta > TFHE_LUT_EXT_MAX_LOG || !f_table || !out || m == 0 || m > TFHE_LUT_MAX_M)
        return TFHE_ERR_INVALID;
    if (eta == 0) return tfhe_lut_generate(p, m, f_table, out);
    const size_t N = p->N, E = (size_t)1 << eta;
    const double scale = 1.0 / (2.0 * (double)m);  // Encoder.new (encoder.zig:29-42)
    try {
        std::vector<uint32_t> enc(m), tv(2 * N * E);
        for (uint32_t x = 0; x < m; x++) enc[x] = host::f64_to_torus((double)(f_table[x] % m) * scale);
        lut_from_values(N * E, m, enc.data(), tv.data());
        const uint32_t *b = tv.data() + N * E;
        for (size_t j = 0; j < E; j++) {
            uint32_t *c = out + j * 2 * N;
            for (size_t k = 0; k < N; k++) c[k] = 0, c[N + k] = b[k * E + j];
        }
    } catch (const std::bad_alloc &) {
        return TFHE_ERR_OOM;
    }
    return TFHE_OK;
}

// polyMulWithXK (trgsw.zig:442-466) on one half of N words, the exponent taken mod 2N
static void mul_xk_half(const uint32_t *x, size_t N, size_t k, uint32_t *y) {
    k %= 2 * N;
    for (size_t i = 0; i < N; i++) {
        const size_t at = (i + k) % (2 * N);
        y[at % N] = at < N ? x[i] : 0u - x[i];
    }
}

// X^a on E components: a = q E + r sends component c to component (c + r) mod E, times Y^q, and once
// more times Y where c + r wraps (X^E = Y).  Output k reads component (k - r) mod E with q + [k < r].
int tfhe_lut_ext_rotate(const tfhe_params *p, uint32_t eta, const uint32_t *in, uint32_t a, uint32_t *out) {
    std::string why;
    if (!params_ok(p, why) || eta > TFHE_LUT_EXT_MAX_LOG || !in || !out || in == out) return TFHE_ERR_INVALID;
    const size_t N = p->N, E = (size_t)1 << eta;
    if (a > 2 * N * E) return TFHE_ERR_INVALID;
    const size_t q = a >> eta, r = a & (E - 1);
    for (size_t k = 0; k < E; k++) {
        const uint32_t *c = in + ((k + E - r) & (E - 1)) * 2 * N;
        const size_t ex = q + (k < r ? 1 : 0);
        mul_xk_half(c, N, ex, out + k * 2 * N);
        mul_xk_half(c + N, N, ex, out + k * 2 * N + N);
    }
    return TFHE_OK;
}

// (word + 2^(sh-1)) >> sh with sh = 32 - (nbit + 1) - eta, the add in 64 bits (trgsw.zig:297, :312):
// a position in [0, 2N E]
int tfhe_lut_ext_mod_switch(const tfhe_params *p, uint32_t eta, uint32_t word) {
    std::string why;
    if (!params_ok(p, why) || eta > TFHE_LUT_EXT_MAX_LOG) return TFHE_ERR_INVALID;
    const uint32_t sh = 32 - (p->nbit + 1) - eta;
    return (int)(((uint64_t)word + ((uint64_t)1 << (sh - 1))) >> sh);
}

// Table entries for tfhe_gpu_table_lookup_*: entry e as a trivial TRLWELv1 (a = 0) whose
// coefficient c < width carries bit c of values[e] as +-1/8 (f64ToTorus(+-0.125), the gates'
// plaintexts, gates.zig:48-121); bits past 63 read as clear.
int tfhe_lookup_table_pack_bits(const tfhe_params *p, const uint64_t *values, size_t entries, uint32_t width,
                                uint32_t *table) {
    std::string why;
    if (!params_ok(p, why) || (entries && (!values || !table)) || width > p->N) return TFHE_ERR_INVALID;
    const size_t N = p->N;
    const uint32_t plus = host::f64_to_torus(0.125), minus = host::f64_to_torus(-0.125);
    for (size_t e = 0; e < entries; e++) {
        uint32_t *t = table + e * 2 * N;
        std::memset(t, 0, 2 * N * sizeof(uint32_t));
        for (uint32_t c = 0; c < width; c++) t[N + c] = c < 64 && ((values[e] >> c) & 1u) ? plus : minus;
    }
    return TFHE_OK;
}

// The packed lookup's shape (tfhe_gpu_packed_lookup_*): entries of `width` bits sit `stride` (the
// next power of two) coefficients apart, N / stride to a TRLWE; the low h address bits choose
// the slot (one rotate-CMUX each, by X^-(stride 2^j) = X^(2N - stride 2^j)), the other v the TRLWE.
int tfhe_packed_lookup_plan(const tfhe_params *p, uint32_t k, uint32_t width, tfhe_packed_plan *out) {
    std::string why;
    if (!params_ok(p, why) || !out || k == 0 || width == 0 || width > p->N) return TFHE_ERR_INVALID;
    uint32_t stride = 1, slot_bits = 0;
    while (stride < width) stride *= 2;
    while ((stride << slot_bits) < p->N) slot_bits++;
    const uint32_t h = std::min(k, slot_bits);
    if (k - h > 12) return TFHE_ERR_INVALID;  // the tree's limit (tfhe_gpu_table_lookup_*)
    tfhe_packed_plan pl{};
    pl.stride = stride;
    pl.slots = p->N / stride;
    pl.h = h;
    pl.v = k - h;
    pl.trlwes = 1u << pl.v;
    pl.cmuxes = pl.trlwes - 1 + h;
    for (uint32_t j = 0; j < h; j++) pl.rot[j] = 2 * p->N - (stride << j);
    *out = pl;
    return TFHE_OK;
}

// A CMUX graph's levels and scratch slots (plan_cmux_graph above); nothing is written on a refusal.
int tfhe_cmux_graph_plan(uint32_t nL, uint32_t V, uint32_t k, const uint32_t *var, const uint32_t *lo, const uint32_t *hi,
                         const uint32_t *rlo, const uint32_t *rhi, uint32_t R, const uint32_t *roots, uint32_t N,
                         uint32_t *level, uint32_t *slot, uint32_t *depth, uint32_t *n_slots) {
    CmuxGraphPlan pl;
    if (V && (!level || !slot)) return TFHE_ERR_INVALID;
    if (plan_cmux_graph(nL, V, k, var, lo, hi, rlo, rhi, R, roots, N, pl)) return TFHE_ERR_INVALID;
    if (V) {
        std::memcpy(level, pl.level.data(), V * sizeof(uint32_t));
        std::memcpy(slot, pl.slot.data(), V * sizeof(uint32_t));
    }
    if (depth) *depth = pl.depth;
    if (n_slots) *n_slots = pl.n_slots;
    return TFHE_OK;
}

// The packed table of 2^k values: entry e in TRLWE e >> h, bit c of it at coefficient
// (e & (2^h - 1)) * stride + c as +-1/8 (tfhe_lookup_table_pack_bits' plaintexts); trivial (a = 0).
int tfhe_lookup_table_pack_slots(const tfhe_params *p, const uint64_t *values, uint32_t k, uint32_t width, uint32_t *table) {
    tfhe_packed_plan pl;
    if (!values || !table || width > 64 || tfhe_packed_lookup_plan(p, k, width, &pl) != TFHE_OK) return TFHE_ERR_INVALID;
    const size_t N = p->N, entries = (size_t)1 << k;
    const uint32_t plus = host::f64_to_torus(0.125), minus = host::f64_to_torus(-0.125);
    std::memset(table, 0, (size_t)pl.trlwes * 2 * N * sizeof(uint32_t));
    for (size_t e = 0; e < entries; e++) {
        uint32_t *b = table + (e >> pl.h) * 2 * N + N + (e & (((size_t)1 << pl.h) - 1)) * pl.stride;
        for (uint32_t c = 0; c < width; c++) b[c] = ((values[e] >> c) & 1u) ? plus : minus;
    }
    return TFHE_OK;
}

// The packing key switch on the host (include/tfhe_gpu.h): per item R = (0, (b, 0, ..)) - sum_{i,j}
// row[base t i + base j + digit j of a_i + PREC], then out[b] += X^coef[c] R on each half.
int tfhe_pack_tlwe(const tfhe_params *p, const uint32_t *rows, uint32_t basebit, uint32_t t, const uint32_t *in,
                   const uint32_t *coef, size_t C, uint32_t *out_trlwe, size_t B) {
    std::string why;
    if (!params_ok(p, why) || !rows || !coef || (B && (!in || !out_trlwe))) return TFHE_ERR_INVALID;
    if (check_pack_args(*p, basebit, t, coef, C)) return TFHE_ERR_INVALID;
    const size_t N = p->N, n = p->n, base = (size_t)1 << basebit;
    const uint32_t prec = 1u << (32 - (1 + basebit * t));
    std::vector<uint32_t> R(2 * N);
    for (size_t b = 0; b < B; b++) {
        uint32_t *o = out_trlwe + b * 2 * N;
        std::memset(o, 0, 2 * N * sizeof(uint32_t));
        for (size_t c = 0; c < C; c++) {
            const uint32_t *x = in + (b * C + c) * (n + 1);
            std::fill(R.begin(), R.end(), 0u);
            R[N] = x[n];
            for (size_t i = 0; i < n; i++) {
                const uint32_t abar = x[i] + prec;
                for (uint32_t j = 0; j < t; j++) {
                    const uint32_t d = (abar >> (32 - (j + 1) * basebit)) & (uint32_t)(base - 1);
                    const uint32_t *row = rows + (base * t * i + base * j + d) * 2 * N;
                    for (size_t w = 0; w < 2 * N; w++) R[w] -= row[w];
                }
            }
            const size_t k = coef[c];
            for (size_t half = 0; half < 2; half++) {
                const uint32_t *r = R.data() + half * N;
                uint32_t *oh = o + half * N;
                for (size_t q = 0; q < N - k; q++) oh[q + k] += r[q];
                for (size_t q = N - k; q < N; q++) oh[q + k - N] -= r[q];
            }
        }
    }
    return TFHE_OK;
}

int tfhe_fft_tables(uint32_t N, int source, double *twist_re, double *twist_im, double *stage_re, double *stage_im) {
    if (N < 4 || (N & (N - 1)) || (source != TFHE_TWIDDLES_GLIBC && source != TFHE_TWIDDLES_FDLIBM))
        return TFHE_ERR_INVALID;
    std::vector<double> a, b;
    host::twist_table(N, a, b, source);
    if (twist_re) std::memcpy(twist_re, a.data(), a.size() * 8);
    if (twist_im) std::memcpy(twist_im, b.data(), b.size() * 8);
    host::stage_twiddles(N, false, a, b, source);
    if (stage_re) std::memcpy(stage_re, a.data(), a.size() * 8);
    if (stage_im) std::memcpy(stage_im, b.data(), b.size() * 8);
    return TFHE_OK;
}

}  // extern "C"
