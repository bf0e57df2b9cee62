// tfhe_cpu.hpp — what the GPU half of the C ABI (tfhe_gpu.cpp, tfhe_multi.cpp)
// calls in the GPU-free half (tfhe_cpu.cpp: plain C++17, no HIP).  Not installed.
#pragma once

#include "tfhe_gpu.h"

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace tfhe {

bool params_ok(const tfhe_params *p, std::string &why);
size_t bk_rows(const tfhe_params &p);
size_t ksk_rows(const tfhe_params &p);
size_t ksk_words(const tfhe_params &p);
uint32_t decomposition_offset(const tfhe_params &p);
void tlwe_encrypt(uint32_t n, double mu, double alpha, const uint32_t *key, uint64_t seed, uint32_t *out);

// The level packing's model of a blind-rotation launch's time (tfhe_gpu.cpp
// passes blind_rotate_cost, tfhe_kernels.hip); unused when `pack` is false.
using CostModel = double (*)(size_t items, size_t cus);

const char *schedule_levels(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                            const uint32_t *in_b, bool pack, size_t cus, CostModel cost, std::vector<uint32_t> &level,
                            uint32_t &max_level, std::vector<std::vector<uint32_t>> &bs,
                            std::vector<std::vector<uint32_t>> &nots);

// A circuit's evaluation plan: the level schedule and the device wire table
// laid out in evaluation order — inputs | NOTs of level 0 | gates of level 1 |
// NOTs of level 1 | ... — so each level's batch writes one contiguous run of
// slots; its inputs are gathered by index inside the blind-rotation prologue.
// idx / cops: per-group gather indices and op codes, concatenated in
// evaluation order, then the output wires' slots.
struct CircuitPlan {
    std::vector<std::vector<uint32_t>> bs, nots;
    uint32_t max_level = 0;
    std::vector<uint32_t> idx;
    std::vector<uint8_t> cops;
};

const char *plan_circuit(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                         const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires, bool pack, size_t cus,
                         CostModel cost, CircuitPlan &pl);
const char *check_circuit(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                          const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires);
void partition_gates(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a, const uint32_t *in_b,
                     size_t D, std::vector<uint32_t> &dev_of_gate);

// One device's part of a circuit placed by partition_gates: `inputs` are the
// whole circuit's primary inputs it reads, in its own numbering; in_a / in_b /
// out_wires use that numbering (inputs, then its gates); out_index[k] is the
// whole circuit's output that its k-th output is.
struct SubCircuit {
    std::vector<uint32_t> inputs, in_a, in_b, out_wires, out_index;
    std::vector<uint8_t> ops;
};
std::vector<SubCircuit> split_circuit(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                                      const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires,
                                      const std::vector<uint32_t> &dev_of_gate, size_t D);

// ---- LUT circuits (tfhe_lut.cpp evaluates the plan) -------------------------
// The descriptors of B "linear combination, then bootstrap with table lut[i]" nodes
// over a pool of P ciphertexts and a set of T tables: nullptr, or what is wrong
// (term_off[0] != 0 or not monotone, a source >= P, a table >= T).  lut may be NULL
// (the schedule call has none).
const char *check_lut_nodes(size_t B, size_t P, size_t T, const uint32_t *term_off, const uint32_t *term_src,
                            const uint32_t *lut);
// ASAP levels: level[g] = 1 + the largest level of node g's term wires (inputs are
// level 0; a node without terms is level 1).  Wire w < n_inputs is input w, node g
// drives wire n_inputs + g and reads earlier wires only.  nullptr, or the reason.
// Multi-output form (theta != nullptr, n_nodes entries, each <= TFHE_LUT_MULTI_MAX_LOG): node g
// drives the 2^theta[g] wires n_inputs + o_g + j, o_g = sum_{g' < g} 2^theta[g'], and reads wires
// below n_inputs + o_g only; a wire's level is its node's.
// Select nodes (sel != nullptr, include/tfhe_gpu.h "Select nodes"): node g has the sel->off[g+1] - sel->off[g]
// entries sel->wire[..], 0 (an ordinary node) or m of them; an entry is TFHE_LUT_ENTRY_CONST or a wire below
// n_inputs + o_g, and counts towards the node's level as a term wire does.  A select node has theta 0.
struct LutSelect {
    uint32_t m;
    const uint32_t *off, *wire, *konst;  // konst may be NULL where only levels are asked for
};
const char *schedule_lut_levels(size_t n_inputs, size_t n_nodes, const uint32_t *term_off, const uint32_t *term_wire,
                                std::vector<uint32_t> &level, uint32_t &depth, const uint32_t *theta = nullptr,
                                const LutSelect *sel = nullptr);
// round_theta's shift, s = 32 - (log2 N + 1) + theta; 0 for theta = 0 (the identity, not the formula)
uint32_t lut_round_shift(const tfhe_params &p, uint32_t theta);

// A LUT circuit's evaluation plan.  The device wire table is laid out in
// evaluation order, inputs | nodes of level 1 | nodes of level 2 | ..., as
// plan_circuit lays out a gate circuit's, so a level's bootstrap writes one
// contiguous run of slots.  Level lv (1-based) evaluates the nodes
// order[first[lv-1] .. first[lv]); its CSR offsets are the first[lv] - first[lv-1] + 1
// entries of `off` from first[lv-1] + lv - 1 on and index src / coef directly;
// src holds slots, not wires.  konst / lut / theta are per node in evaluation order.
// Multi-output form: slot is over the n_inputs + sum 2^theta wires, and level lv's outputs are the
// contiguous run of slots n_inputs + ofirst[lv-1] .. n_inputs + ofirst[lv), node by node in evaluation
// order, so the level's key switch writes the wire table directly.  fan holds one (node's index in its
// level, coefficient) pair per output slot, in slot order.  Without theta, ofirst == first.
// Select nodes: a level's run of `order` holds its ordinary nodes (node order), then its select nodes
// (node order), nsel[lv-1] of them, and the output slots follow that order, so level_out stays one run.
// sfirst counts the select nodes below a level as first counts the nodes.  tv_sel is, per node in evaluation
// order, where the item's test vector comes from in the level's bootstrap launch: the table lut for an
// ordinary node, LUT_TV_EACH | k for the level's k-th select node (test vector k of the level's own).
// The entries are one CSR over all select nodes in evaluation order, m per node in pack order: entry j
// has the e_off[j+1] - e_off[j] <= 1 terms e_src[..] (a slot, coefficient 1) and the constant e_konst[j],
// which is what the combine kernel takes; level lv's start at sfirst[lv-1] * m.
// Extended nodes (eta != nullptr, include/tfhe_gpu.h "Extended nodes"): a level's run of `order` is grouped by eta,
// eta = 0 first, and inside each group holds the ordinary nodes, then the select nodes, as above; so the eta = 0
// part of a level is laid out as the whole level is without eta, and each extended group is one run of items and
// of output slots behind it.  neta[3 (lv-1) + e] / nsel_eta[3 (lv-1) + e] count the nodes / the select nodes of
// group e of level lv.  The level's select nodes are numbered (tv_sel, the entries' CSR) in evaluation order across
// the groups, so one staging, pack and spread serves them all.  An extended node has theta 0: one output slot.
// eta holds each node's eta in evaluation order (all 0 without eta).
constexpr uint32_t LUT_TV_EACH = 0x80000000u;
struct LutCircuitPlan {
    uint32_t depth = 0;
    std::vector<uint32_t> level;  // per node
    std::vector<uint32_t> first;  // depth + 1 entries
    std::vector<uint32_t> order;  // the nodes in evaluation order
    std::vector<uint32_t> slot;   // per wire
    std::vector<uint32_t> off, src, konst, lut;
    std::vector<int32_t> coef;
    std::vector<uint32_t> out_slots;
    std::vector<uint32_t> theta;   // per node, evaluation order (all 0 without theta)
    std::vector<uint32_t> ofirst;  // depth + 1 entries
    std::vector<uint32_t> fan;     // 2 words per output slot
    std::vector<uint32_t> nsel;    // per level (depth entries)
    std::vector<uint32_t> sfirst;  // depth + 1 entries
    std::vector<uint32_t> tv_sel;  // per node, evaluation order
    std::vector<uint32_t> e_off, e_src, e_konst;  // sfirst[depth] * m + 1 offsets, the wire entries' slots, one constant per entry
    std::vector<uint32_t> eta;             // per node, evaluation order
    std::vector<uint32_t> neta, nsel_eta;  // 3 per level
};
const char *plan_lut_circuit(size_t n_inputs, size_t n_nodes, const uint32_t *term_off, const uint32_t *term_wire,
                             const int32_t *term_coef, const uint32_t *konst, const uint32_t *lut, size_t T,
                             size_t n_outputs, const uint32_t *out_wires, LutCircuitPlan &pl,
                             const uint32_t *theta = nullptr, const LutSelect *sel = nullptr,
                             const uint32_t *eta = nullptr);
// nullptr, or what is wrong with the etas themselves: one > TFHE_LUT_EXT_MAX_LOG, or eta > 0 with theta > 0 on a node
const char *check_lut_eta(size_t n_nodes, const uint32_t *theta, const uint32_t *eta);

// ---- Packing key switch (tfhe_pack_tlwe here; tfhe_pack.cpp runs it on the device) ----
// The shapes with the one-hot GEMM form (ks_gemm_supported, tfhe_kernels.hip): basebit 2 with
// t 7..9, basebit 5 with t 2..3.
bool pack_shape_ok(uint32_t basebit, uint32_t t);
size_t pack_key_words(const tfhe_params &p, uint32_t basebit, uint32_t t);  // n * t * 2^basebit rows of 2N
// nullptr, or what is wrong with a pack call's shape and coefficient list (C outside 1..N, a
// coefficient >= N or listed twice)
const char *check_pack_args(const tfhe_params &p, uint32_t basebit, uint32_t t, const uint32_t *coef, size_t C);

// ---- CMUX graphs (tfhe_cmux_graph_plan here; tfhe_leveled.cpp evaluates the plan) ----
// level / slot per node; the nodes in evaluation order, order[first[l-1] .. first[l]) being level l
// (1-based; first has depth + 1 entries); n_slots TRLWELv1 of scratch per query.
struct CmuxGraphPlan {
    std::vector<uint32_t> level, slot, order, first;
    uint32_t depth = 0, n_slots = 0;
};
// nullptr, or what is wrong with the graph (include/tfhe_gpu.h "CMUX graphs").
const char *plan_cmux_graph(uint32_t nL, uint32_t V, uint32_t k, const uint32_t *var, const uint32_t *lo,
                            const uint32_t *hi, const uint32_t *rlo, const uint32_t *rhi, uint32_t R,
                            const uint32_t *roots, uint32_t N, CmuxGraphPlan &pl);

// Device d's contiguous slice of B items over D devices: ceil(B/D) each, the
// last non-empty one ragged, the ones after it empty.
struct Slice {
    size_t lo, n;
};
inline Slice slice_of(size_t B, size_t D, size_t d) {
    const size_t per = (B + D - 1) / D, lo = B < d * per ? B : d * per;
    return {lo, (B < lo + per ? B : lo + per) - lo};
}

}  // namespace tfhe
