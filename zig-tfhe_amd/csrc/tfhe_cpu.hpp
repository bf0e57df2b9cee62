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
