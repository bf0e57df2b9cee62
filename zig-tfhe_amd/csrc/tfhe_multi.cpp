// tfhe_multi.cpp — what only a context over several devices runs
// (tfhe_gpu_create_multi): peer access, the RCCL loader, the
// key broadcast, and circuits split over the devices.  Host code, compiled like
// tfhe_gpu.cpp; the types and the per-device functions are in tfhe_ctx.hpp.
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <deque>
#include <mutex>

#include "tfhe_ctx.hpp"

namespace tfhe {

// Peer access for every ordered pair of distinct devices: the level split
// all-gathers between all of them.
int enable_peer_access(const std::vector<int> &devs, std::string &why) {
    for (int a : devs)
        for (int b : devs) {
            if (a == b) continue;
            int can = 0;
            hipError_t e = hipDeviceCanAccessPeer(&can, a, b);
            if (e != hipSuccess || !can) {
                why = "device " + std::to_string(a) + " cannot access device " + std::to_string(b) +
                      "'s memory (hipDeviceCanAccessPeer" + (e != hipSuccess ? std::string(": ") + hipGetErrorString(e) : "") +
                      "): the multi-device context needs xGMI peer access";
                return TFHE_ERR_DEVICE;
            }
            e = hipSetDevice(a);
            if (e == hipSuccess) e = hipDeviceEnablePeerAccess(b, 0);
            if (e == hipErrorPeerAccessAlreadyEnabled) {
                (void)hipGetLastError();  // clear the sticky status of an already-enabled pair
                e = hipSuccess;
            }
            if (e != hipSuccess) {
                why = "hipDeviceEnablePeerAccess(" + std::to_string(a) + " -> " + std::to_string(b) + "): " + hipGetErrorString(e);
                return TFHE_ERR_DEVICE;
            }
        }
    (void)hipSetDevice(devs[0]);
    return TFHE_OK;
}

// librccl, loaded on the first multi-device key broadcast.  dlopen keeps the
// library loadable where RCCL is absent and, under PyTorch, reuses the RCCL
// that torch has already mapped (same SONAME) instead of a second copy.
struct RcclApi {
    decltype(&ncclCommInitAll) comm_init_all = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclBroadcast) broadcast = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
};

static const RcclApi *rccl_api(std::string &why) {
    static std::once_flag once;
    static RcclApi api;
    static std::string load_error;
    std::call_once(once, [] {
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW);
        if (!h) {
            load_error = std::string("cannot load librccl.so.1: ") + dlerror();
            return;
        }
        api.comm_init_all = (decltype(api.comm_init_all))dlsym(h, "ncclCommInitAll");
        api.comm_destroy = (decltype(api.comm_destroy))dlsym(h, "ncclCommDestroy");
        api.broadcast = (decltype(api.broadcast))dlsym(h, "ncclBroadcast");
        api.group_start = (decltype(api.group_start))dlsym(h, "ncclGroupStart");
        api.group_end = (decltype(api.group_end))dlsym(h, "ncclGroupEnd");
        api.error_string = (decltype(api.error_string))dlsym(h, "ncclGetErrorString");
        if (!api.comm_init_all || !api.comm_destroy || !api.broadcast || !api.group_start || !api.group_end ||
            !api.error_string)
            load_error = "librccl.so.1 lacks an nccl* entry point";
    });
    why = load_error;
    return load_error.empty() ? &api : nullptr;
}

void destroy_comms(tfhe_gpu_ctx *c) {
    if (c->comms.empty()) return;
    std::string why;
    if (const RcclApi *r = rccl_api(why))
        for (ncclComm_t m : c->comms)
            if (m) r->comm_destroy(m);
    c->comms.clear();
}

// The key just loaded (and admitted) on device 0 -> every other device of a
// multi-device context: one ncclBroadcast of the device BK and KSK (RCCL over
// xGMI), or a device-to-device copy when a device appears twice.  The test
// vector / offset are host state (8 KB).  A context of
// tfhe_gpu_create_on_device has nothing to do here.
int broadcast_key(tfhe_gpu_ctx *c) {
    if (!c->multi) return TFHE_OK;
    const size_t D = c->dev.size();
    Device &root = c->dev[0];  // the source; the key goes to devices 1..D-1
    for (size_t d = 1; d < D; d++) {
        Device &s = c->dev[d];
        s.has_key = false;
        HIPCHK(c, hipSetDevice(s.device));
        const int rc = set_key_common(s, root.offset, root.testvec.data(), root.testvec.data() + c->P.N);
        if (rc) return lift(c, d, rc);
        HIPCHK(c, hipStreamSynchronize(s.stream));
    }
    if (c->distinct_devices) {
        std::string why;
        const RcclApi *r = rccl_api(why);
        if (!r) return fail(c, TFHE_ERR_HIP, why);
        if (c->comms.empty()) {
            std::vector<int> devs(D);
            for (size_t d = 0; d < D; d++) devs[d] = c->dev[d].device;
            c->comms.assign(D, nullptr);
            ncclResult_t e = r->comm_init_all(c->comms.data(), (int)D, devs.data());
            if (e != ncclSuccess) {
                c->comms.clear();
                return fail(c, TFHE_ERR_HIP, std::string("ncclCommInitAll: ") + r->error_string(e));
            }
        }
        ncclResult_t e = r->group_start();
        for (size_t d = 0; d < D && e == ncclSuccess; d++) {
            Device &s = c->dev[d];
            e = r->broadcast(root.d_bk, s.d_bk, root.bk_bytes, ncclUint8, 0, c->comms[d], s.stream);
            if (e == ncclSuccess) e = r->broadcast(root.d_ksk, s.d_ksk, root.ksk_bytes, ncclUint8, 0, c->comms[d], s.stream);
        }
        ncclResult_t e2 = r->group_end();
        if (e == ncclSuccess) e = e2;
        if (e != ncclSuccess) return fail(c, TFHE_ERR_HIP, std::string("ncclBroadcast: ") + r->error_string(e));
    } else {
        for (size_t d = 1; d < D; d++) {
            Device &s = c->dev[d];
            HIPCHK(c, hipSetDevice(s.device));
            HIPCHK(c, hipMemcpyPeerAsync(s.d_bk, s.device, root.d_bk, root.device, root.bk_bytes, s.stream));
            HIPCHK(c, hipMemcpyPeerAsync(s.d_ksk, s.device, root.d_ksk, root.device, root.ksk_bytes, s.stream));
        }
    }
    for (size_t d = D; d-- > 0;) {  // every copy landed; device 0 last, which stays the current one
        Device &s = c->dev[d];
        HIPCHK(c, hipSetDevice(s.device));
        HIPCHK(c, hipStreamSynchronize(s.stream));
        s.ksk_gemm_ok = false;
    }
    // every copy must fingerprint like the source's before a device may use it
    uint64_t bk0 = 0, ksk0 = 0;
    for (size_t d = 0; d < D; d++) {
        Device &s = c->dev[d];
        uint64_t bk = 0, ksk = 0;
        if (const int rc = key_fingerprint(s, bk, ksk)) return lift(c, d, rc);
        if (d == 0) bk0 = bk, ksk0 = ksk;
        if (bk != bk0 || ksk != ksk0)
            return fail(c, TFHE_ERR_HIP, "key broadcast: the copy on device " + std::to_string(s.device) +
                                             " differs from device " + std::to_string(root.device) + "'s");
        s.bk_absmax = root.bk_absmax;  // same bits, same admission
        s.bk_row_rms = root.bk_row_rms;
        s.opts.key_fused_ok = root.opts.key_fused_ok;
        s.has_key = true;
    }
    HIPCHK(c, hipSetDevice(root.device));
    return TFHE_OK;
}

// Level split or components (TFHE_OPT_CIRCUIT_SPLIT: 0 auto, 1 components, 2
// levels).  Auto: levels when the component placement leaves the busiest device
// more than 10 % above an even share of at least one whole-form round per device
// (e.g. one big connected circuit); components otherwise (independent gates,
// MUXes and adders place evenly, and nothing crosses devices).
static bool split_by_levels(const tfhe_gpu_ctx *c, size_t n_gates, const uint8_t *ops, const std::vector<uint32_t> &dev) {
    if (c->circuit_split != 0) return c->circuit_split == 2;
    const size_t D = c->dev.size();
    std::vector<uint64_t> load(D, 0);
    uint64_t total = 0;
    for (size_t g = 0; g < n_gates; g++)
        if (ops[g] != TFHE_GATE_NOT) {
            load[dev[g]]++;
            total++;
        }
    const uint64_t even = (total + D - 1) / D;
    return even >= 4 * device_cus() && *std::max_element(load.begin(), load.end()) * 10 > even * 11;
}

// circuit_eval over the devices, level by level ("a level barrier
// across GPUs"), for circuits whose gates form one dominant connected
// component.  Every device holds the whole wire table in the same layout (the
// plan of circuit_eval_one, its level packing modelled on all devices' CUs)
// and the primary inputs.  Per level, device d bootstraps its slice (slice_of)
// of the level's gates into its table; each slice is then copied to every other
// device (peer copies over xGMI, ordered by an event on the producer's stream:
// an all-gather), and every device applies the level's NOTs itself.  Outputs
// come from the first device's table.  Every device's frame stays open for the
// whole call: the wire tables are the peer copies' sources and targets.
static int circuit_eval_levels(tfhe_gpu_ctx *c, size_t n_inputs, const uint32_t *inputs, size_t n_gates,
                               const uint8_t *ops, const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs,
                               const uint32_t *out_wires, uint32_t *outputs, uint32_t *depth_out) {
    const size_t W = n_inputs + n_gates, D = c->dev.size(), w1 = tlwe0_words(c->P);
    CircuitPlan pl;
    if (const char *why = plan_circuit(n_inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires,
                                       c->dev[0].circuit_pack != 0, device_cus() * D, level_cost, pl))
        return fail(c, TFHE_ERR_INVALID, why);
    std::deque<Frame> frames;  // one per device
    std::vector<PlanBufs> pb(D);
    for (size_t d = 0; d < D; d++) {
        Device &s = c->dev[d];
        frames.emplace_back(s);
        int rc = upload_plan(frames[d], pl, W, n_inputs, inputs, pb[d]);
        if (!rc && !s.level_ev && hipEventCreateWithFlags(s.level_ev.make(s.device), hipEventDisableTiming) != hipSuccess)
            rc = fail(s, TFHE_ERR_HIP, "hipEventCreate");
        if (rc) return lift(c, d, rc);
    }
    size_t ip = 0, op_pos = 0, sp = n_inputs;
    // the per-level issue (launches, peer copies, event waits) runs on this one
    // host thread for all devices; it is asynchronous, so it costs wall time only
    // where it outruns the devices' per-level work (measured: DESIGN.md §7)
    const auto t_issue = std::chrono::steady_clock::now();
    for (uint32_t lv = 0; lv <= pl.max_level; lv++) {
        const size_t nb = pl.bs[lv].size(), nn = pl.nots[lv].size();
        if (nb) {
            for (size_t d = 0; d < D; d++) {  // each device its slice
                Device &s = c->dev[d];
                const Slice sl = slice_of(nb, D, d);
                if (!sl.n) continue;
                if (hipSetDevice(s.device) != hipSuccess) return fail(c, TFHE_ERR_HIP, "hipSetDevice");
                uint32_t *wires = pb[d].wires;
                int rc = run_bootstrap_dev(s, pb[d].ops + op_pos + sl.lo, wires, wires, nullptr, wires + (sp + sl.lo) * w1,
                                           sl.n, RUN_BOOTSTRAP, pb[d].idx + ip + 2 * sl.lo);
                if (!rc && hipEventRecord(s.level_ev, s.stream) != hipSuccess) rc = fail(s, TFHE_ERR_HIP, "hipEventRecord");
                if (rc) return lift(c, d, rc);
            }
            for (size_t to = 0; to < D; to++) {  // all-gather of the level's outputs
                Device &t = c->dev[to];
                if (hipSetDevice(t.device) != hipSuccess) return fail(c, TFHE_ERR_HIP, "hipSetDevice");
                for (size_t d = 0; d < D; d++) {
                    Device &s = c->dev[d];
                    const Slice sl = slice_of(nb, D, d);
                    if (&s == &t || !sl.n) continue;
                    const size_t off = (sp + sl.lo) * w1;
                    if (hipStreamWaitEvent(t.stream, s.level_ev, 0) != hipSuccess ||
                        hipMemcpyPeerAsync(pb[to].wires + off, t.device, pb[d].wires + off, s.device, sl.n * w1 * 4,
                                           t.stream) != hipSuccess)
                        return fail(c, TFHE_ERR_HIP, "level all-gather to device " + std::to_string(t.device));
                }
            }
            ip += 2 * nb;
            op_pos += nb;
            sp += nb;
        }
        if (nn) {
            for (size_t d = 0; d < D; d++) {  // every device negates the level's NOT inputs itself
                Device &s = c->dev[d];
                uint32_t *wires = pb[d].wires;
                if (hipSetDevice(s.device) != hipSuccess ||
                    launch_tlwe_gather(s.K, wires, pb[d].idx + ip, wires + sp * w1, nn, true, s.stream) != hipSuccess)
                    return fail(c, TFHE_ERR_HIP, "NOT gather on device " + std::to_string(s.device));
            }
            ip += nn;
            sp += nn;
        }
    }
    c->level_issue_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_issue).count();
    // every device's work done and its error word clean; device 0 last, whose wait brings the outputs
    for (size_t d = D; d-- > 0;) {
        Device &s = c->dev[d];
        Io io{frames[d], /*dev*/ false};
        if (hipSetDevice(s.device) != hipSuccess) return fail(c, TFHE_ERR_HIP, "hipSetDevice");
        if (d == 0 && n_outputs) {
            if (const int rc = io.out(outputs, n_outputs * w1 * 4)) return lift(c, d, rc);
            if (launch_tlwe_gather(s.K, pb[d].wires, pb[d].idx + ip, outputs, n_outputs, false, s.stream) != hipSuccess)
                return fail(c, TFHE_ERR_HIP, "output gather");
        }
        if (const int rc = io.finish()) return lift(c, d, rc);
    }
    if (depth_out) *depth_out = pl.max_level;
    return TFHE_OK;
}

// circuit_eval over the devices.  Primary inputs are read-only, so every
// device gets its own copy of the ones it reads; only gate-to-gate wires tie
// gates together.  The connected components of the gate DAG under those wires
// go whole to one device each, largest first onto the least-loaded device
// (bootstrapped gates), so each device evaluates an independent sub-circuit
// (split_circuit) with its own level schedule and no wire crosses devices.
// Config 4's independent AND/OR/XOR gates and MUXes over shared inputs
// (gates.zig:124-129) spread evenly; one adder
// (examples/add_two_numbers.zig:24-73) stays whole.
int circuit_eval_multi(tfhe_gpu_ctx *c, size_t n_inputs, const uint32_t *inputs, size_t n_gates, const uint8_t *ops,
                       const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires,
                       uint32_t *outputs, uint32_t *depth_out) {
    if (!c->dev[0].has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    if (n_inputs + n_gates > 0xFFFFFFFFull) return fail(c, TFHE_ERR_INVALID, "too many wires");
    const size_t D = c->dev.size(), w1 = tlwe0_words(c->P);
    // validate the whole graph first (same errors as one device)
    if (const char *why = check_circuit(n_inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires))
        return fail(c, TFHE_ERR_INVALID, why);
    std::vector<uint32_t> dev_of_gate;
    partition_gates(n_inputs, n_gates, ops, in_a, in_b, D, dev_of_gate);
    if (split_by_levels(c, n_gates, ops, dev_of_gate))
        return circuit_eval_levels(c, n_inputs, inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires, outputs, depth_out);
    const std::vector<SubCircuit> sub = split_circuit(n_inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires, dev_of_gate, D);
    std::vector<std::vector<uint32_t>> sub_out(D);
    std::vector<uint32_t> sub_levels(D, 0);
    // one "item" per device: every device evaluates its sub-circuit, concurrently
    const int rc = for_each_slice(c, D, [&](Device &dev, size_t d, size_t, size_t) -> int {
        const SubCircuit &s = sub[d];
        if (s.ops.empty() && s.out_wires.empty()) return TFHE_OK;
        std::vector<uint32_t> in(s.inputs.size() * w1);
        for (size_t i = 0; i < s.inputs.size(); i++)
            std::memcpy(in.data() + i * w1, inputs + (size_t)s.inputs[i] * w1, w1 * 4);
        sub_out[d].resize(s.out_wires.size() * w1);
        return circuit_eval_one(dev, s.inputs.size(), in.data(), s.ops.size(), s.ops.data(), s.in_a.data(), s.in_b.data(),
                                s.out_wires.size(), s.out_wires.data(), sub_out[d].data(), &sub_levels[d]);
    });
    if (rc) return rc;
    for (size_t d = 0; d < D; d++)
        for (size_t k = 0; k < sub[d].out_index.size(); k++)
            std::memcpy(outputs + (size_t)sub[d].out_index[k] * w1, sub_out[d].data() + k * w1, w1 * 4);
    if (depth_out) *depth_out = *std::max_element(sub_levels.begin(), sub_levels.end());
    return TFHE_OK;
}

}  // namespace tfhe
