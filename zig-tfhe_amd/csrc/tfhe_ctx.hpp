// tfhe_ctx.hpp — the two types behind the C handle and what the host units
// share: Device (everything that belongs to one GPU) and tfhe_gpu_ctx (the
// handle: one Device or several), the owners of their HIP resources, error
// reporting, a call's scratch frame (Frame), descriptor upload (DescBlob) and
// host-or-device buffers (Io), and the functions the host units call in each
// other.  Not installed.
#pragma once

#include "tfhe_gpu.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl is dlopen'ed on first multi-device key load

#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "tfhe_cpu.hpp"
#include "tfhe_internal.hpp"
#include "tfhe_scratch.hpp"

namespace tfhe {

// Move-only owner of one HIP resource made on `device`: released in the
// destructor, after hipSetDevice to that device.
template <class T, auto Release>
class Owned {
  public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(o.h_), device_(o.device_) { o.h_ = T{}; }
    Owned &operator=(Owned &&) = delete;
    ~Owned() { reset(); }
    void reset() {
        if (!h_) return;
        (void)hipSetDevice(device_);
        (void)Release(h_);
        h_ = T{};
    }
    // Where hipMalloc / hipEventCreate / ... on `device` (the current one) puts a new resource; the old one goes first.
    T *make(int device) {
        reset();
        device_ = device;
        return &h_;
    }
    operator T() const { return h_; }

  private:
    T h_{};
    int device_ = 0;
};
template <class T>
using DevPtr = Owned<T *, hipFree>;
template <class T>
using HostPtr = Owned<T *, hipHostFree>;  // pinned
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

static_assert(Scratch::KS_INPUT_SLACK == KS_GEMM_INPUT_SLACK, "the scratch arena's key-switch input slack is the GEMM's");

struct PinBuf {  // pinned host buffer, grown on demand (ensure_pinned)
    HostPtr<char> p;
    size_t bytes = 0;
};

// Persistent host workers of one device (the host-buffer pipeline's staging
// copies and its per-stream enqueueing): run(n, f) calls
// f(0..n-1) on n workers (n <= size) and returns when all are done.
class WorkerPool {
  public:
    explicit WorkerPool(int n) {
        for (int i = 0; i < n; i++) th_.emplace_back([this, i] { loop(i); });
    }
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (std::thread &t : th_) t.join();
    }
    void run(int n, const std::function<void(int)> &f) {
        std::unique_lock<std::mutex> g(m_);
        job_ = &f;
        active_ = n;
        pending_ = n;
        gen_++;
        cv_.notify_all();
        done_.wait(g, [this] { return pending_ == 0; });
        job_ = nullptr;
    }

  private:
    void loop(int i) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)> *f = nullptr;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return stop_ || (gen_ != seen && i < active_); });
                if (stop_) return;
                seen = gen_;
                f = job_;
            }
            (*f)(i);
            std::lock_guard<std::mutex> g(m_);
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(int)> *job_ = nullptr;
    int active_ = 0, pending_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

constexpr int PIPE_STREAMS = 4;  // concurrent chunks of the host-buffer pipeline (HIP's 4 hardware queues)

// One GPU of a context: its stream, tables, resident key, scratch and options.
// Members are destroyed last to first: the worker pool stops before the
// pipeline's streams go, and the context's own stream goes last.
struct Device {
    tfhe_params P{};
    KParams K{};
    int device = 0;
    Stream own_stream;
    hipStream_t stream = nullptr;  // own_stream, or the caller's (tfhe_gpu_set_stream)
    Event stream_ev;               // tfhe_gpu_set_stream: the old stream's work, waited for by the new one
    std::string err;               // this device's last failure (lift puts it into the handle's)
    // device error word (KParams::err; DEV_ERR_* bits) and its pinned host copy,
    // read at every synchronisation point (sync_check); words 2-3 of both hold
    // a key fingerprint (key_fingerprint)
    DevPtr<uint32_t> d_err;
    HostPtr<uint32_t> h_err;
    // constant tables
    DevPtr<C2> d_twist, d_tw;
    C2 twa[4] = {};  // host copy of the pass-A twiddles (DevTables::twa)
    // cloud key
    bool has_key = false;
    uint32_t offset = 0;
    std::vector<uint32_t> testvec;  // host copy, 2N
    DevPtr<uint32_t> d_testvec;     // cloud testvec (2N)
    DevPtr<double> d_bk;            // device layout, n*2L*512 double4
    DevPtr<uint32_t> d_ksk;         // reference rows padded to K.ks_stride words (ksk_dev_bytes)
    size_t bk_bytes = 0, ksk_bytes = 0;
    // scratch: the calls' stack of frames (tfhe_scratch.hpp; Frame below), and the one buffer that persists
    Scratch scratch;
    DevPtr<uint8_t> s_ties;  // near-tie flags (KParams::tie_flags), one byte per item, zero between launches:
    size_t ties_cap = 0;     // only a new buffer is memset, so they cannot live in a frame (ensure_tie_flags)
    std::string lut_multi_ks;        // multi-output LUT nodes: what last_ks names after one: the fan-out extraction, then the key switch
    DevPtr<uint32_t> d_ksk_gemm;     // gemm key switch: the MFMA-layout KSK (ks_gemm_bytes), built from d_ksk
    bool ksk_gemm_ok = false;        // d_ksk_gemm matches d_ksk
    Event level_ev;                  // level-split circuits: this device's slice of a level is computed
    // device timing (tfhe_gpu_profile_begin/end): 3 events per bootstrap launch
    bool profiling = false;
    std::vector<Event> events;
    size_t ev_used = 0;
    // kernel-form options (tfhe_gpu_set_option) and what the last launch ran
    LaunchOpts opts{};
    int64_t circuit_pack = 1;
    int64_t pack_scratch_mb = 256;  // TFHE_OPT_PACK_SCRATCH_MB: bound on the packing key switch's GEMM sums per chunk
    int64_t scatter_scratch_mb = 256;  // TFHE_OPT_SCATTER_SCRATCH_MB: bound on the packed scatter-add's leaves per chunk
    int64_t graph_chunk_queries = 0;   // TFHE_OPT_GRAPH_CHUNK_QUERIES: a CMUX graph's queries per chunk at most (0: the 256 MB bound alone)
    int64_t twiddle_source = TFHE_TWIDDLES_GLIBC;
    bool key_from_keygen = false;  // the resident BK was transformed with this device's tables
    double bk_absmax = 0.0;        // largest |BK spectrum component| of the resident key, reference scale
    double bk_row_rms = 0.0;       // largest TRGSW row RMS / 2^31 of the resident key (by Parseval)
    uint64_t near_tie_items = 0;   // items the margin guard recomputed (device err[1], read by sync_check)
    const char *last_br = "", *last_ks = "";
    // blind rotations launched on this device since creation (tfhe_gpu_device_bootstraps)
    uint64_t bootstraps = 0;
    // host-buffer pipeline (pipelined_bootstrap): streams, pinned staging, workers
    Stream pipe[PIPE_STREAMS];
    Event pipe_ev;
    PinBuf pin_in, pin_out;
    std::unique_ptr<WorkerPool> workers;
    int64_t pipeline = 0;  // TFHE_OPT_HOST_PIPELINE (off by default: measured slower)
    // host-buffer copies through pinned staging (TFHE_OPT_HOST_STAGING; h2d / d2h_sync): the
    // arena's bytes in use since the last synchronisation of this device's stream
    int64_t host_staging = TFHE_STAGING_PAGEABLE;
    PinBuf stage_in, stage_out;
    size_t stage_used = 0;
};

}  // namespace tfhe

// The C handle: one Device (tfhe_gpu_create_on_device) or one per listed device
// (tfhe_gpu_create_multi; a device listed twice is two Devices).  dev[0] loads
// keys and serves the calls that take one device.
struct tfhe_gpu_ctx {
    tfhe_params P{};
    std::vector<tfhe::Device> dev;  // never empty; reserved at creation, so its elements stay put
    std::string err;
    std::string last_kernels;
    // created by tfhe_gpu_create_multi: key loads end in the RCCL broadcast (even over
    // one device); a context of tfhe_gpu_create_on_device never touches RCCL
    bool multi = false;
    bool distinct_devices = true;    // RCCL needs each device once; else D2D copies
    std::vector<ncclComm_t> comms;   // one communicator per device, created on the first key broadcast
    int64_t circuit_split = 0;       // TFHE_OPT_CIRCUIT_SPLIT
    int64_t level_issue_us = 0;      // host time the last level-split circuit spent issuing (TFHE_OPT_LEVEL_ISSUE_US)
};

// A packing key resident on one device: the MFMA layout of its rows only (pack_gemm_bytes).  Loaded and
// run by tfhe_pack.cpp; the bivariate LUT bootstrap (tfhe_lut.cpp) packs with it too.
struct tfhe_gpu_packing_key {
    const tfhe_gpu_ctx *ctx = nullptr;  // the context that loaded it (identity only, never dereferenced)
    tfhe_params P{};
    uint32_t basebit = 0, t = 0;
    tfhe::DevPtr<uint32_t> key_gemm;
};

namespace tfhe {

inline int fail(tfhe_gpu_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}
inline int fail(Device &d, int code, const std::string &msg) {
    d.err = msg;
    return code;
}
template <class C>  // a handle (tfhe_gpu_ctx *) or a Device
int hip_fail(C &c, hipError_t e, const char *where) {
    return fail(c, TFHE_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e));
}

#define HIPCHK(c, expr)                                         \
    do {                                                        \
        hipError_t _e = (expr);                                 \
        if (_e != hipSuccess) return hip_fail((c), _e, #expr);  \
    } while (0)

// A device's failure `rc` becomes the handle's: device 0's message as it is,
// another's behind "device <id>: ".
inline int lift(tfhe_gpu_ctx *c, size_t slot, int rc) {
    if (rc) c->err = slot ? "device " + std::to_string(c->dev[slot].device) + ": " + c->dev[slot].err : c->dev[0].err;
    return rc;
}
inline bool is_multi(const tfhe_gpu_ctx *c) { return c && c->dev.size() > 1; }  // over more than one Device

// f(device, slot, first item, count) on every device's slice of B items
// (slice_of), concurrently: one host thread per non-empty slice beyond device
// 0's, which runs on the calling thread.  The handle of one device calls f
// there and then, an empty batch included (f's own refusals come before its
// B == 0 return).  The first failing slot's failure becomes the handle's.
template <class F>
int for_each_slice(tfhe_gpu_ctx *c, size_t B, F f) {
    const size_t D = c->dev.size();
    if (D == 1) return lift(c, 0, f(c->dev[0], (size_t)0, (size_t)0, B));
    std::vector<int> rc(D, TFHE_OK);
    std::vector<std::thread> th;
    for (size_t d = D; d-- > 0;) {
        const Slice s = slice_of(B, D, d);
        if (!s.n) continue;
        if (d) th.emplace_back([&, d, s] { rc[d] = f(c->dev[d], d, s.lo, s.n); });
        else rc[0] = f(c->dev[0], d, s.lo, s.n);
    }
    for (std::thread &t : th) t.join();
    for (size_t d = 0; d < D; d++)
        if (rc[d]) return lift(c, d, rc[d]);
    return TFHE_OK;
}

// f(device 0), with that device current, for an entry point that works on one device; a
// failure is lifted into the handle's.
template <class F>
int on_device0(tfhe_gpu_ctx *c, F f) {
    Device &d = c->dev[0];
    const hipError_t e = hipSetDevice(d.device);
    return lift(c, 0, e == hipSuccess ? f(d) : hip_fail(d, e, "hipSetDevice(d.device)"));
}

// Refuses a resident set (`what`: "selector set", "LUT set") that does not belong to this
// context and its parameter set.
template <class Set>
int set_mismatch(tfhe_gpu_ctx *c, const Set *set, const char *what) {
    const char *why = nullptr;
    if (set->ctx != c) why = "on another context";
    else if (std::memcmp(&set->P, &c->P, sizeof(tfhe_params)) != 0) why = "for another parameter set";
    return why ? fail(c, TFHE_ERR_INVALID, std::string("the ") + what + " was loaded " + why) : TFHE_OK;
}

inline size_t tlwe0_words(const tfhe_params &p) { return (size_t)p.n + 1; }
inline double level_cost(size_t items, size_t cus) { return blind_rotate_cost(items, cus); }  // the planner's CostModel

// What a blind-rotation launch hands back.
enum RunKind : int {
    RUN_BOOTSTRAP = 0,     // sample extract + key switch: TLWELv0 (vanilla.zig:38-52)
    RUN_TRLWE = 1,         // the accumulator: TRLWELv1 (trgsw.zig:290-333)
    RUN_NO_KEYSWITCH = 2,  // sampleExtractIndex2, n+1 words (vanilla.zig:58-69)
};

// ---- tfhe_gpu.cpp, for the other host units --------------------------------------
int h2d_copy(Device &d, void *dst, const void *src, size_t bytes);    // host -> device memory, async on the device's stream

// A frame of one device's scratch (tfhe_scratch.hpp).  Every entry point's _on function opens the call's
// outermost one, and whatever has temporaries of its own (a bootstrap launch, a level, a chunk) a nested
// one.  A slice is its taker's until the frame closes.  Reuse after that is safe because everything a call
// launches is on the device's stream, or on the pipeline's streams, which the call joins before it returns.
struct Frame : Scratch::Frame {
    Device &d;
    explicit Frame(Device &dv) : Scratch::Frame(dv.scratch), d(dv) {}
    // host -> a new slice, async on the device's stream: the device copy, or NULL (rc())
    template <class T>
    const T *h2d(const T *src, size_t n_bytes) {
        void *p = bytes(n_bytes);
        if (!p) return nullptr;
        if (const int rc = h2d_copy(d, p, src, n_bytes)) return fail(rc), nullptr;
        return static_cast<const T *>(p);
    }
};

// Descriptor arrays of one call, concatenated into one upload (u32 words; signed
// coefficients keep their bits): where each starts in the device copy.
struct DescBlob {
    std::vector<uint32_t> words;
    size_t add(const void *p, size_t count) {
        const size_t at = reserve(count);
        if (count) std::memcpy(words.data() + at, p, count * sizeof(uint32_t));
        return at;
    }
    size_t add_bytes(const void *p, size_t count) {  // padded to words
        const size_t at = reserve((count + 3) / 4);
        if (count) std::memcpy(words.data() + at, p, count);
        return at;
    }
    size_t reserve(size_t count) {  // zeros, for the caller to fill
        const size_t at = words.size();
        words.resize(at + count);
        return at;
    }
    // The device copy in a slice of f (NULL: f.rc()).  The blob is pageable: hipMemcpyAsync stages it
    // before it returns, so the blob may go while the copy is still in flight (a _dev call does not sync).
    const uint32_t *upload(Frame &f) const {
        return words.empty() ? f.take<uint32_t>(1) : f.h2d(words.data(), words.size() * sizeof(uint32_t));
    }
};

DevTables tables(const Device &d);
int ks_gemm_args(Frame &f, size_t B, KsGemm &G);                      // the gemm key switch's buffers for B items
int set_key_common(Device &d, uint32_t offset, const uint32_t *tv_a, const uint32_t *tv_b);
int upload_ksk(Device &d, const uint32_t *ksk);                       // host KSK (reference layout) -> device KSK, async
int key_loaded(Device &d, bool from_keygen);                          // the end of every key load on device 0: admission
int key_fingerprint(Device &d, uint64_t &bk, uint64_t &ksk);
int run_bootstrap_dev(Device &d, const uint8_t *ops, const uint32_t *a, const uint32_t *b, const uint32_t *testvec_dev,
                      uint32_t *out, size_t B, int kind, const uint32_t *idx = nullptr, const uint32_t *tv_sel = nullptr,
                      const uint32_t *tv_each = nullptr);
int sync_check(Device &d);
int d2h_sync(Device &d, void *dst, const void *src, size_t bytes);
// A circuit plan on one device, in slices of f: the wire table with the inputs, the gather indices and the op codes.
struct PlanBufs {
    uint32_t *wires = nullptr;
    const uint32_t *idx = nullptr;
    const uint8_t *ops = nullptr;
};
int upload_plan(Frame &f, const CircuitPlan &pl, size_t W, size_t n_inputs, const uint32_t *inputs, PlanBufs &pb,
                bool inputs_on_device = false);
int circuit_eval_one(Device &d, size_t n_inputs, const uint32_t *inputs, size_t n_gates, const uint8_t *ops,
                     const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires,
                     uint32_t *outputs, uint32_t *depth_out, bool dev = false);

// The buffers of one call on one device.  Host buffers (dev = false) are staged through the
// call's frame: in() uploads one, out() takes room for one and inout() does both for a buffer
// the call updates, each leaving its pointer at the slice for the launches that follow, and
// finish() copies the output back and waits.  Device pointers (dev = true) stay as they are,
// and nothing is waited for.
struct Io {
    Frame &f;
    bool dev;
    void *host_out = nullptr;  // out() / inout(): the caller's buffer, its slice and size
    const void *staged_out = nullptr;
    size_t out_bytes = 0;

    template <class T>
    int in(const T *&p, size_t bytes) {
        if (!dev) p = f.h2d(p, bytes);
        return f.rc();
    }
    template <class T>
    int out(T *&p, size_t bytes) {
        return dev ? f.rc() : staged(p, bytes, f.bytes(bytes));
    }
    template <class T>
    int inout(T *&p, size_t bytes) {
        return dev ? f.rc() : staged(p, bytes, const_cast<T *>(f.h2d(p, bytes)));
    }
    // The host call waits: for its output, or without one for the work and the error word.
    int finish() {
        if (dev) return TFHE_OK;
        return host_out ? d2h_sync(f.d, host_out, staged_out, out_bytes) : sync_check(f.d);
    }

  private:
    template <class T>
    int staged(T *&p, size_t bytes, void *slice) {
        host_out = p;
        out_bytes = bytes;
        staged_out = p = static_cast<T *>(slice);
        return f.rc();
    }
};

// ---- tfhe_pack.cpp, for tfhe_lut.cpp --------------------------------------------
// Items per chunk of a pack of `items` inputs: what keeps the GEMM sums within TFHE_OPT_PACK_SCRATCH_MB.
size_t pack_chunk_items(const Device &d, size_t items, int basebit);
// The pack's launches over device buffers, async: x = B * C TLWELv0 from Frame::ks_input(.., pack) for its
// readable bytes past the last, coef = C device words, out = B TRLWELv1; chunked by pack_chunk_items.
int pack_launch(Device &d, const tfhe_gpu_packing_key &key, const uint32_t *x, const uint32_t *coef_dev, size_t C,
                uint32_t *out, size_t B);

// ---- tfhe_multi.cpp, for tfhe_gpu.cpp ------------------------------------------
int enable_peer_access(const std::vector<int> &devs, std::string &why);
int broadcast_key(tfhe_gpu_ctx *c);
void destroy_comms(tfhe_gpu_ctx *c);
int circuit_eval_multi(tfhe_gpu_ctx *c, size_t n_inputs, const uint32_t *inputs, size_t n_gates, const uint8_t *ops,
                       const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires,
                       uint32_t *outputs, uint32_t *depth_out);

}  // namespace tfhe
