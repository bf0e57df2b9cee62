// tfhe_gpu.cpp — C-ABI implementation (include/tfhe_gpu.h): contexts, device
// key residency, batch entry points and seeded key generation.  Host code;
// all bootstrap arithmetic runs in tfhe_kernels.hip.  The functions that take
// no context, and the circuit planner, are in tfhe_cpu.cpp (no HIP).
#include "tfhe_gpu.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl is dlopen'ed on first multi-device key load

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "host_math.hpp"
#include "tfhe_cpu.hpp"
#include "tfhe_internal.hpp"

using namespace tfhe;

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

// Persistent host workers of one context (the host-buffer pipeline's staging
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
    int size() const { return (int)th_.size(); }
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

struct tfhe_gpu_ctx {
    tfhe_params P{};
    KParams K{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    hipEvent_t stream_ev = nullptr;  // tfhe_gpu_set_stream: the old stream's work, waited for by the new one
    std::string err;
    // device error word (KParams::err; DEV_ERR_* bits) and its pinned host copy,
    // read at every synchronisation point (sync_check); words 2-3 of both hold
    // a key fingerprint (key_fingerprint)
    uint32_t *d_err = nullptr;
    uint32_t *h_err = nullptr;
    // constant tables
    C2 *d_twist = nullptr, *d_tw = nullptr;
    C2 twa[4] = {};  // host copy of the pass-A twiddles (DevTables::twa)
    // cloud key
    bool has_key = false;
    uint32_t offset = 0;
    std::vector<uint32_t> testvec;  // host copy, 2N
    uint32_t *d_testvec = nullptr;  // cloud testvec (2N)
    double *d_bk = nullptr;         // device layout, n*2L*512 double4
    uint32_t *d_ksk = nullptr;      // reference rows padded to K.ks_stride words (ksk_dev_bytes)
    size_t bk_bytes = 0, ksk_bytes = 0;
    // scratch, grown on demand
    DevBuf s_a, s_b, s_out, s_lv1, s_ops, s_tv, s_tmp;
    DevBuf s_wires, s_cidx, s_cops;  // circuit evaluator: wire table, gather indices, op codes
    DevBuf s_ties;                   // near-tie flags (KParams::tie_flags), one byte per item, zero between launches
    DevBuf s_kspart;                 // gemm key switch: the K splits' partial sums
    uint32_t *d_ksk_gemm = nullptr;  // gemm key switch: the MFMA-layout KSK (ks_gemm_bytes), built from d_ksk
    bool ksk_gemm_ok = false;        // d_ksk_gemm matches d_ksk
    // device timing (tfhe_gpu_profile_begin/end): 3 events per bootstrap launch
    bool profiling = false;
    std::vector<hipEvent_t> events;
    size_t ev_used = 0;
    // kernel-form options (tfhe_gpu_set_option) and what the last launch ran
    LaunchOpts opts{};
    int64_t circuit_pack = 1;
    int64_t circuit_split = 0;  // TFHE_OPT_CIRCUIT_SPLIT
    int64_t twiddle_source = TFHE_TWIDDLES_GLIBC;
    bool key_from_keygen = false;  // the resident BK was transformed with this context's tables
    double bk_absmax = 0.0;        // largest |BK spectrum component| of the resident key, reference scale
    double bk_row_rms = 0.0;       // largest TRGSW row RMS / 2^31 of the resident key (by Parseval)
    int64_t level_issue_us = 0;    // host time the last level-split circuit spent issuing (TFHE_OPT_LEVEL_ISSUE_US)
    uint64_t near_tie_items = 0;   // items the margin guard recomputed (device err[1], read by sync_check)
    const char *last_br = "", *last_ks = "";
    std::string last_kernels;
    // multi-device context (tfhe_gpu_create_multi): shards[0] is this context
    // (device devices[0]); shards[k > 0] are owned single-device contexts.
    // Empty for a single-device context.
    std::vector<tfhe_gpu_ctx *> shards;
    bool distinct_devices = true;    // RCCL needs each device once; else D2D copies
    // blind rotations launched on this device since creation (tfhe_gpu_device_bootstraps)
    uint64_t bootstraps = 0;
    // host-buffer pipeline (pipelined_bootstrap): streams, pinned staging, workers
    hipStream_t pipe[PIPE_STREAMS] = {};
    hipEvent_t pipe_ev = nullptr;
    char *pin_in = nullptr, *pin_out = nullptr;
    size_t pin_in_bytes = 0, pin_out_bytes = 0;
    std::unique_ptr<WorkerPool> workers;
    int64_t pipeline = 0;  // TFHE_OPT_HOST_PIPELINE (off by default: measured slower)
    // host-buffer copies through pinned staging (TFHE_OPT_HOST_STAGING; h2d / d2h_sync): the
    // arena's bytes in use since the last synchronisation of this context's stream
    int64_t host_staging = TFHE_STAGING_PAGEABLE;
    char *stage_in = nullptr, *stage_out = nullptr;
    size_t stage_in_bytes = 0, stage_out_bytes = 0, stage_used = 0;
    std::vector<ncclComm_t> comms;   // one communicator per shard, created on the first key broadcast
};

namespace {

int fail(tfhe_gpu_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}

// the calling thread's last failed create (tfhe_gpu_last_error(NULL))
thread_local std::string g_create_error;
static int create_fail(int code, const std::string &msg) {
    g_create_error = msg;
    return code;
}

int hip_fail(tfhe_gpu_ctx *c, hipError_t e, const char *where) {
    return fail(c, TFHE_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e));
}

#define HIPCHK(c, expr)                                         \
    do {                                                        \
        hipError_t _e = (expr);                                 \
        if (_e != hipSuccess) return hip_fail((c), _e, #expr);  \
    } while (0)

int ensure(tfhe_gpu_ctx *c, DevBuf &b, size_t bytes) {
    if (b.bytes >= bytes) return TFHE_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
    size_t want = std::max<size_t>(bytes, 4096);
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) return fail(c, TFHE_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e));
    b.bytes = want;
    return TFHE_OK;
}

DevTables tables(const tfhe_gpu_ctx *c) {
    return DevTables{c->d_twist, c->d_tw, {c->twa[0], c->twa[1], c->twa[2], c->twa[3]}};
}

size_t tlwe0_words(const tfhe_gpu_ctx *c) { return (size_t)c->P.n + 1; }
double level_cost(size_t items, size_t cus) { return blind_rotate_cost(items, cus); }  // the planner's CostModel
// device KSK: padded rows + zero tail (tfhe_internal.hpp)
size_t ksk_dev_bytes(const tfhe_params &p) {
    return (ksk_rows(p) * ks_stride_for((int)p.n) + KS_TAIL_WORDS) * sizeof(uint32_t);
}

// host KSK (reference layout) -> device KSK (padded rows), async on the ctx stream
int upload_ksk(tfhe_gpu_ctx *c, const uint32_t *ksk) {
    const size_t w = c->P.n + 1, stride = c->K.ks_stride;
    c->ksk_gemm_ok = false;
    HIPCHK(c, hipMemsetAsync(c->d_ksk, 0, c->ksk_bytes, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(c->d_ksk, stride * 4, ksk, w * 4, w * 4, ksk_rows(c->P), hipMemcpyHostToDevice,
                               c->stream));
    return TFHE_OK;
}

int set_key_common(tfhe_gpu_ctx *c, uint32_t offset, const uint32_t *tv_a, const uint32_t *tv_b) {
    const uint32_t N = c->P.N;
    c->offset = offset;
    c->K.offset = offset;
    c->testvec.assign(tv_a, tv_a + N);
    c->testvec.insert(c->testvec.end(), tv_b, tv_b + N);
    if (!c->d_testvec) HIPCHK(c, hipMalloc((void **)&c->d_testvec, sizeof(uint32_t) * 2 * N));
    HIPCHK(c, hipMemcpyAsync(c->d_testvec, c->testvec.data(), sizeof(uint32_t) * 2 * N, hipMemcpyHostToDevice,
                             c->stream));
    if (!c->d_bk) {
        c->bk_bytes = bk_rows(c->P) * 2048 * sizeof(double);
        c->ksk_bytes = ksk_dev_bytes(c->P);
        hipError_t e = hipMalloc((void **)&c->d_bk, c->bk_bytes);
        if (e != hipSuccess) return fail(c, TFHE_ERR_OOM, "hipMalloc(bk)");
        e = hipMalloc((void **)&c->d_ksk, c->ksk_bytes);
        if (e != hipSuccess) return fail(c, TFHE_ERR_OOM, "hipMalloc(ksk)");
    }
    return TFHE_OK;
}

// What a blind-rotation launch hands back.
enum RunKind : int {
    RUN_BOOTSTRAP = 0,     // sample extract + key switch: TLWELv0 (vanilla.zig:38-52)
    RUN_TRLWE = 1,         // the accumulator: TRLWELv1 (trgsw.zig:290-333)
    RUN_NO_KEYSWITCH = 2,  // sampleExtractIndex2, n+1 words (vanilla.zig:58-69)
};

// The gemm key switch's buffers for a batch of B where it is the form to run
// (ks_use_gemm): the MFMA-layout KSK, rebuilt on the stream after a key change,
// and the partial sums.  G stays empty for the other forms (launch_key_switch
// ignores it).
int ks_gemm_args(tfhe_gpu_ctx *c, size_t B, KsGemm &G) {
    G = KsGemm();
    if (!ks_use_gemm(c->opts, c->K.iks_t, c->K.basebit, B, nullptr)) return TFHE_OK;
    if (!c->d_ksk_gemm) {
        hipError_t e = hipMalloc((void **)&c->d_ksk_gemm, ks_gemm_bytes(c->K, 1024, c->K.iks_t, c->K.basebit));
        if (e != hipSuccess) return fail(c, TFHE_ERR_OOM, "hipMalloc(ksk gemm layout)");
    }
    if (!c->ksk_gemm_ok) {
        HIPCHK(c, launch_ksk_to_gemm(c->K, c->d_ksk, c->d_ksk_gemm, 1024, c->K.iks_t, c->K.basebit, c->stream));
        c->ksk_gemm_ok = true;
    }
    int rc = ensure(c, c->s_kspart, ks_gemm_part_bytes(c->K, B, 1024, c->K.basebit));
    if (rc) return rc;
    G.kg = c->d_ksk_gemm;
    G.part = (uint32_t *)c->s_kspart.p;
    return TFHE_OK;
}

// Near-tie flags (KParams::tie_flags) for B items.  The flags are all zero between
// launches, so only a new buffer is zeroed (on the context stream).
int ensure_tie_flags(tfhe_gpu_ctx *c, size_t B) {
    if (c->s_ties.bytes >= B) return TFHE_OK;
    int rc = ensure(c, c->s_ties, B);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(c->s_ties.p, 0, c->s_ties.bytes, c->stream));
    return TFHE_OK;
}

// Blind rotation (+ key switch for RUN_BOOTSTRAP) over device buffers, async.
int run_bootstrap_dev(tfhe_gpu_ctx *c, const uint8_t *ops, const uint32_t *a, const uint32_t *b,
                      const uint32_t *testvec_dev, uint32_t *out, size_t B, int kind,
                      const uint32_t *idx = nullptr) {
    const bool key_switch = kind == RUN_BOOTSTRAP;
    const int out_mode = kind == RUN_BOOTSTRAP ? BR_OUT_LV1 : kind == RUN_TRLWE ? BR_OUT_TRLWE : BR_OUT_LV0_EXTRACT2;
    if (!c->has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    if (B == 0) return TFHE_OK;
    int rc = ensure(c, c->s_lv1, B * 1025 * sizeof(uint32_t));
    if (!rc) rc = ensure_tie_flags(c, B);
    if (rc) return rc;
    KParams K = c->K;
    K.tie_flags = (uint8_t *)c->s_ties.p;
    uint32_t *lv1 = key_switch ? (uint32_t *)c->s_lv1.p : out;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (c->profiling) {
        while (c->events.size() < c->ev_used + 3) {
            hipEvent_t e;
            HIPCHK(c, hipEventCreate(&e));
            c->events.push_back(e);
        }
        for (int i = 0; i < 3; i++) ev[i] = c->events[c->ev_used + i];
        c->ev_used += 3;
        HIPCHK(c, hipEventRecord(ev[0], c->stream));
    }
    const BrBatch batch{ops, a, b, idx, testvec_dev ? testvec_dev : c->d_testvec, c->d_bk, lv1, out_mode, B};
    HIPCHK(c, launch_blind_rotate(K, tables(c), batch, c->stream, c->opts, &c->last_br));
    c->bootstraps += B;
    if (ev[1]) HIPCHK(c, hipEventRecord(ev[1], c->stream));
    c->last_ks = "";
    if (key_switch) {
        KsGemm G;
        if ((rc = ks_gemm_args(c, B, G))) return rc;
        HIPCHK(c, launch_key_switch(c->K, lv1, c->d_ksk, out, B, c->stream, c->opts, &c->last_ks, &G));
    }
    if (ev[2]) HIPCHK(c, hipEventRecord(ev[2], c->stream));
    return TFHE_OK;
}

bool staged(const tfhe_gpu_ctx *c) { return c->host_staging == TFHE_STAGING_PINNED; }

// Pinned host buffer of at least `bytes` (grown by doubling; nothing may be in flight from it).
int ensure_stage(tfhe_gpu_ctx *c, char *&p, size_t &have, size_t bytes) {
    if (have >= bytes) return TFHE_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    have = 0;
    const size_t want = std::max(bytes, (size_t)1 << 20);
    HIPCHK(c, hipHostMalloc((void **)&p, want, hipHostMallocDefault));
    have = want;
    return TFHE_OK;
}

// Host -> device into `buf`.  Pageable: one hipMemcpyAsync from the caller's buffer.  Staged
// (TFHE_OPT_HOST_STAGING): a host memcpy into this context's pinned arena, then the DMA from
// there, so concurrent shards' copies do not go through the runtime's pageable staging
// (for hosts where those serialise across host threads; on the MI355X box they do not and
// pageable copies are faster).  The arena is reused from
// offset 0 after every synchronisation of the stream (d2h_sync); when it is full the stream
// is synchronised first, so no copy in flight ever reads overwritten bytes.
int h2d(tfhe_gpu_ctx *c, DevBuf &buf, const void *src, size_t bytes) {
    int rc = ensure(c, buf, bytes);
    if (rc) return rc;
    if (!staged(c) || !bytes) {
        HIPCHK(c, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, c->stream));
        return TFHE_OK;
    }
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (c->stage_used + need > c->stage_in_bytes) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->stage_used = 0;
        if (need > c->stage_in_bytes) {  // grow (doubling) only when one copy does not fit the empty arena
            rc = ensure_stage(c, c->stage_in, c->stage_in_bytes, std::max(need, 2 * c->stage_in_bytes));
            if (rc) return rc;
        }
    }
    char *p = c->stage_in + c->stage_used;
    std::memcpy(p, src, bytes);
    HIPCHK(c, hipMemcpyAsync(buf.p, p, bytes, hipMemcpyHostToDevice, c->stream));
    c->stage_used += need;
    return TFHE_OK;
}

// Synchronise the context stream and fail the call if a kernel on it set the
// device error word (a slot-counter wait of the blind rotation gave up: its
// words are not the reference's).  The word is copied into pinned host memory
// on the stream, so the one synchronisation covers both; a reported error is
// cleared, and the context stays usable.
// Queue the copy of the device error word (and the recompute counter) into
// pinned host memory on the context stream.
static int queue_err_copy(tfhe_gpu_ctx *c) {
    HIPCHK(c, hipMemcpyAsync(c->h_err, c->d_err, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    return TFHE_OK;
}

// After a synchronisation that covered queue_err_copy: fail the call if a
// kernel set the error word (clearing it; the context stays usable).
static int check_err_word(tfhe_gpu_ctx *c) {
    c->near_tie_items = c->h_err[1];
    const uint32_t e = *c->h_err;
    if (!e) return TFHE_OK;
    *c->h_err = 0;
    HIPCHK(c, hipMemsetAsync(c->d_err, 0, sizeof(uint32_t), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::string what;
    if (e & DEV_ERR_GATE_WAIT) what += "slot-counter protocol failure: a gate wave's wait for a BK slot timed out";
    if (e & DEV_ERR_LOADER_WAIT)
        what += std::string(what.empty() ? "slot-counter protocol failure:" : " and") +
                " a loader wave's wait for a free BK slot timed out";
    if (e & DEV_ERR_LDS_LAYOUT) what += std::string(what.empty() ? "" : "; ") + "LDS array not at address 0, nothing computed";
    return fail(c, TFHE_ERR_DEVICE,
                "blind rotation: " + what + " (device error word 0x" +
                    [&] { char b[16]; std::snprintf(b, sizeof b, "%x", e); return std::string(b); }() +
                    "); the outputs of the work since the last synchronisation are invalid");
}

int sync_check(tfhe_gpu_ctx *c) {
    int rc = queue_err_copy(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return check_err_word(c);
}

// 64-bit fingerprints of this context's device BK and KSK (k_checksum), synchronous.
int key_fingerprint(tfhe_gpu_ctx *c, uint64_t &bk, uint64_t &ksk) {
    auto *d = reinterpret_cast<unsigned long long *>(c->d_err + 2);
    auto *h = reinterpret_cast<volatile unsigned long long *>(c->h_err + 2);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_checksum(c->d_bk, c->bk_bytes, d, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_err + 2, d, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bk = *h;
    HIPCHK(c, launch_checksum(c->d_ksk, c->ksk_bytes, d, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_err + 2, d, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ksk = *h;
    return TFHE_OK;
}

// Key admission of the fused arithmetic.  Its margin guard gives
// the reference's words while the fused and the reference's pre-rounding values
// differ by less than 1/4 — measured, not proven.  Two rules, both on the device
// key at load:
//  - spectrum: the largest BK spectrum component (reference scale) <= 2^39 (round
//    4: concentrated spectra, 2^40.4-2^41.3, reached gaps of 0.19-0.31);
//  - row energy (round 5): every TRGSW row's RMS <= 0.65 x 2^31.  By Parseval the
//    spectrum energy of a row is 2048 x its coefficient energy, so this bounds
//    every row's L1 norm by 1024 x 0.65 x 2^31 and with it every pre-rounding value
//    of the external product, |sum_i digit . row_i| <= 6 x 32 x 1024 x 0.65 x 2^31
//    < 2^48 at the 128-bit set: below 2^48 an f64 ulp is at most 2^-5, half what it
//    is above.  A hill-climbing search for the worst admitted key
//    (tools/admission_search.py, profiles/r05_admission_search.json) finds gaps of
//    at most 0.1875 under the spectrum rule alone (rows of +-(2^31 - 1), RMS 1) and
//    0.125 under both.  Keygen'd rows have RMS 0.545-0.605 (8,400 rows of the
//    seeded 128-bit key); exceeding 0.65 needs a 9.6-sigma row mean of a square.
// A key outside either rule runs the reference's expression trees
// (TFHE_OPT_FUSED_ADMITTED reads the outcome, TFHE_OPT_KEY_ROW_RMS_PPM the RMS).
constexpr double FUSED_BK_SPECTRUM_MAX = 549755813888.0;  // 2^39
constexpr double FUSED_BK_ROW_RMS_MAX = 0.65;             // x 2^31
int key_admission(tfhe_gpu_ctx *c) {
    // refused until measured: a failure below (absmax launch, copy, sync) must not
    // leave the previous key's admission in place
    c->opts.key_fused_ok = 0;
    auto *d = reinterpret_cast<unsigned long long *>(c->d_err + 2);
    auto *h = reinterpret_cast<volatile unsigned long long *>(c->h_err + 2);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_absmax(c->d_bk, c->bk_bytes / sizeof(double), d, c->stream));
    HIPCHK(c, launch_row_energy_max(c->d_bk, (size_t)c->P.n * 2 * c->P.L, d + 1, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_err + 2, d, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const unsigned long long bits = h[0], ebits = h[1];
    double m, e;
    std::memcpy(&m, (const void *)&bits, 8);
    std::memcpy(&e, (const void *)&ebits, 8);
    c->bk_absmax = std::ldexp(m, 10);  // the device BK is the reference's spectrum x 2^-10 (k_bk_permute)
    // row energy: device spectrum energy x 2^20 = reference spectrum energy = 2048 x N x RMS^2
    c->bk_row_rms = std::sqrt(std::ldexp(e, 20) / (2048.0 * c->P.N)) / 2147483648.0;
    c->opts.key_fused_ok =
        c->bk_absmax <= FUSED_BK_SPECTRUM_MAX && c->bk_row_rms <= FUSED_BK_ROW_RMS_MAX ? 1 : 0;  // NaN fails
    return TFHE_OK;
}

// The outputs and the error word in one synchronisation: the word's copy is
// queued first, so it has landed when the outputs have (one round trip fewer
// than copying it after them: DESIGN.md §2.1).
int d2h_sync(tfhe_gpu_ctx *c, void *dst, const void *src, size_t bytes) {
    int rc = queue_err_copy(c);
    if (rc) return rc;
    if (staged(c) && bytes) {  // DMA into the pinned arena, one synchronisation, then a host memcpy
        rc = ensure_stage(c, c->stage_out, c->stage_out_bytes, bytes);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(c->stage_out, src, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->stage_used = 0;  // every staged H2D of the call has landed
        std::memcpy(dst, c->stage_out, bytes);
        return check_err_word(c);
    }
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    // a pageable destination makes the copy synchronous: the stream is idle by
    // now and hipStreamQuery says so at once, where hipStreamSynchronize on an
    // idle stream still took ~19 us (profiles/r03_host_path_trace.txt)
    const hipError_t q = hipStreamQuery(c->stream);
    if (q == hipErrorNotReady) HIPCHK(c, hipStreamSynchronize(c->stream));
    else HIPCHK(c, q);
    return check_err_word(c);
}

int broadcast_key(tfhe_gpu_ctx *c);    // multi-device key broadcast (end of file)
bool is_multi(const tfhe_gpu_ctx *c);  // a context over more than one device (end of file)
void destroy_shards(tfhe_gpu_ctx *c);  // sub-contexts and RCCL communicators (end of file)

// FFT constant tables (fft.zig:92-106 twists, :590-616 recurrence) from the
// chosen cos/sin source (host_math.hpp), uploaded to the context's device.
int build_tables(tfhe_gpu_ctx *c, int source) {
    std::vector<double> tre, tim, fre, fim, ire, iim;
    host::twist_table(c->P.N, tre, tim, source);
    host::stage_twiddles(c->P.N, false, fre, fim, source);
    host::stage_twiddles(c->P.N, true, ire, iim, source);
    // the inverse kernels use conj(forward): that must equal the inverse
    // recurrence bit for bit (both sources have an odd sin and an even cos)
    for (size_t i = 0; i < fre.size(); i++)
        if (std::memcmp(&fre[i], &ire[i], 8) != 0 || -fim[i] != iim[i])
            return fail(c, TFHE_ERR_INVALID, "inverse twiddle table is not the conjugate of the forward one");
    std::vector<C2> tw2(tre.size()), st2(fre.size());
    for (size_t i = 0; i < tre.size(); i++) tw2[i] = C2{tre[i], tim[i]};
    for (size_t i = 0; i < fre.size(); i++) st2[i] = C2{fre[i], fim[i]};
    // passA's bf_m1 (tfhe_kernels.hip) relies on W4[1].im == W8[2].im == -1.0 exactly
    if (st2[2].y != -1.0 || st2[5].y != -1.0)
        return fail(c, TFHE_ERR_INVALID, "twiddle table: W4[1] / W8[2] imaginary part is not exactly -1");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_twist) HIPCHK(c, hipMalloc((void **)&c->d_twist, sizeof(C2) * tw2.size()));
    if (!c->d_tw) HIPCHK(c, hipMalloc((void **)&c->d_tw, sizeof(C2) * st2.size()));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // no launch may still read the old tables
    HIPCHK(c, hipMemcpy(c->d_twist, tw2.data(), sizeof(C2) * tw2.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_tw, st2.data(), sizeof(C2) * st2.size(), hipMemcpyHostToDevice));
    c->twa[0] = st2[2];
    c->twa[1] = st2[4];
    c->twa[2] = st2[5];
    c->twa[3] = st2[6];
    c->twiddle_source = source;
    return TFHE_OK;
}

}  // namespace

extern "C" {

int tfhe_gpu_abi_version(void) { return TFHE_GPU_ABI_VERSION; }

static const char *AB_REFUSAL =
    "tfhe_gpu_create: this library is an A/B build (tfhe_gpu_build_kind), not the product; set "
    "TFHE_ALLOW_AB_BUILD=1 to use it for A/B runs";
static bool ab_build_refused() {  // knock-out / timing / losing-form builds need the opt-in
    if (tfhe_gpu_build_kind() == TFHE_BUILD_PRODUCT) return false;
    const char *allow = std::getenv("TFHE_ALLOW_AB_BUILD");
    return !allow || std::strcmp(allow, "1") != 0;
}

int tfhe_gpu_build_kind(void) {
#ifdef TFHE_AB_BUILD
    return TFHE_BUILD_AB;
#else
    return kernels_ab_build() || ab_forms_linked() ? TFHE_BUILD_AB : TFHE_BUILD_PRODUCT;
#endif
}

int tfhe_gpu_create_on_device(const tfhe_params *params, int device, tfhe_gpu_ctx **out) {
    if (!out) return TFHE_ERR_INVALID;
    *out = nullptr;
    std::string why;
    if (!params_ok(params, why)) return create_fail(TFHE_ERR_INVALID, "tfhe_gpu_create: " + why);
    if (ab_build_refused()) return create_fail(TFHE_ERR_INVALID, AB_REFUSAL);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return create_fail(TFHE_ERR_HIP, "device " + std::to_string(device) + " does not exist (" +
                                             std::to_string(ndev) + " HIP device(s) visible)");
    auto *c = new tfhe_gpu_ctx();
    c->P = *params;
    c->device = device;
    c->K = KParams{(int)params->n, (int)params->N, (int)params->L, (int)params->bgbit, (int)params->basebit,
                   (int)params->iks_t, 0, ks_stride_for((int)params->n), nullptr, 0u, nullptr, 0};
    int rc = TFHE_OK;
    do {
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) { rc = hip_fail(c, e, "hipSetDevice"); break; }
        e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
        if (e != hipSuccess) { rc = hip_fail(c, e, "hipStreamCreate"); break; }
        c->stream = c->own_stream;
        e = hipMalloc((void **)&c->d_err, 64);
        if (e == hipSuccess) e = hipMemset(c->d_err, 0, 64);
        if (e == hipSuccess) e = hipHostMalloc((void **)&c->h_err, 64, hipHostMallocDefault);
        if (e != hipSuccess) { rc = hip_fail(c, e, "device error word"); break; }
        std::memset(c->h_err, 0, 64);
        c->K.err = c->d_err;
        rc = build_tables(c, TFHE_TWIDDLES_GLIBC);
    } while (0);
    if (rc != TFHE_OK) {
        const std::string msg = "tfhe_gpu_create: " + c->err;
        tfhe_gpu_destroy(c);
        return create_fail(rc, msg);
    }
    *out = c;
    return TFHE_OK;
}

void tfhe_gpu_destroy(tfhe_gpu_ctx *c) {
    if (!c) return;
    destroy_shards(c);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);  // NULL is a valid stream here (the device's null stream)
    for (void *p : {(void *)c->d_err, (void *)c->d_twist, (void *)c->d_tw, (void *)c->d_testvec, (void *)c->d_bk, (void *)c->d_ksk,
                    c->s_a.p, c->s_b.p, c->s_out.p, c->s_lv1.p, c->s_ops.p, c->s_tv.p, c->s_tmp.p, c->s_ties.p,
                    c->s_wires.p, c->s_cidx.p, c->s_cops.p, c->s_kspart.p, (void *)c->d_ksk_gemm})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
    if (c->h_err) (void)hipHostFree(c->h_err);
    c->workers.reset();
    for (hipStream_t &p : c->pipe)
        if (p) (void)hipStreamDestroy(p);
    if (c->pipe_ev) (void)hipEventDestroy(c->pipe_ev);
    if (c->pin_in) (void)hipHostFree(c->pin_in);
    if (c->pin_out) (void)hipHostFree(c->pin_out);
    if (c->stage_in) (void)hipHostFree(c->stage_in);
    if (c->stage_out) (void)hipHostFree(c->stage_out);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->stream_ev) (void)hipEventDestroy(c->stream_ev);
    delete c;
}

const char *tfhe_gpu_last_error(const tfhe_gpu_ctx *c) {
    if (c) return c->err.c_str();
    return g_create_error.empty() ? "null context" : g_create_error.c_str();
}

int tfhe_gpu_key_fingerprint(tfhe_gpu_ctx *c, uint64_t *bk, uint64_t *ksk) {
    if (!c || !bk || !ksk) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (!c->has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    uint64_t b = 0, k = 0;
    const int rc = key_fingerprint(c, b, k);
    if (rc) return rc;
    *bk = b;
    *ksk = k;
    return TFHE_OK;
}

int tfhe_gpu_sync(tfhe_gpu_ctx *c) {
    if (!c) return TFHE_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    return sync_check(c);
}

// The context queues its own work on its stream too (the MFMA-layout KSK build,
// the near-tie flag and error-word clears): the new stream waits for everything
// queued on the old one, so a _dev call on the new stream never overtakes it.
static int switch_stream(tfhe_gpu_ctx *c, hipStream_t ns) {
    if (ns == c->stream) return TFHE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->stream_ev) HIPCHK(c, hipEventCreateWithFlags(&c->stream_ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->stream_ev, c->stream));
    HIPCHK(c, hipStreamWaitEvent(ns, c->stream_ev, 0));
    c->stream = ns;
    return TFHE_OK;
}

// ABI 7: NULL is the device's null stream (torch's default stream has handle 0),
// no longer "back to the context's own stream", which is tfhe_gpu_reset_stream.
// Up to ABI 6 a caller passing torch's default stream got the context's own
// non-blocking stream, unordered with torch's work.
int tfhe_gpu_set_stream(tfhe_gpu_ctx *c, void *s) {
    if (!c) return TFHE_ERR_INVALID;
    return switch_stream(c, (hipStream_t)s);
}

int tfhe_gpu_reset_stream(tfhe_gpu_ctx *c) {
    if (!c) return TFHE_ERR_INVALID;
    return switch_stream(c, c->own_stream);
}

int tfhe_gpu_load_cloud_key(tfhe_gpu_ctx *c, uint32_t offset, const uint32_t *tv_a, const uint32_t *tv_b,
                            const double *bsk, size_t bsk_len, const uint32_t *ksk, size_t ksk_len) {
    if (!c || !tv_a || !tv_b || !bsk || !ksk) return fail(c, TFHE_ERR_INVALID, "null argument");
    const size_t rows = bk_rows(c->P);
    if (bsk_len != rows * 2 * c->P.N) return fail(c, TFHE_ERR_INVALID, "bsk_len != n*2L*2*N");
    if (ksk_len != ksk_words(c->P)) return fail(c, TFHE_ERR_INVALID, "ksk_len != N*t*2^basebit*(n+1)");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = set_key_common(c, offset, tv_a, tv_b);
    if (rc) return rc;
    rc = h2d(c, c->s_tmp, bsk, bsk_len * sizeof(double));
    if (rc) return rc;
    HIPCHK(c, launch_bk_permute(c->K, (const double *)c->s_tmp.p, c->d_bk, rows, c->stream));
    rc = upload_ksk(c, ksk);
    if (rc) return rc;
    HIPCHK(c, launch_ksk_zero_k0(c->K, c->d_ksk, c->stream));  // reference leaves k=0 rows undefined
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->has_key = true;
    c->key_from_keygen = false;
    return broadcast_key(c);
}

int tfhe_gpu_key_blob_bytes(const tfhe_gpu_ctx *c, size_t *bsk_bytes, size_t *ksk_bytes) {
    if (!c || !bsk_bytes || !ksk_bytes) return TFHE_ERR_INVALID;
    *bsk_bytes = bk_rows(c->P) * 2048 * sizeof(double);
    *ksk_bytes = ksk_dev_bytes(c->P);  // device layout (padded rows), not the reference's
    return TFHE_OK;
}

int tfhe_gpu_export_key_device(tfhe_gpu_ctx *c, void *bsk_dev, void *ksk_dev, uint32_t *offset,
                               uint32_t *testvec) {
    if (!c || !bsk_dev || !ksk_dev) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (!c->has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(bsk_dev, c->d_bk, c->bk_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(ksk_dev, c->d_ksk, c->ksk_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (offset) *offset = c->offset;
    if (testvec) std::memcpy(testvec, c->testvec.data(), sizeof(uint32_t) * 2 * c->P.N);
    return TFHE_OK;
}

int tfhe_gpu_import_key_device(tfhe_gpu_ctx *c, const void *bsk_dev, const void *ksk_dev, uint32_t offset,
                               const uint32_t *testvec) {
    if (!c || !bsk_dev || !ksk_dev || !testvec) return fail(c, TFHE_ERR_INVALID, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = set_key_common(c, offset, testvec, testvec + c->P.N);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_bk, bsk_dev, c->bk_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_ksk, ksk_dev, c->ksk_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, launch_ksk_zero_k0(c->K, c->d_ksk, c->stream));
    c->ksk_gemm_ok = false;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->has_key = true;
    c->key_from_keygen = false;
    return broadcast_key(c);
}

// Device key -> reference host layout: BK un-permuted (and un-scaled) by
// k_bk_permute's inverse, KSK rows un-padded.
int tfhe_gpu_export_cloud_key(tfhe_gpu_ctx *c, uint32_t *offset, uint32_t *tv_a, uint32_t *tv_b, double *bsk,
                              uint32_t *ksk) {
    if (!c) return TFHE_ERR_INVALID;
    if (!c->has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = c->P.N;
    if (offset) *offset = c->offset;
    if (tv_a) std::memcpy(tv_a, c->testvec.data(), N * sizeof(uint32_t));
    if (tv_b) std::memcpy(tv_b, c->testvec.data() + N, N * sizeof(uint32_t));
    if (bsk) {
        const size_t rows = bk_rows(c->P), bytes = rows * 2 * N * sizeof(double);
        int rc = ensure(c, c->s_tmp, bytes);
        if (rc) return rc;
        HIPCHK(c, launch_bk_unpermute(c->K, c->d_bk, (double *)c->s_tmp.p, rows, c->stream));
        HIPCHK(c, hipMemcpyAsync(bsk, c->s_tmp.p, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    if (ksk) {
        const size_t w = c->P.n + 1;
        HIPCHK(c, hipMemcpy2DAsync(ksk, w * 4, c->d_ksk, (size_t)c->K.ks_stride * 4, w * 4, ksk_rows(c->P),
                                   hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TFHE_OK;
}

int tfhe_gpu_save_cloud_key(tfhe_gpu_ctx *c, const char *path) {
    if (!c || !path) return fail(c, TFHE_ERR_INVALID, "null argument");
    const size_t N = c->P.N, bl = bk_rows(c->P) * 2 * N, kl = ksk_words(c->P);
    std::vector<uint32_t> ta(N), tb(N), ksk(kl);
    std::vector<double> bsk(bl);
    uint32_t off = 0;
    int rc = tfhe_gpu_export_cloud_key(c, &off, ta.data(), tb.data(), bsk.data(), ksk.data());
    if (rc) return rc;
    rc = tfhe_cloud_key_write(path, &c->P, off, ta.data(), tb.data(), bsk.data(), bl, ksk.data(), kl);
    if (rc) return fail(c, rc, std::string("cannot write key file ") + path);
    return TFHE_OK;
}

int tfhe_gpu_load_cloud_key_file(tfhe_gpu_ctx *c, const char *path) {
    if (!c || !path) return fail(c, TFHE_ERR_INVALID, "null argument");
    const size_t N = c->P.N, bl = bk_rows(c->P) * 2 * N, kl = ksk_words(c->P);
    std::vector<uint32_t> ta(N), tb(N), ksk(kl);
    std::vector<double> bsk(bl);
    uint32_t off = 0;
    int rc = tfhe_cloud_key_read(path, &c->P, &off, ta.data(), tb.data(), bsk.data(), bl, ksk.data(), kl);
    if (rc == TFHE_ERR_IO) return fail(c, rc, std::string("cannot read key file ") + path);
    if (rc) return fail(c, rc, std::string(path) + ": not a key file of this parameter set, or checksum mismatch");
    return tfhe_gpu_load_cloud_key(c, off, ta.data(), tb.data(), bsk.data(), bl, ksk.data(), kl);
}

// SecretKey.new + CloudKey.new, seeded.  Host: every RNG draw in reference
// order; device: the FFT-based poly_mul of each TRLWE encryption
// (trlwe.zig:56-61) and the TRGSWLv1FFT forward transforms (trgsw.zig:81-91).
int tfhe_gpu_keygen(tfhe_gpu_ctx *c, uint64_t secret_seed, uint64_t cloud_seed, uint32_t *key_lv0,
                    uint32_t *key_lv1, double *bsk_out, uint32_t *ksk_out) {
    if (!c || !key_lv0 || !key_lv1) return fail(c, TFHE_ERR_INVALID, "null argument");
    const tfhe_params &p = c->P;
    const uint32_t N = p.N, n = p.n, L = p.L, T = p.iks_t, base = 1u << p.basebit;
    HIPCHK(c, hipSetDevice(c->device));
    tfhe_secret_key_new(&p, secret_seed, key_lv0, key_lv1);
    host::Rng master(cloud_seed);
    // genKeySwitchingKey (key.zig:148-172): k = 0 rows are zeroed
    std::vector<uint32_t> ksk(ksk_words(p), 0u);
    for (uint32_t i = 0; i < N; i++)
        for (uint32_t j = 0; j < T; j++)
            for (uint32_t k = 1; k < base; k++) {
                size_t idx = (size_t)base * T * i + (size_t)base * j + k;
                uint32_t shift = (j + 1) * p.basebit;
                double pv = ((double)k * (double)key_lv1[i]) / (double)(1u << shift);
                tlwe_encrypt(n, pv, p.alpha_ksk, key_lv0, master.next(), ksk.data() + idx * (n + 1));
            }
    // genBootstrappingKey (key.zig:175-212): per i, TRGSW encryptTorus of
    // key_lv0[i]: 2L TRLWE encryptions of zero (trlwe.zig:30-64), gadget on
    // a[0] of row l / b[0] of row L+l.
    const size_t R = bk_rows(p);  // n*2L TRLWE rows
    std::vector<uint32_t> rows(R * 2 * N);
    std::vector<uint32_t> noise(R * N);
    for (size_t row = 0; row < R; row++) {
        host::Rng r(master.next());
        uint32_t *a = rows.data() + row * 2 * N;
        for (uint32_t x = 0; x < N; x++) a[x] = r.u32();
        host::NormalDist nd(0.0, p.alpha_bsk);
        for (uint32_t x = 0; x < N; x++) noise[row * N + x] = host::gaussian_torus(0u, nd, r);
    }
    int rc = h2d(c, c->s_b, key_lv1, N * sizeof(uint32_t));
    if (rc) return rc;
    rc = ensure(c, c->s_out, R * N * sizeof(uint32_t));
    if (rc) return rc;
    // a*s for all rows: a_i lives at stride 2N inside `rows`
    std::vector<uint32_t> a_only(R * N);
    for (size_t row = 0; row < R; row++)
        std::memcpy(a_only.data() + row * N, rows.data() + row * 2 * N, N * sizeof(uint32_t));
    rc = h2d(c, c->s_a, a_only.data(), a_only.size() * sizeof(uint32_t));
    if (rc) return rc;
    HIPCHK(c, launch_poly_mul(tables(c), (const uint32_t *)c->s_a.p, (const uint32_t *)c->s_b.p, 0,
                              (uint32_t *)c->s_out.p, R, c->stream));
    std::vector<uint32_t> as(R * N);
    rc = d2h_sync(c, as.data(), c->s_out.p, as.size() * sizeof(uint32_t));
    if (rc) return rc;
    for (size_t row = 0; row < R; row++) {
        uint32_t *b = rows.data() + row * 2 * N + N;
        for (uint32_t x = 0; x < N; x++) b[x] = noise[row * N + x] + as[row * N + x];
    }
    for (uint32_t i = 0; i < n; i++) {
        uint32_t mu = key_lv0[i];
        for (uint32_t l = 0; l < L; l++) {
            uint32_t h = host::f64_to_torus(std::ldexp(1.0, -(int)((l + 1) * p.bgbit)));
            rows[((size_t)i * 2 * L + l) * 2 * N] += mu * h;              // trlwe[l].a[0]
            rows[((size_t)i * 2 * L + L + l) * 2 * N + N] += mu * h;      // trlwe[L+l].b[0]
        }
    }
    // TRGSWLv1FFT.new: ifft of every a and b polynomial -> reference BK layout
    rc = h2d(c, c->s_a, rows.data(), rows.size() * sizeof(uint32_t));
    if (rc) return rc;
    rc = ensure(c, c->s_tmp, R * 2 * N * sizeof(double));
    if (rc) return rc;
    HIPCHK(c, launch_fft_forward(tables(c), (const uint32_t *)c->s_a.p, (double *)c->s_tmp.p, R * 2, c->stream));
    std::vector<uint32_t> tv(2 * N);
    for (uint32_t x = 0; x < N; x++) {  // genTestvec (key.zig:134-145)
        tv[x] = 0;
        tv[N + x] = host::f64_to_torus(0.125);
    }
    rc = set_key_common(c, decomposition_offset(p), tv.data(), tv.data() + N);
    if (rc) return rc;
    HIPCHK(c, launch_bk_permute(c->K, (const double *)c->s_tmp.p, c->d_bk, R, c->stream));
    rc = upload_ksk(c, ksk.data());
    if (rc) return rc;
    if (bsk_out)
        HIPCHK(c, hipMemcpyAsync(bsk_out, c->s_tmp.p, R * 2 * N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (ksk_out) std::memcpy(ksk_out, ksk.data(), ksk.size() * sizeof(uint32_t));
    c->has_key = true;
    c->key_from_keygen = true;
    return broadcast_key(c);
}

}  // extern "C"

namespace {

int ensure_pinned(tfhe_gpu_ctx *c, char *&p, size_t &have, size_t bytes) {
    if (have >= bytes) return TFHE_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    have = 0;
    HIPCHK(c, hipHostMalloc((void **)&p, bytes, hipHostMallocDefault));
    have = bytes;
    return TFHE_OK;
}

// Host-buffer bootstrap of B >= one whole-form round, pipelined (DESIGN.md
// §2.1): the batch is cut into chunks of #CUs items (a quarter round: #CUs/4
// workgroups of the whole form).  Worker s owns stream s and chunks s, s+S, ...;
// per chunk it copies the caller's inputs into pinned staging, then enqueues
// H2D -> blind rotation (whole form; the guard's recompute) -> key switch ->
// D2H on its stream, so chunk k+1's copies run while chunks <= k compute and
// the S streams' kernels share the CUs.  Each worker then waits for its stream
// and copies its chunks' outputs to the caller.  ops / b / tv_dev may be NULL.
int pipelined_bootstrap(tfhe_gpu_ctx *c, const uint8_t *ops, const uint32_t *a, const uint32_t *b,
                        const uint32_t *tv_dev, uint32_t *out, size_t B) {
    const size_t w = tlwe0_words(c), wb = w * 4, chunk = device_cus();
    const size_t nch = (B + chunk - 1) / chunk;
    const int S = (int)std::min<size_t>(PIPE_STREAMS, nch);
    // staging layout per item: op byte region, then a, then b (all chunks contiguous)
    const size_t ops_bytes = ops ? (B + 15) / 16 * 16 : 0, a_bytes = B * wb, b_bytes = b ? B * wb : 0;
    int rc = ensure_pinned(c, c->pin_in, c->pin_in_bytes, ops_bytes + a_bytes + b_bytes);
    if (!rc) rc = ensure_pinned(c, c->pin_out, c->pin_out_bytes, B * wb);
    if (!rc && ops) rc = ensure(c, c->s_ops, B);
    if (!rc) rc = ensure(c, c->s_a, B * wb);
    if (!rc && b) rc = ensure(c, c->s_b, B * wb);
    if (!rc) rc = ensure(c, c->s_out, B * wb);
    if (!rc) rc = ensure(c, c->s_lv1, B * 1025 * sizeof(uint32_t));
    if (!rc) rc = ensure_tie_flags(c, B);
    if (rc) return rc;
    if (!c->pipe_ev) HIPCHK(c, hipEventCreateWithFlags(&c->pipe_ev, hipEventDisableTiming));
    for (hipStream_t &p : c->pipe)
        if (!p) HIPCHK(c, hipStreamCreateWithFlags(&p, hipStreamNonBlocking));
    if (!c->workers) c->workers.reset(new WorkerPool(PIPE_STREAMS));
    // the GEMM key switch per chunk (the default form where it applies): its MFMA-layout
    // key is built once on the context stream, and each stream gets its own
    // partial-sum buffer, so every chunk runs the same key-switch form as the
    // unpipelined path (last_kernels names it)
    KsGemm G;
    rc = ks_gemm_args(c, chunk, G);
    if (rc) return rc;
    std::vector<KsGemm> Gs(S, G);
    if (G.kg) {
        const size_t pb = ks_gemm_part_bytes(c->K, chunk, 1024, c->K.basebit);
        rc = ensure(c, c->s_kspart, pb * S);
        if (rc) return rc;
        for (int s = 0; s < S; s++) Gs[s].part = (uint32_t *)((char *)c->s_kspart.p + (size_t)s * pb);
    }
    // everything enqueued on the context stream (key loads, the flags' memset) first
    HIPCHK(c, hipEventRecord(c->pipe_ev, c->stream));
    LaunchOpts o = c->opts;
    if (!o.br_form) o.br_form = 1;  // whole form for every chunk (a chunk is a quarter round)
    char *pin_ops = c->pin_in, *pin_a = c->pin_in + ops_bytes, *pin_b = pin_a + a_bytes;
    uint8_t *d_ops = (uint8_t *)c->s_ops.p;
    uint32_t *d_a = (uint32_t *)c->s_a.p, *d_b = (uint32_t *)c->s_b.p, *d_out = (uint32_t *)c->s_out.p;
    uint32_t *d_lv1 = (uint32_t *)c->s_lv1.p;
    std::vector<hipError_t> err(S, hipSuccess);
    std::vector<const char *> where(S, "");
    c->workers->run(S, [&](int s) {
        hipStream_t st = c->pipe[s];
        auto chk = [&](hipError_t e, const char *what) {
            if (e != hipSuccess && err[s] == hipSuccess) {
                err[s] = e;
                where[s] = what;
            }
            return e == hipSuccess;
        };
        if (!chk(hipSetDevice(c->device), "hipSetDevice") || !chk(hipStreamWaitEvent(st, c->pipe_ev, 0), "hipStreamWaitEvent"))
            return;
        for (size_t k = (size_t)s; k < nch; k += (size_t)S) {
            const size_t k0 = k * chunk, n = std::min(B, k0 + chunk) - k0;
            if (ops) std::memcpy(pin_ops + k0, ops + k0, n);
            std::memcpy(pin_a + k0 * wb, a + k0 * w, n * wb);
            if (b) std::memcpy(pin_b + k0 * wb, b + k0 * w, n * wb);
            if (ops && !chk(hipMemcpyAsync(d_ops + k0, pin_ops + k0, n, hipMemcpyHostToDevice, st), "H2D ops")) return;
            if (!chk(hipMemcpyAsync(d_a + k0 * w, pin_a + k0 * wb, n * wb, hipMemcpyHostToDevice, st), "H2D a")) return;
            if (b && !chk(hipMemcpyAsync(d_b + k0 * w, pin_b + k0 * wb, n * wb, hipMemcpyHostToDevice, st), "H2D b"))
                return;
            KParams K = c->K;
            K.tie_flags = (uint8_t *)c->s_ties.p + k0;
            const BrBatch batch{ops ? d_ops + k0 : nullptr, d_a + k0 * w, b ? d_b + k0 * w : nullptr, nullptr,
                                tv_dev ? tv_dev : c->d_testvec, c->d_bk, d_lv1 + k0 * 1025, BR_OUT_LV1, n};
            if (!chk(launch_blind_rotate(K, tables(c), batch, st, o, s == 0 && k == 0 ? &c->last_br : nullptr),
                     "blind rotation") ||
                !chk(launch_key_switch(c->K, d_lv1 + k0 * 1025, c->d_ksk, d_out + k0 * w, n, st, c->opts,
                                       s == 0 && k == 0 ? &c->last_ks : nullptr, &Gs[s]),
                     "key switch") ||
                !chk(hipMemcpyAsync(c->pin_out + k0 * wb, d_out + k0 * w, n * wb, hipMemcpyDeviceToHost, st), "D2H"))
                return;
        }
        if (!chk(hipStreamSynchronize(st), "hipStreamSynchronize")) return;
        for (size_t k = (size_t)s; k < nch; k += (size_t)S) {
            const size_t k0 = k * chunk, n = std::min(B, k0 + chunk) - k0;
            std::memcpy(out + k0 * w, c->pin_out + k0 * wb, n * wb);
        }
    });
    for (int s = 0; s < S; s++)
        if (err[s] != hipSuccess) {
            for (int t = 0; t < S; t++) (void)hipStreamSynchronize(c->pipe[t]);
            return hip_fail(c, err[s], where[s]);
        }
    c->bootstraps += B;
    return sync_check(c);  // the device error word (and the recompute counter) after all streams
}

// The pipeline serves host-buffer bootstraps of at least one whole-form round
// (4 x #CUs items) unless TFHE_OPT_HOST_PIPELINE = 0 or device timing is on
// (its events bracket single launches on the context stream).
bool use_pipeline(const tfhe_gpu_ctx *c, size_t B) {
    return c->pipeline && !c->profiling && B >= 4 * device_cus();
}

}  // namespace

extern "C" {

// One host-buffer batch through the blind rotation: what the bootstrap, gate,
// blind-rotate and LUT entry points differ in.
struct HostBatch {
    const uint8_t *ops;       // NULL unless gate
    const uint32_t *a, *b;    // b NULL unless gate
    const uint32_t *testvec;  // host test vector, or NULL: the key's
    uint32_t *out;
    int kind;                 // RunKind
    bool gate;                // a gate batch: ops and b are arguments too
    bool needs_key;           // refuse a context without a cloud key before any upload
    bool may_pipeline;        // large batches may take pipelined_bootstrap
};
static bool host_batch_args_ok(const HostBatch &d, size_t B) {
    return B == 0 || (d.a && d.out && (!d.gate || (d.ops && d.b)));
}
static size_t host_batch_out_words(const tfhe_gpu_ctx *c, const HostBatch &d) {
    return d.kind == RUN_TRLWE ? 2 * (size_t)c->P.N : tlwe0_words(c);
}

static int host_batch_one(tfhe_gpu_ctx *c, const HostBatch &d, size_t B) {
    if (!c || !host_batch_args_ok(d, B)) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (B == 0) return TFHE_OK;
    if (d.gate)
        for (size_t i = 0; i < B; i++)
            if (d.ops[i] > TFHE_GATE_ORYN && d.ops[i] != TFHE_GATE_COPY) return fail(c, TFHE_ERR_INVALID, "bad gate op");
    HIPCHK(c, hipSetDevice(c->device));
    if (d.needs_key && !c->has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t in_bytes = B * tlwe0_words(c) * 4, out_bytes = B * host_batch_out_words(c, d) * 4;
    const uint32_t *tv = nullptr;
    int rc = TFHE_OK;
    if (d.testvec) {
        if ((rc = h2d(c, c->s_tv, d.testvec, 2 * c->P.N * 4))) return rc;
        tv = (const uint32_t *)c->s_tv.p;
    }
    if (d.may_pipeline && use_pipeline(c, B)) return pipelined_bootstrap(c, d.ops, d.a, d.b, tv, d.out, B);
    if (d.gate) rc = h2d(c, c->s_ops, d.ops, B);
    if (!rc) rc = h2d(c, c->s_a, d.a, in_bytes);
    if (!rc && d.gate) rc = h2d(c, c->s_b, d.b, in_bytes);
    if (!rc) rc = ensure(c, c->s_out, out_bytes);
    if (!rc)
        rc = run_bootstrap_dev(c, d.gate ? (const uint8_t *)c->s_ops.p : nullptr, (const uint32_t *)c->s_a.p,
                               d.gate ? (const uint32_t *)c->s_b.p : nullptr, tv, (uint32_t *)c->s_out.p, B, d.kind);
    if (!rc) rc = d2h_sync(c, d.out, c->s_out.p, out_bytes);
    return rc;
}

// ---- Proxy re-encryption ------------------------------------
}  // extern "C"

struct tfhe_gpu_reenc_key {
    int device = 0;
    uint32_t basebit = 0, t = 0;
    uint32_t *d_key = nullptr;  // padded rows like the KSK (K.ks_stride words) + zero tail
    uint32_t *d_key_gemm = nullptr;  // the gemm key switch's layout of d_key (basebit 2, t 7..9), or NULL
    std::vector<tfhe_gpu_reenc_key *> peers;  // multi-device context: the copy on shard k is peers[k - 1]
};

extern "C" {

static int reenc_key_load_one(tfhe_gpu_ctx *c, const uint32_t *key_encryptions, size_t len, uint32_t basebit,
                            uint32_t t, tfhe_gpu_reenc_key **out) {
    if (!c || !key_encryptions || !out) return fail(c, TFHE_ERR_INVALID, "null argument");
    const size_t n = c->P.n, rows = n * t * ((size_t)1 << basebit);
    if (basebit < 1 || basebit > 8 || t < 1 || basebit * t >= 31 || !reencrypt_supported((int)t, (int)basebit))
        return fail(c, TFHE_ERR_INVALID, "unsupported re-encryption base/levels");
    if (len != rows * (n + 1)) return fail(c, TFHE_ERR_INVALID, "len != n*t*2^basebit*(n+1)");
    HIPCHK(c, hipSetDevice(c->device));
    auto *k = new tfhe_gpu_reenc_key;
    k->device = c->device;
    k->basebit = basebit;
    k->t = t;
    const size_t stride = c->K.ks_stride, bytes = (rows * stride + KS_TAIL_WORDS) * sizeof(uint32_t);
    hipError_t e = hipMalloc((void **)&k->d_key, bytes);
    if (e != hipSuccess) {
        delete k;
        return fail(c, TFHE_ERR_OOM, "hipMalloc(reencryption key)");
    }
    e = hipMemsetAsync(k->d_key, 0, bytes, c->stream);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(k->d_key, stride * 4, key_encryptions, (n + 1) * 4, (n + 1) * 4, rows,
                             hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_key_zero_k0(c->K, k->d_key, (int)n, (int)t, (int)basebit, c->stream);
    if (e == hipSuccess && ks_gemm_supported((int)t, (int)basebit)) {  // §4.4b layout for the gemm form
        e = hipMalloc((void **)&k->d_key_gemm, ks_gemm_bytes(c->K, (int)n, (int)t, (int)basebit));
        if (e == hipSuccess) e = launch_ksk_to_gemm(c->K, k->d_key, k->d_key_gemm, (int)n, (int)t, (int)basebit, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipFree(k->d_key);
        if (k->d_key_gemm) (void)hipFree(k->d_key_gemm);
        delete k;
        return hip_fail(c, e, "upload reencryption key");
    }
    *out = k;
    return TFHE_OK;
}

void tfhe_gpu_reenc_key_destroy(tfhe_gpu_reenc_key *k) {
    if (!k) return;
    for (tfhe_gpu_reenc_key *p : k->peers) tfhe_gpu_reenc_key_destroy(p);
    (void)hipSetDevice(k->device);
    (void)hipFree(k->d_key);
    if (k->d_key_gemm) (void)hipFree(k->d_key_gemm);
    delete k;
}

// dev: in and out are device pointers (tfhe_gpu_reencrypt_batch_dev): the input is copied
// device-to-device into the staging buffer, the kernel writes `out` directly, and the call
// returns without waiting (async on the context stream, like the other _dev entries)
static int reencrypt_batch_one(tfhe_gpu_ctx *c, const tfhe_gpu_reenc_key *k, const uint32_t *in, uint32_t *out,
                               size_t B, bool dev = false) {
    if (!c || !k || (B && (!in || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (k->device != c->device) return fail(c, TFHE_ERR_INVALID, "key belongs to another device");
    if (B == 0) return TFHE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t w = tlwe0_words(c);
    int rc = ensure(c, c->s_a, B * w * 4 + KS_GEMM_INPUT_SLACK);  // the gemm form reads whole blocks of 8
    if (rc) return rc;
    if (dev) {
        HIPCHK(c, hipMemcpyAsync(c->s_a.p, in, B * w * 4, hipMemcpyDeviceToDevice, c->stream));
    } else {
        rc = h2d(c, c->s_a, in, B * w * 4);
        if (!rc) rc = ensure(c, c->s_out, B * w * 4);
        if (rc) return rc;
    }
    KsGemm G;
    if (k->d_key_gemm) {
        rc = ensure(c, c->s_kspart, ks_gemm_part_bytes(c->K, B, (int)c->P.n, (int)k->basebit));
        if (rc) return rc;
        G.kg = k->d_key_gemm;
        G.part = (uint32_t *)c->s_kspart.p;
    }
    HIPCHK(c, launch_reencrypt(c->K, (int)k->t, (int)k->basebit, (const uint32_t *)c->s_a.p, k->d_key,
                               dev ? out : (uint32_t *)c->s_out.p, B, c->stream, c->opts, &c->last_ks, &G));
    return dev ? TFHE_OK : d2h_sync(c, out, c->s_out.p, B * w * 4);
}

// Circuits (planner: tfhe_cpu.cpp).  The one context-free function here: it needs the launchers' cost model.
int tfhe_circuit_schedule(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                          const uint32_t *in_b, uint32_t cus, int pack, uint32_t *levels, uint32_t *depth) {
    if ((n_gates && (!ops || !in_a || !in_b || !levels)) || cus == 0) return TFHE_ERR_INVALID;
    if (n_inputs + n_gates > 0xFFFFFFFFull) return TFHE_ERR_INVALID;
    std::vector<uint32_t> level;
    std::vector<std::vector<uint32_t>> bs, nots;
    uint32_t max_level = 0;
    if (schedule_levels(n_inputs, n_gates, ops, in_a, in_b, pack != 0, cus, level_cost, level, max_level, bs, nots))
        return TFHE_ERR_INVALID;
    for (size_t g = 0; g < n_gates; g++) levels[g] = level[n_inputs + g];
    if (depth) *depth = max_level;
    return TFHE_OK;
}

}  // extern "C"

namespace {

// Device side of a plan on one context: wire table with the inputs, the gather
// indices and op codes, uploaded on its stream.
int upload_plan(tfhe_gpu_ctx *c, const CircuitPlan &pl, size_t W, size_t n_inputs, const uint32_t *inputs,
                size_t n_outputs, bool inputs_on_device = false) {
    const size_t w1 = tlwe0_words(c);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure(c, c->s_wires, std::max<size_t>(W, 1) * w1 * 4);
    if (!rc) rc = ensure(c, c->s_cidx, std::max<size_t>(pl.idx.size(), 1) * 4);
    if (!rc) rc = ensure(c, c->s_cops, std::max<size_t>(pl.cops.size(), 1));
    if (!rc) rc = ensure(c, c->s_out, std::max<size_t>(n_outputs, 1) * w1 * 4);
    if (rc) return rc;
    if (n_inputs)
        HIPCHK(c, hipMemcpyAsync(c->s_wires.p, inputs, n_inputs * w1 * 4,
                                 inputs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    // the plan vectors are pageable: hipMemcpyAsync stages them before it returns, so the caller
    // may drop `pl` while the copies are still in flight (the _dev circuit call does not sync)
    if (!pl.idx.empty())
        HIPCHK(c, hipMemcpyAsync(c->s_cidx.p, pl.idx.data(), pl.idx.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!pl.cops.empty())
        HIPCHK(c, hipMemcpyAsync(c->s_cops.p, pl.cops.data(), pl.cops.size(), hipMemcpyHostToDevice, c->stream));
    return TFHE_OK;
}

}  // namespace

extern "C" {

// dev: inputs and outputs are device pointers (tfhe_gpu_circuit_eval_dev): the inputs are copied
// device-to-device into the wire table, the outputs gathered straight into `outputs`, and the call
// returns without waiting (async on the context stream, like the other _dev entries)
static int circuit_eval_one(tfhe_gpu_ctx *c, size_t n_inputs, const uint32_t *inputs, size_t n_gates,
                          const uint8_t *ops, const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs,
                          const uint32_t *out_wires, uint32_t *outputs, uint32_t *levels_out, bool dev = false) {
    if (!c || (n_inputs && !inputs) || (n_gates && (!ops || !in_a || !in_b)) || (n_outputs && (!out_wires || !outputs)))
        return fail(c, TFHE_ERR_INVALID, "null argument");
    if (!c->has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t W = n_inputs + n_gates, w1 = tlwe0_words(c);
    HIPCHK(c, hipSetDevice(c->device));
    CircuitPlan pl;
    if (const char *why = plan_circuit(n_inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires, c->circuit_pack != 0,
                                       device_cus(), level_cost, pl))
        return fail(c, TFHE_ERR_INVALID, why);
    int rc = upload_plan(c, pl, W, n_inputs, inputs, n_outputs, dev);
    if (rc) return rc;
    const auto &bs = pl.bs;
    const auto &nots = pl.nots;
    const uint32_t max_level = pl.max_level;
    uint32_t *wires = (uint32_t *)c->s_wires.p;
    const uint32_t *d_idx = (const uint32_t *)c->s_cidx.p;
    const uint8_t *d_ops = (const uint8_t *)c->s_cops.p;
    size_t ip = 0, op_pos = 0, sp = n_inputs;
    for (uint32_t lv = 0; lv <= max_level; lv++) {
        const size_t nb = bs[lv].size(), nn = nots[lv].size();
        if (nb) {
            rc = run_bootstrap_dev(c, d_ops + op_pos, wires, wires, nullptr, wires + sp * w1, nb, RUN_BOOTSTRAP,
                                   d_idx + ip);
            if (rc) return rc;
            ip += 2 * nb;
            op_pos += nb;
            sp += nb;
        }
        if (nn) {
            HIPCHK(c, launch_tlwe_gather(c->K, wires, d_idx + ip, wires + sp * w1, nn, true, c->stream));
            ip += nn;
            sp += nn;
        }
    }
    if (n_outputs && dev) {
        HIPCHK(c, launch_tlwe_gather(c->K, wires, d_idx + ip, outputs, n_outputs, false, c->stream));
    } else if (n_outputs) {
        HIPCHK(c, launch_tlwe_gather(c->K, wires, d_idx + ip, (uint32_t *)c->s_out.p, n_outputs, false, c->stream));
        rc = d2h_sync(c, outputs, c->s_out.p, n_outputs * w1 * 4);
        if (rc) return rc;
    } else if (dev) {
    } else {
        rc = sync_check(c);
        if (rc) return rc;
    }
    if (levels_out) *levels_out = max_level;
    return TFHE_OK;
}

int tfhe_gpu_gate_batch_dev(tfhe_gpu_ctx *c, const uint8_t *ops_dev, const uint32_t *a_dev, const uint32_t *b_dev,
                            uint32_t *out_dev, size_t B) {
    if (!c || (B && (!ops_dev || !a_dev || !b_dev || !out_dev))) return fail(c, TFHE_ERR_INVALID, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    return run_bootstrap_dev(c, ops_dev, a_dev, b_dev, nullptr, out_dev, B, RUN_BOOTSTRAP);
}

int tfhe_gpu_bootstrap_batch_dev(tfhe_gpu_ctx *c, const uint32_t *in_dev, uint32_t *out_dev, size_t B) {
    if (!c || (B && (!in_dev || !out_dev))) return fail(c, TFHE_ERR_INVALID, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    return run_bootstrap_dev(c, nullptr, in_dev, nullptr, nullptr, out_dev, B, RUN_BOOTSTRAP);
}

int tfhe_gpu_bootstrap_lut_batch_dev(tfhe_gpu_ctx *c, const uint32_t *in_dev, const uint32_t *testvec_dev,
                                     uint32_t *out_dev, size_t B) {
    if (!c || !testvec_dev || (B && (!in_dev || !out_dev))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    return run_bootstrap_dev(c, nullptr, in_dev, nullptr, testvec_dev, out_dev, B, RUN_BOOTSTRAP);
}

int tfhe_gpu_profile_begin(tfhe_gpu_ctx *c) {
    if (!c) return TFHE_ERR_INVALID;
    c->profiling = true;
    c->ev_used = 0;
    return TFHE_OK;
}

int tfhe_gpu_profile_end(tfhe_gpu_ctx *c, double *br_ms, double *ks_ms, int *launches) {
    if (!c) return TFHE_ERR_INVALID;
    c->profiling = false;
    const int rc = sync_check(c);
    if (rc) {
        c->ev_used = 0;
        return rc;
    }
    double br = 0.0, ks = 0.0;
    for (size_t i = 0; i + 3 <= c->ev_used; i += 3) {
        float a = 0.f, b = 0.f;
        HIPCHK(c, hipEventElapsedTime(&a, c->events[i], c->events[i + 1]));
        HIPCHK(c, hipEventElapsedTime(&b, c->events[i + 1], c->events[i + 2]));
        br += a;
        ks += b;
    }
    if (br_ms) *br_ms = br;
    if (ks_ms) *ks_ms = ks;
    if (launches) *launches = (int)(c->ev_used / 3);
    c->ev_used = 0;
    return TFHE_OK;
}

int tfhe_gpu_fft_forward_batch(tfhe_gpu_ctx *c, const uint32_t *in, double *out, size_t B) {
    if (!c || (B && (!in || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (B == 0) return TFHE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = h2d(c, c->s_a, in, B * 1024 * 4);
    if (!rc) rc = ensure(c, c->s_tmp, B * 1024 * 8);
    if (rc) return rc;
    HIPCHK(c, launch_fft_forward(tables(c), (const uint32_t *)c->s_a.p, (double *)c->s_tmp.p, B, c->stream));
    return d2h_sync(c, out, c->s_tmp.p, B * 1024 * 8);
}

int tfhe_gpu_fft_inverse_batch(tfhe_gpu_ctx *c, const double *in, uint32_t *out, size_t B) {
    if (!c || (B && (!in || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (B == 0) return TFHE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = h2d(c, c->s_tmp, in, B * 1024 * 8);
    if (!rc) rc = ensure(c, c->s_out, B * 1024 * 4);
    if (rc) return rc;
    HIPCHK(c, launch_fft_inverse(tables(c), (const double *)c->s_tmp.p, (uint32_t *)c->s_out.p, B, c->stream));
    return d2h_sync(c, out, c->s_out.p, B * 1024 * 4);
}

int tfhe_gpu_poly_mul_batch(tfhe_gpu_ctx *c, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t B) {
    if (!c || (B && (!a || !b || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (B == 0) return TFHE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = h2d(c, c->s_a, a, B * 1024 * 4);
    if (!rc) rc = h2d(c, c->s_b, b, B * 1024 * 4);
    if (!rc) rc = ensure(c, c->s_out, B * 1024 * 4);
    if (rc) return rc;
    HIPCHK(c, launch_poly_mul(tables(c), (const uint32_t *)c->s_a.p, (const uint32_t *)c->s_b.p, 1024,
                              (uint32_t *)c->s_out.p, B, c->stream));
    return d2h_sync(c, out, c->s_out.p, B * 1024 * 4);
}

int tfhe_gpu_external_product_batch(tfhe_gpu_ctx *c, const double *trgsw_fft, uint32_t bk_index,
                                    const uint32_t *in, uint32_t *out, size_t B) {
    if (!c || (B && (!in || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (B == 0) return TFHE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t row_d = (size_t)2 * c->P.L * 2048;  // doubles per TRGSW
    const double *row = nullptr;
    int rc = TFHE_OK;
    if (trgsw_fft) {
        rc = h2d(c, c->s_tmp, trgsw_fft, row_d * 8);
        if (!rc) rc = ensure(c, c->s_tv, row_d * 8);
        if (rc) return rc;
        HIPCHK(c, launch_bk_permute(c->K, (const double *)c->s_tmp.p, (double *)c->s_tv.p, 2 * c->P.L, c->stream));
        row = (const double *)c->s_tv.p;
        if (c->K.offset == 0) c->K.offset = decomposition_offset(c->P);  // no key loaded yet: the parameter set's
    } else {
        if (!c->has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
        if (bk_index >= c->P.n) return fail(c, TFHE_ERR_INVALID, "bk_index >= n");
        row = c->d_bk + (size_t)bk_index * row_d;
    }
    rc = h2d(c, c->s_a, in, B * 2048 * 4);
    if (!rc) rc = ensure(c, c->s_out, B * 2048 * 4);
    if (rc) return rc;
    HIPCHK(c, launch_external_product(c->K, tables(c), row, (const uint32_t *)c->s_a.p, (uint32_t *)c->s_out.p, B,
                                      c->stream));
    return d2h_sync(c, out, c->s_out.p, B * 2048 * 4);
}

static int key_switch_batch_one(tfhe_gpu_ctx *c, const uint32_t *in_lv1, uint32_t *out_lv0, size_t B) {
    if (!c || (B && (!in_lv1 || !out_lv0))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (!c->has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    if (B == 0) return TFHE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t w = tlwe0_words(c);
    int rc = h2d(c, c->s_lv1, in_lv1, B * 1025 * 4);
    if (!rc) rc = ensure(c, c->s_out, B * w * 4);
    if (rc) return rc;
    KsGemm G;
    if ((rc = ks_gemm_args(c, B, G))) return rc;
    HIPCHK(c, launch_key_switch(c->K, (const uint32_t *)c->s_lv1.p, c->d_ksk, (uint32_t *)c->s_out.p, B, c->stream,
                                c->opts, &c->last_ks, &G));
    return d2h_sync(c, out_lv0, c->s_out.p, B * w * 4);
}

}  // extern "C"

// ---- Options ------------------------------------------------------------------
namespace {

// Range check of one option value, before anything is applied to any device.
bool option_ok(const tfhe_gpu_ctx *c, int key, int64_t v, std::string &why) {
    bool ok = false;
    switch (key) {
    case TFHE_OPT_BR_FORM:
        // 2 split, 4 pair: removed in round 4; 6 duo, 7 split-transform latency
        // form, 8 the whole form without loader assist, 30 the latency form with row
        // counters: A/B libraries only (tools/ab/); 5 octo: L = 1 only
        ok = v == 0 || v == 1 || v == 3 || (v == 5 && c->P.L == 1) ||
             ((v == 6 || v == 7 || v == 8 || v == 30) && ab_forms_linked());
        if (!ok && v == 5) why = "TFHE_OPT_BR_FORM 5 (octo form) exists at L = 1 only";
        if (!ok && v >= 6 && v <= 8) why = "TFHE_OPT_BR_FORM " + std::to_string(v) + ": an A/B-only form, not in the product library (tools/ab/)";
        break;
    case TFHE_OPT_KS_FORM: ok = v >= 0 && v <= 3; break;
    case TFHE_OPT_BR_LOADER:  // the whole form always runs loader waves with slot counters (the
    case TFHE_OPT_BR_SYNC:    // gate-wave DMA and per-pair barrier variants were removed in round 5)
        ok = v == 1;
        if (!ok) why = "option " + std::to_string(key) + ": only 1 (the variant with value 0 was removed in round 5)";
        break;
    case TFHE_OPT_KS_NARROW:
    case TFHE_OPT_CIRCUIT_PACK: ok = v == 0 || v == 1; break;
    case TFHE_OPT_KS_ITEM_GROUPS: ok = v == 0 || v == 1 || v == 2 || v == 4 || v == 8; break;
    case TFHE_OPT_KS_SEL_ITEMS: ok = v == 8 || v == 16 || v == 32; break;
    case TFHE_OPT_ARITH: ok = v == TFHE_ARITH_AUTO || v == TFHE_ARITH_REFERENCE || v == TFHE_ARITH_FUSED_FORCED; break;
    case TFHE_OPT_BR_SPIN_CAP: ok = v >= 0 && v <= 0xFFFFFFFFll; break;
    case TFHE_OPT_HOST_PIPELINE: ok = v == 0 || v == 1; break;
    case TFHE_OPT_CIRCUIT_SPLIT: ok = v >= 0 && v <= 2; break;
    case TFHE_OPT_HOST_STAGING: ok = v == TFHE_STAGING_PAGEABLE || v == TFHE_STAGING_PINNED; break;
    case TFHE_OPT_TWIDDLES:
        ok = v == TFHE_TWIDDLES_GLIBC || v == TFHE_TWIDDLES_FDLIBM;
        // tfhe_gpu_keygen transformed the resident BK with the current tables:
        // other tables would no longer match it (a loaded reference key is data
        // and may be paired with either table)
        if (ok && c->key_from_keygen && v != c->twiddle_source) {
            why = "TFHE_OPT_TWIDDLES: the resident key was generated (tfhe_gpu_keygen) with the current FFT tables; "
                  "set the twiddle source before keygen";
            return false;
        }
        break;
    default: why = "unknown option key " + std::to_string(key); return false;
    }
    if (!ok && why.empty()) why = "bad value " + std::to_string(v) + " for option " + std::to_string(key);
    return ok;
}

// Apply a checked option to one device's context.
int apply_option(tfhe_gpu_ctx *c, int key, int64_t v) {
    LaunchOpts &o = c->opts;
    switch (key) {
    case TFHE_OPT_BR_FORM: o.br_form = (int)v; break;
    case TFHE_OPT_BR_LOADER: break;
    case TFHE_OPT_KS_FORM: o.ks_form = (int)v; break;
    case TFHE_OPT_KS_NARROW: o.ks_narrow = (int)v; break;
    case TFHE_OPT_KS_ITEM_GROUPS: o.ks_groups = (int)v; break;
    case TFHE_OPT_KS_SEL_ITEMS: o.ks_sel_items = (int)v; break;
    case TFHE_OPT_CIRCUIT_PACK: c->circuit_pack = v; break;
    case TFHE_OPT_TWIDDLES: return v == c->twiddle_source ? TFHE_OK : build_tables(c, (int)v);
    case TFHE_OPT_BR_SYNC: break;
    case TFHE_OPT_ARITH: o.arith_strict = v == TFHE_ARITH_REFERENCE ? 1 : v == TFHE_ARITH_FUSED_FORCED ? 2 : 0; break;
    case TFHE_OPT_BR_SPIN_CAP: c->K.spin_cap = (uint32_t)v; break;
    case TFHE_OPT_HOST_PIPELINE: c->pipeline = v; break;
    case TFHE_OPT_CIRCUIT_SPLIT: c->circuit_split = v; break;
    case TFHE_OPT_HOST_STAGING:
        if (c->stage_used) HIPCHK(c, hipStreamSynchronize(c->stream));  // nothing in flight from the arena
        c->stage_used = 0;
        c->host_staging = v;
        break;
    default: return TFHE_ERR_INVALID;
    }
    return TFHE_OK;
}

}  // namespace

extern "C" {

// Validated once, then applied to every device (shards 1.., then the root).
int tfhe_gpu_set_option(tfhe_gpu_ctx *c, int key, int64_t v) {
    if (!c) return TFHE_ERR_INVALID;
    std::string why;
    if (!option_ok(c, key, v, why)) return fail(c, TFHE_ERR_INVALID, why);
    for (size_t d = 1; d < c->shards.size(); d++) {
        const int rc = apply_option(c->shards[d], key, v);
        if (rc) return fail(c, rc, c->shards[d]->err);
    }
    return apply_option(c, key, v);
}

int tfhe_gpu_get_option(const tfhe_gpu_ctx *c, int key, int64_t *v) {
    if (!c || !v) return TFHE_ERR_INVALID;
    const LaunchOpts &o = c->opts;
    switch (key) {
    case TFHE_OPT_BR_FORM: *v = o.br_form; break;
    case TFHE_OPT_BR_LOADER: *v = 1; break;
    case TFHE_OPT_KS_FORM: *v = o.ks_form; break;
    case TFHE_OPT_KS_NARROW: *v = o.ks_narrow; break;
    case TFHE_OPT_KS_ITEM_GROUPS: *v = o.ks_groups; break;
    case TFHE_OPT_KS_SEL_ITEMS: *v = o.ks_sel_items; break;
    case TFHE_OPT_CIRCUIT_PACK: *v = c->circuit_pack; break;
    case TFHE_OPT_TWIDDLES: *v = c->twiddle_source; break;
    case TFHE_OPT_ARITH: *v = o.arith_strict == 1 ? TFHE_ARITH_REFERENCE : o.arith_strict == 2 ? TFHE_ARITH_FUSED_FORCED : TFHE_ARITH_AUTO; break;
    case TFHE_OPT_FUSED_ADMITTED: *v = o.key_fused_ok; break;
    case TFHE_OPT_LEVEL_ISSUE_US: *v = c->level_issue_us; break;
    case TFHE_OPT_KEY_ROW_RMS_PPM: *v = (int64_t)std::llround(c->bk_row_rms * 1e6); break;
    case TFHE_OPT_BR_SYNC: *v = 1; break;
    case TFHE_OPT_BR_SPIN_CAP: *v = c->K.spin_cap; break;
    case TFHE_OPT_HOST_PIPELINE: *v = c->pipeline; break;
    case TFHE_OPT_CIRCUIT_SPLIT: *v = c->circuit_split; break;
    case TFHE_OPT_HOST_STAGING: *v = c->host_staging; break;
    default: return TFHE_ERR_INVALID;
    }
    return TFHE_OK;
}

const char *tfhe_gpu_last_kernels(tfhe_gpu_ctx *c) {
    if (!c) return "";
    c->last_kernels = c->last_br;
    if (c->last_ks && c->last_ks[0]) c->last_kernels += std::string(" + ") + c->last_ks;
    return c->last_kernels.c_str();
}

}  // extern "C"

// ---- Multi-device context ----------------------------------
namespace {

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

const RcclApi *rccl_api(std::string &why) {
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

bool is_multi(const tfhe_gpu_ctx *c) { return c && c->shards.size() > 1; }

void destroy_shards(tfhe_gpu_ctx *c) {
    if (!c->comms.empty()) {
        std::string why;
        if (const RcclApi *r = rccl_api(why))
            for (ncclComm_t m : c->comms)
                if (m) r->comm_destroy(m);
        c->comms.clear();
    }
    for (size_t d = 1; d < c->shards.size(); d++) tfhe_gpu_destroy(c->shards[d]);
    c->shards.clear();
}

// The key just loaded on shard 0 -> every other shard: one ncclBroadcast of
// the device BK and KSK (RCCL over xGMI), or a device-to-device copy when a
// device appears twice.  The test vector / offset are host state (8 KB).
int broadcast_key(tfhe_gpu_ctx *c) {
    int rc0 = key_admission(c);  // every key load ends here: admit the fused arithmetic or not
    if (rc0) {  // an unmeasured key is not a loaded key
        c->has_key = false;
        return rc0;
    }
    if (c->shards.empty()) return TFHE_OK;
    const size_t D = c->shards.size();
    for (size_t d = 1; d < D; d++) {
        tfhe_gpu_ctx *s = c->shards[d];
        s->has_key = false;
        HIPCHK(c, hipSetDevice(s->device));
        int rc = set_key_common(s, c->offset, c->testvec.data(), c->testvec.data() + c->P.N);
        if (rc) return fail(c, rc, s->err);
        HIPCHK(c, hipStreamSynchronize(s->stream));
    }
    if (c->distinct_devices) {
        std::string why;
        const RcclApi *r = rccl_api(why);
        if (!r) return fail(c, TFHE_ERR_HIP, why);
        if (c->comms.empty()) {
            std::vector<int> devs(D);
            for (size_t d = 0; d < D; d++) devs[d] = c->shards[d]->device;
            c->comms.assign(D, nullptr);
            ncclResult_t e = r->comm_init_all(c->comms.data(), (int)D, devs.data());
            if (e != ncclSuccess) {
                c->comms.clear();
                return fail(c, TFHE_ERR_HIP, std::string("ncclCommInitAll: ") + r->error_string(e));
            }
        }
        ncclResult_t e = r->group_start();
        for (size_t d = 0; d < D && e == ncclSuccess; d++) {
            tfhe_gpu_ctx *s = c->shards[d];
            e = r->broadcast(c->d_bk, s->d_bk, c->bk_bytes, ncclUint8, 0, c->comms[d], s->stream);
            if (e == ncclSuccess) e = r->broadcast(c->d_ksk, s->d_ksk, c->ksk_bytes, ncclUint8, 0, c->comms[d], s->stream);
        }
        ncclResult_t e2 = r->group_end();
        if (e == ncclSuccess) e = e2;
        if (e != ncclSuccess) return fail(c, TFHE_ERR_HIP, std::string("ncclBroadcast: ") + r->error_string(e));
    } else {
        for (size_t d = 1; d < D; d++) {
            tfhe_gpu_ctx *s = c->shards[d];
            HIPCHK(c, hipSetDevice(s->device));
            HIPCHK(c, hipMemcpyPeerAsync(s->d_bk, s->device, c->d_bk, c->device, c->bk_bytes, s->stream));
            HIPCHK(c, hipMemcpyPeerAsync(s->d_ksk, s->device, c->d_ksk, c->device, c->ksk_bytes, s->stream));
        }
    }
    for (size_t d = 1; d < D; d++) {
        tfhe_gpu_ctx *s = c->shards[d];
        HIPCHK(c, hipSetDevice(s->device));
        HIPCHK(c, hipStreamSynchronize(s->stream));
        s->ksk_gemm_ok = false;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // every copy must fingerprint like the root's before a shard may use it
    uint64_t bk0 = 0, ksk0 = 0;
    int rc = key_fingerprint(c, bk0, ksk0);
    if (rc) return rc;
    for (size_t d = 1; d < D; d++) {
        tfhe_gpu_ctx *s = c->shards[d];
        uint64_t bk = 0, ksk = 0;
        rc = key_fingerprint(s, bk, ksk);
        if (rc) return fail(c, rc, s->err);
        if (bk != bk0 || ksk != ksk0)
            return fail(c, TFHE_ERR_HIP, "key broadcast: the copy on device " + std::to_string(s->device) +
                                             " differs from device " + std::to_string(c->device) + "'s");
        s->bk_absmax = c->bk_absmax;  // same bits, same admission
        s->bk_row_rms = c->bk_row_rms;
        s->opts.key_fused_ok = c->opts.key_fused_ok;
        s->has_key = true;
    }
    HIPCHK(c, hipSetDevice(c->device));
    return TFHE_OK;
}

// f(shard, first item, count) on every device's contiguous slice of B items
// (ceil(B/D) each), concurrently: one host thread per device beyond the first.
template <class F>
int run_sharded(tfhe_gpu_ctx *c, size_t B, F f) {
    const size_t D = c->shards.size(), per = (B + D - 1) / D;
    std::vector<int> rc(D, TFHE_OK);
    std::vector<std::thread> th;
    for (size_t d = 1; d < D; d++) {
        const size_t b0 = std::min(B, d * per), n = std::min(B, b0 + per) - b0;
        if (n) th.emplace_back([&, d, b0, n] { rc[d] = f(c->shards[d], b0, n); });
    }
    if (B) rc[0] = f(c, 0, std::min(B, per));
    for (std::thread &t : th) t.join();
    for (size_t d = 1; d < D; d++)
        if (rc[d]) return fail(c, rc[d], "device " + std::to_string(c->shards[d]->device) + ": " + c->shards[d]->err);
    return rc[0];
}

// A shard's part of a per-item host array of `words` words per item (NULL stays NULL).
template <class T>
T *shard_items(T *p, size_t first, size_t words) {
    return p ? p + first * words : nullptr;
}

// Level split or components (TFHE_OPT_CIRCUIT_SPLIT: 0 auto, 1 components, 2
// levels).  Auto: levels when the component placement leaves the busiest device
// more than 10 % above an even share of at least one whole-form round per device
// (e.g. one big connected circuit); components otherwise (independent gates,
// MUXes and adders place evenly, and nothing crosses devices).
bool split_by_levels(const tfhe_gpu_ctx *c, size_t n_gates, const uint8_t *ops, const std::vector<uint32_t> &dev) {
    if (c->circuit_split != 0) return c->circuit_split == 2;
    const size_t D = c->shards.size();
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
// and the primary inputs.  Per level, device d bootstraps its contiguous slice
// of the level's gates into its table; each slice is then copied to every other
// device (peer copies over xGMI, ordered by an event on the producer's stream:
// an all-gather), and every device applies the level's NOTs itself.  Outputs
// come from the first device's table.
int circuit_eval_levels(tfhe_gpu_ctx *c, size_t n_inputs, const uint32_t *inputs, size_t n_gates, const uint8_t *ops,
                        const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires,
                        uint32_t *outputs, uint32_t *levels_out) {
    const size_t W = n_inputs + n_gates, D = c->shards.size(), w1 = tlwe0_words(c);
    CircuitPlan pl;
    if (const char *why = plan_circuit(n_inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires, c->circuit_pack != 0,
                                       device_cus() * D, level_cost, pl))
        return fail(c, TFHE_ERR_INVALID, why);
    std::vector<hipEvent_t> ev(D, nullptr);
    auto cleanup = [&] {
        for (size_t d = 0; d < D; d++)
            if (ev[d]) {
                (void)hipSetDevice(c->shards[d]->device);
                (void)hipEventDestroy(ev[d]);
            }
        (void)hipSetDevice(c->device);
    };
    int rc = TFHE_OK;
    for (size_t d = 0; d < D && !rc; d++) {
        tfhe_gpu_ctx *s = c->shards[d];
        rc = upload_plan(s, pl, W, n_inputs, inputs, n_outputs);
        if (!rc && hipEventCreateWithFlags(&ev[d], hipEventDisableTiming) != hipSuccess) rc = fail(s, TFHE_ERR_HIP, "hipEventCreate");
        if (rc) rc = fail(c, rc, "device " + std::to_string(s->device) + ": " + s->err);
    }
    size_t ip = 0, op_pos = 0, sp = n_inputs;
    // the per-level issue (launches, peer copies, event waits) runs on this one
    // host thread for all devices; it is asynchronous, so it costs wall time only
    // where it outruns the devices' per-level work (measured: DESIGN.md §7)
    const auto t_issue = std::chrono::steady_clock::now();
    for (uint32_t lv = 0; lv <= pl.max_level && !rc; lv++) {
        const size_t nb = pl.bs[lv].size(), nn = pl.nots[lv].size(), per = (nb + D - 1) / D;
        if (nb) {
            for (size_t d = 0; d < D && !rc; d++) {  // each device its slice
                tfhe_gpu_ctx *s = c->shards[d];
                const size_t lo = std::min(nb, d * per), n = std::min(nb, lo + per) - lo;
                if (!n) continue;
                if (hipSetDevice(s->device) != hipSuccess) { rc = fail(c, TFHE_ERR_HIP, "hipSetDevice"); break; }
                uint32_t *wires = (uint32_t *)s->s_wires.p;
                rc = run_bootstrap_dev(s, (const uint8_t *)s->s_cops.p + op_pos + lo, wires, wires, nullptr,
                                       wires + (sp + lo) * w1, n, RUN_BOOTSTRAP, (const uint32_t *)s->s_cidx.p + ip + 2 * lo);
                if (!rc && hipEventRecord(ev[d], s->stream) != hipSuccess) rc = fail(s, TFHE_ERR_HIP, "hipEventRecord");
                if (rc) rc = fail(c, rc, "device " + std::to_string(s->device) + ": " + s->err);
            }
            for (size_t e = 0; e < D && !rc; e++) {  // all-gather of the level's outputs
                tfhe_gpu_ctx *t = c->shards[e];
                if (hipSetDevice(t->device) != hipSuccess) { rc = fail(c, TFHE_ERR_HIP, "hipSetDevice"); break; }
                for (size_t d = 0; d < D && !rc; d++) {
                    const size_t lo = std::min(nb, d * per), n = std::min(nb, lo + per) - lo;
                    if (d == e || !n) continue;
                    tfhe_gpu_ctx *s = c->shards[d];
                    const size_t off = (sp + lo) * w1;
                    if (hipStreamWaitEvent(t->stream, ev[d], 0) != hipSuccess ||
                        hipMemcpyPeerAsync((uint32_t *)t->s_wires.p + off, t->device, (const uint32_t *)s->s_wires.p + off,
                                           s->device, n * w1 * 4, t->stream) != hipSuccess)
                        rc = fail(c, TFHE_ERR_HIP, "level all-gather to device " + std::to_string(t->device));
                }
            }
            ip += 2 * nb;
            op_pos += nb;
            sp += nb;
        }
        if (nn && !rc) {
            for (size_t d = 0; d < D && !rc; d++) {  // every device negates the level's NOT inputs itself
                tfhe_gpu_ctx *s = c->shards[d];
                uint32_t *wires = (uint32_t *)s->s_wires.p;
                if (hipSetDevice(s->device) != hipSuccess ||
                    launch_tlwe_gather(s->K, wires, (const uint32_t *)s->s_cidx.p + ip, wires + sp * w1, nn, true,
                                       s->stream) != hipSuccess)
                    rc = fail(c, TFHE_ERR_HIP, "NOT gather on device " + std::to_string(s->device));
            }
            ip += nn;
            sp += nn;
        }
    }
    c->level_issue_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_issue).count();
    for (size_t d = 1; d < D && !rc; d++) {  // every device's work done, its error word clean
        tfhe_gpu_ctx *s = c->shards[d];
        if (hipSetDevice(s->device) != hipSuccess) { rc = fail(c, TFHE_ERR_HIP, "hipSetDevice"); break; }
        rc = sync_check(s);
        if (rc) rc = fail(c, rc, "device " + std::to_string(s->device) + ": " + s->err);
    }
    if (!rc && hipSetDevice(c->device) != hipSuccess) rc = fail(c, TFHE_ERR_HIP, "hipSetDevice");
    if (!rc && n_outputs) {
        if (launch_tlwe_gather(c->K, (const uint32_t *)c->s_wires.p, (const uint32_t *)c->s_cidx.p + ip,
                               (uint32_t *)c->s_out.p, n_outputs, false, c->stream) != hipSuccess)
            rc = fail(c, TFHE_ERR_HIP, "output gather");
        else
            rc = d2h_sync(c, outputs, c->s_out.p, n_outputs * w1 * 4);
    } else if (!rc) {
        rc = sync_check(c);
    }
    cleanup();
    if (!rc && levels_out) *levels_out = pl.max_level;
    return rc;
}

// circuit_eval over the devices.  Primary inputs are read-only, so every
// device gets its own copy of the ones it reads; only gate-to-gate wires tie
// gates together.  The connected components of the gate DAG under those wires
// go whole to one device each, largest first onto the least-loaded device
// (bootstrapped gates), so each device evaluates an independent sub-circuit
// with its own level schedule and no wire crosses devices.  Config 4's
// independent AND/OR/XOR gates and MUXes over shared inputs (gates.zig:124-129)
// spread evenly; one adder (examples/add_two_numbers.zig:24-73) stays whole.
int circuit_eval_multi(tfhe_gpu_ctx *c, size_t n_inputs, const uint32_t *inputs, size_t n_gates, const uint8_t *ops,
                       const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires,
                       uint32_t *outputs, uint32_t *levels_out) {
    const size_t D = c->shards.size(), w1 = tlwe0_words(c);
    // validate the whole graph first (same errors as one device)
    if (const char *why = check_circuit(n_inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires))
        return fail(c, TFHE_ERR_INVALID, why);
    std::vector<uint32_t> dev_of_gate;
    partition_gates(n_inputs, n_gates, ops, in_a, in_b, D, dev_of_gate);
    if (split_by_levels(c, n_gates, ops, dev_of_gate))
        return circuit_eval_levels(c, n_inputs, inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires, outputs, levels_out);
    // per-device sub-circuits; wires renumbered: the device's inputs first, then its gates
    struct Sub {
        std::vector<uint32_t> inputs, in_a, in_b, out_wires, out_index;
        std::vector<uint8_t> ops;
        std::vector<uint32_t> outputs;
        uint32_t levels = 0;
        std::vector<uint32_t> input_id;  // global input -> local id (or none)
    };
    std::vector<Sub> sub(D);
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    auto gate_dev = [&](size_t g) { return dev_of_gate[g]; };
    // an output that is a primary input is copied out by device 0
    auto wire_dev = [&](uint32_t w) { return w < n_inputs ? 0u : gate_dev(w - n_inputs); };
    auto use_input = [&](uint32_t d, uint32_t w) {
        if (w >= n_inputs) return;
        Sub &s = sub[d];
        if (s.input_id.empty()) s.input_id.assign(n_inputs, NONE);
        if (s.input_id[w] == NONE) {
            s.input_id[w] = (uint32_t)s.inputs.size();
            s.inputs.push_back(w);
        }
    };
    for (size_t g = 0; g < n_gates; g++) {
        use_input(gate_dev(g), in_a[g]);
        if (ops[g] <= TFHE_GATE_ORYN) use_input(gate_dev(g), in_b[g]);
    }
    for (size_t o = 0; o < n_outputs; o++) use_input(wire_dev(out_wires[o]), out_wires[o]);
    std::vector<uint32_t> local_gate(n_gates), gate_count(D, 0);
    for (size_t g = 0; g < n_gates; g++) local_gate[g] = gate_count[gate_dev(g)]++;
    auto id = [&](uint32_t d, uint32_t w) {
        return w < n_inputs ? sub[d].input_id[w] : (uint32_t)sub[d].inputs.size() + local_gate[w - n_inputs];
    };
    for (size_t g = 0; g < n_gates; g++) {
        const uint32_t d = gate_dev(g);
        Sub &s = sub[d];
        s.ops.push_back(ops[g]);
        s.in_a.push_back(id(d, in_a[g]));
        s.in_b.push_back(ops[g] <= TFHE_GATE_ORYN ? id(d, in_b[g]) : 0u);
    }
    for (size_t o = 0; o < n_outputs; o++) {
        const uint32_t d = wire_dev(out_wires[o]);
        sub[d].out_wires.push_back(id(d, out_wires[o]));
        sub[d].out_index.push_back((uint32_t)o);
    }
    std::vector<int> rc(D, TFHE_OK);
    auto run = [&](size_t d) {
        Sub &s = sub[d];
        if (s.ops.empty() && s.out_wires.empty()) return;
        std::vector<uint32_t> in(s.inputs.size() * w1);
        for (size_t i = 0; i < s.inputs.size(); i++)
            std::memcpy(in.data() + i * w1, inputs + (size_t)s.inputs[i] * w1, w1 * 4);
        s.outputs.resize(s.out_wires.size() * w1);
        rc[d] = circuit_eval_one(c->shards[d], s.inputs.size(), in.data(), s.ops.size(), s.ops.data(), s.in_a.data(),
                                 s.in_b.data(), s.out_wires.size(), s.out_wires.data(), s.outputs.data(), &s.levels);
    };
    std::vector<std::thread> th;
    for (size_t d = 1; d < D; d++) th.emplace_back(run, d);
    run(0);
    for (std::thread &t : th) t.join();
    uint32_t depth = 0;
    for (size_t d = 0; d < D; d++) {
        if (rc[d]) return fail(c, rc[d], "device " + std::to_string(c->shards[d]->device) + ": " + c->shards[d]->err);
        const Sub &s = sub[d];
        for (size_t k = 0; k < s.out_index.size(); k++)
            std::memcpy(outputs + (size_t)s.out_index[k] * w1, s.outputs.data() + k * w1, w1 * 4);
        depth = std::max(depth, s.levels);
    }
    if (levels_out) *levels_out = depth;
    return TFHE_OK;
}

}  // namespace

extern "C" {

int tfhe_gpu_create_multi(const tfhe_params *params, int num_devices, const int *devices, tfhe_gpu_ctx **out) {
    if (!out || num_devices < 1) return TFHE_ERR_INVALID;
    *out = nullptr;
    std::vector<int> devs(num_devices);
    for (int d = 0; d < num_devices; d++) devs[d] = devices ? devices[d] : d;
    std::string why;
    if (!params_ok(params, why)) return create_fail(TFHE_ERR_INVALID, "tfhe_gpu_create_multi: " + why);
    if (ab_build_refused()) return create_fail(TFHE_ERR_INVALID, AB_REFUSAL);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return create_fail(TFHE_ERR_HIP, "hipGetDeviceCount failed");
    for (int d : devs)
        if (d < 0 || d >= ndev)
            return create_fail(TFHE_ERR_HIP, "device " + std::to_string(d) + " does not exist (" +
                                                 std::to_string(ndev) + " HIP device(s) visible)");
    tfhe_gpu_ctx *root = nullptr;
    int rc = tfhe_gpu_create_on_device(params, devs[0], &root);
    if (rc) return rc;
    root->shards.push_back(root);
    for (int d = 1; d < num_devices; d++) {
        tfhe_gpu_ctx *s = nullptr;
        rc = tfhe_gpu_create_on_device(params, devs[d], &s);
        if (rc) {
            tfhe_gpu_destroy(root);
            return rc;
        }
        root->shards.push_back(s);
    }
    std::vector<int> sorted = devs;
    std::sort(sorted.begin(), sorted.end());
    root->distinct_devices = std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
    if (root->distinct_devices) {
        // every ordered pair: the level split all-gathers between all of them
        for (int a : devs)
            for (int b : devs) {
                if (a == b) continue;
                int can = 0;
                hipError_t e = hipDeviceCanAccessPeer(&can, a, b);
                if (e != hipSuccess || !can) {
                    tfhe_gpu_destroy(root);
                    return create_fail(TFHE_ERR_DEVICE, "device " + std::to_string(a) + " cannot access device " +
                                                            std::to_string(b) + "'s memory (hipDeviceCanAccessPeer" +
                                                            (e != hipSuccess ? std::string(": ") + hipGetErrorString(e) : "") +
                                                            "): the multi-device context needs xGMI peer access");
                }
                e = hipSetDevice(a);
                if (e == hipSuccess) e = hipDeviceEnablePeerAccess(b, 0);
                if (e == hipErrorPeerAccessAlreadyEnabled) {
                    (void)hipGetLastError();  // clear the sticky status of an already-enabled pair
                    e = hipSuccess;
                }
                if (e != hipSuccess) {
                    tfhe_gpu_destroy(root);
                    return create_fail(TFHE_ERR_DEVICE, "hipDeviceEnablePeerAccess(" + std::to_string(a) + " -> " +
                                                            std::to_string(b) + "): " + hipGetErrorString(e));
                }
            }
        (void)hipSetDevice(devs[0]);
    }
    *out = root;
    return TFHE_OK;
}

// SURVEY §8b's entry point: devices 0..num_devices-1 of this node (one device:
// a plain context on device 0; more: the multi-device context above).
int tfhe_gpu_create(const tfhe_params *params, int num_devices, tfhe_gpu_ctx **out) {
    if (!out) return TFHE_ERR_INVALID;
    *out = nullptr;
    std::string why;
    if (num_devices < 1 || !params_ok(params, why))
        return create_fail(TFHE_ERR_INVALID, num_devices < 1 ? "num_devices < 1" : "tfhe_gpu_create: " + why);
    if (ab_build_refused()) return create_fail(TFHE_ERR_INVALID, AB_REFUSAL);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || num_devices > ndev)
        return create_fail(TFHE_ERR_HIP, std::to_string(num_devices) + " device(s) requested, " +
                                             std::to_string(ndev) + " HIP device(s) visible");
    if (num_devices == 1) return tfhe_gpu_create_on_device(params, 0, out);
    return tfhe_gpu_create_multi(params, num_devices, nullptr, out);
}

int tfhe_gpu_num_devices(const tfhe_gpu_ctx *c) { return !c ? 0 : c->shards.empty() ? 1 : (int)c->shards.size(); }

int tfhe_gpu_near_tie_items(const tfhe_gpu_ctx *c, uint64_t *count) {
    if (!c || !count) return TFHE_ERR_INVALID;
    uint64_t n = c->near_tie_items;
    for (size_t d = 1; d < c->shards.size(); d++) n += c->shards[d]->near_tie_items;
    *count = n;
    return TFHE_OK;
}

int tfhe_gpu_device_bootstraps(const tfhe_gpu_ctx *c, uint64_t *counts, int max_devices) {
    if (!c || !counts || max_devices < 1) return TFHE_ERR_INVALID;
    const int D = tfhe_gpu_num_devices(c);
    for (int d = 0; d < D && d < max_devices; d++) counts[d] = c->shards.empty() ? c->bootstraps : c->shards[d]->bootstraps;
    return D;
}

// host_batch_one on the context's one device, or on every shard's slice of the batch.
static int host_batch(tfhe_gpu_ctx *c, const HostBatch &d, size_t B) {
    if (!is_multi(c)) return host_batch_one(c, d, B);
    if (!host_batch_args_ok(d, B)) return fail(c, TFHE_ERR_INVALID, "null argument");
    const size_t w = tlwe0_words(c), wo = host_batch_out_words(c, d);
    return run_sharded(c, B, [&](tfhe_gpu_ctx *s, size_t b0, size_t n) {
        HostBatch p = d;
        p.ops = shard_items(d.ops, b0, 1);
        p.a = shard_items(d.a, b0, w);
        p.b = shard_items(d.b, b0, w);
        p.out = shard_items(d.out, b0, wo);
        return host_batch_one(s, p, n);
    });
}

int tfhe_gpu_bootstrap_batch(tfhe_gpu_ctx *c, const uint32_t *in, uint32_t *out, size_t B) {
    const HostBatch d{nullptr, in, nullptr, nullptr, out, RUN_BOOTSTRAP, /*gate*/ false,
                      /*needs_key*/ true, /*may_pipeline*/ true};
    return host_batch(c, d, B);
}

int tfhe_gpu_bootstrap_without_key_switch_batch(tfhe_gpu_ctx *c, const uint32_t *in, uint32_t *out, size_t B) {
    const HostBatch d{nullptr, in, nullptr, nullptr, out, RUN_NO_KEYSWITCH, /*gate*/ false,
                      /*needs_key*/ false, /*may_pipeline*/ false};
    return host_batch(c, d, B);
}

int tfhe_gpu_gate_batch(tfhe_gpu_ctx *c, const uint8_t *ops, const uint32_t *a, const uint32_t *b, uint32_t *out,
                        size_t B) {
    const HostBatch d{ops, a, b, nullptr, out, RUN_BOOTSTRAP, /*gate*/ true,
                      /*needs_key*/ true, /*may_pipeline*/ true};
    return host_batch(c, d, B);
}

int tfhe_gpu_blind_rotate_batch(tfhe_gpu_ctx *c, const uint32_t *in, const uint32_t *testvec, uint32_t *trlwe_out,
                                size_t B) {
    const HostBatch d{nullptr, in, nullptr, testvec, trlwe_out, RUN_TRLWE, /*gate*/ false,
                      /*needs_key*/ false, /*may_pipeline*/ false};
    return host_batch(c, d, B);
}

int tfhe_gpu_bootstrap_lut_batch(tfhe_gpu_ctx *c, const uint32_t *in, const uint32_t *testvec, uint32_t *out,
                                 size_t B) {
    if (!testvec) return fail(c, TFHE_ERR_INVALID, "null argument");
    const HostBatch d{nullptr, in, nullptr, testvec, out, RUN_BOOTSTRAP, /*gate*/ false,
                      /*needs_key*/ true, /*may_pipeline*/ true};
    return host_batch(c, d, B);
}

int tfhe_gpu_key_switch_batch(tfhe_gpu_ctx *c, const uint32_t *in_lv1, uint32_t *out_lv0, size_t B) {
    if (!is_multi(c)) return key_switch_batch_one(c, in_lv1, out_lv0, B);
    if (B && (!in_lv1 || !out_lv0)) return fail(c, TFHE_ERR_INVALID, "null argument");
    const size_t w = tlwe0_words(c), wi = (size_t)c->P.N + 1;
    return run_sharded(c, B, [&](tfhe_gpu_ctx *s, size_t b0, size_t n) {
        return key_switch_batch_one(s, shard_items(in_lv1, b0, wi), shard_items(out_lv0, b0, w), n);
    });
}

int tfhe_gpu_reenc_key_load(tfhe_gpu_ctx *c, const uint32_t *key_encryptions, size_t len, uint32_t basebit,
                            uint32_t t, tfhe_gpu_reenc_key **out) {
    int rc = reenc_key_load_one(c, key_encryptions, len, basebit, t, out);
    if (rc || !is_multi(c)) return rc;
    for (size_t d = 1; d < c->shards.size(); d++) {  // one upload per device (host -> each HBM)
        tfhe_gpu_reenc_key *k = nullptr;
        rc = reenc_key_load_one(c->shards[d], key_encryptions, len, basebit, t, &k);
        if (rc) {
            tfhe_gpu_reenc_key_destroy(*out);
            *out = nullptr;
            return fail(c, rc, c->shards[d]->err);
        }
        (*out)->peers.push_back(k);
    }
    return TFHE_OK;
}

int tfhe_gpu_reencrypt_batch(tfhe_gpu_ctx *c, const tfhe_gpu_reenc_key *k, const uint32_t *in, uint32_t *out,
                             size_t B) {
    if (!is_multi(c)) return reencrypt_batch_one(c, k, in, out, B);
    if (!k || (B && (!in || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (k->peers.size() + 1 != c->shards.size()) return fail(c, TFHE_ERR_INVALID, "key was not loaded on this context");
    const size_t w = tlwe0_words(c);
    return run_sharded(c, B, [&](tfhe_gpu_ctx *s, size_t b0, size_t n) {
        size_t d = 0;
        while (c->shards[d] != s) d++;
        return reencrypt_batch_one(s, d ? k->peers[d - 1] : k, shard_items(in, b0, w), shard_items(out, b0, w), n);
    });
}

int tfhe_gpu_reencrypt_batch_dev(tfhe_gpu_ctx *c, const tfhe_gpu_reenc_key *k, const uint32_t *in_dev,
                                 uint32_t *out_dev, size_t B) {
    if (is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    return reencrypt_batch_one(c, k, in_dev, out_dev, B, true);
}

int tfhe_gpu_circuit_eval_dev(tfhe_gpu_ctx *c, size_t n_inputs, const uint32_t *inputs_dev, size_t n_gates,
                              const uint8_t *ops, const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs,
                              const uint32_t *out_wires, uint32_t *outputs_dev, uint32_t *levels) {
    if (is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    return circuit_eval_one(c, n_inputs, inputs_dev, n_gates, ops, in_a, in_b, n_outputs, out_wires, outputs_dev,
                            levels, true);
}

int tfhe_gpu_circuit_eval(tfhe_gpu_ctx *c, size_t n_inputs, const uint32_t *inputs, size_t n_gates, const uint8_t *ops,
                          const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires,
                          uint32_t *outputs, uint32_t *levels) {
    if (!is_multi(c))
        return circuit_eval_one(c, n_inputs, inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires, outputs, levels);
    if ((n_inputs && !inputs) || (n_gates && (!ops || !in_a || !in_b)) || (n_outputs && (!out_wires || !outputs)))
        return fail(c, TFHE_ERR_INVALID, "null argument");
    if (!c->has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    if (n_inputs + n_gates > 0xFFFFFFFFull) return fail(c, TFHE_ERR_INVALID, "too many wires");
    return circuit_eval_multi(c, n_inputs, inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires, outputs, levels);
}

}  // extern "C"
