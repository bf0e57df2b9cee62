// tfhe_gpu.cpp — C-ABI implementation (include/tfhe_gpu.h): contexts, device
// key residency and the batch entry points.  Host code; all bootstrap arithmetic
// runs in tfhe_kernels.hip.  The functions that take no context, and the circuit
// planner, are in tfhe_cpu.cpp (no HIP); what only a context over several devices
// runs is in tfhe_multi.cpp; seeded key generation and TRLWE / TRGSW encryption
// are in tfhe_encrypt.cpp; the leveled entry points (CMUX, selector sets, table
// lookup) are in tfhe_leveled.cpp, the LUT circuits in tfhe_lut.cpp.
#include "tfhe_gpu.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_math.hpp"
#include "tfhe_ctx.hpp"

using namespace tfhe;

// ---- One device ------------------------------------------------------------------
// Everything here works on one Device and reports into its `err`; the entry
// points lift a failure into the handle's (lift, for_each_slice).  The functions
// the other host units call too are declared in tfhe_ctx.hpp, the rest are static.
namespace tfhe {

// the calling thread's last failed create (tfhe_gpu_last_error(NULL))
static thread_local std::string g_create_error;
static int create_fail(int code, const std::string &msg) {
    g_create_error = msg;
    return code;
}

// The scratch arena's allocator (tfhe_scratch.hpp), user = the Device: a failed take is TFHE_ERR_OOM with
// this message.  hipFree waits for the device, so blocks may go while a _dev call's kernels still run.
static void *scratch_alloc(void *user, size_t bytes) {
    Device &d = *static_cast<Device *>(user);
    void *p = nullptr;
    hipError_t e = hipSetDevice(d.device);
    if (e == hipSuccess) e = hipMalloc(&p, bytes);
    if (e == hipSuccess) return p;
    d.err = std::string("hipMalloc: ") + hipGetErrorString(e);
    return nullptr;
}
static void scratch_free(void *user, void *p) {
    (void)hipSetDevice(static_cast<Device *>(user)->device);
    (void)hipFree(p);
}

DevTables tables(const Device &d) {
    return DevTables{d.d_twist, d.d_tw, {d.twa[0], d.twa[1], d.twa[2], d.twa[3]}};
}

// device KSK: padded rows + zero tail (tfhe_internal.hpp)
static size_t ksk_dev_bytes(const tfhe_params &p) {
    return (ksk_rows(p) * ks_stride_for((int)p.n) + KS_TAIL_WORDS) * sizeof(uint32_t);
}

// host KSK (reference layout) -> device KSK (padded rows), async on the device's stream
int upload_ksk(Device &d, const uint32_t *ksk) {
    const size_t w = d.P.n + 1, stride = d.K.ks_stride;
    d.ksk_gemm_ok = false;
    HIPCHK(d, hipMemsetAsync(d.d_ksk, 0, d.ksk_bytes, d.stream));
    HIPCHK(d, hipMemcpy2DAsync(d.d_ksk, stride * 4, ksk, w * 4, w * 4, ksk_rows(d.P), hipMemcpyHostToDevice,
                               d.stream));
    return TFHE_OK;
}

int set_key_common(Device &d, uint32_t offset, const uint32_t *tv_a, const uint32_t *tv_b) {
    const uint32_t N = d.P.N;
    d.offset = offset;
    d.K.offset = offset;
    d.testvec.assign(tv_a, tv_a + N);
    d.testvec.insert(d.testvec.end(), tv_b, tv_b + N);
    if (!d.d_testvec) HIPCHK(d, hipMalloc((void **)d.d_testvec.make(d.device), sizeof(uint32_t) * 2 * N));
    HIPCHK(d, hipMemcpyAsync(d.d_testvec, d.testvec.data(), sizeof(uint32_t) * 2 * N, hipMemcpyHostToDevice,
                             d.stream));
    if (!d.d_bk) {
        d.bk_bytes = bk_rows(d.P) * 2048 * sizeof(double);
        d.ksk_bytes = ksk_dev_bytes(d.P);
        hipError_t e = hipMalloc((void **)d.d_bk.make(d.device), d.bk_bytes);
        if (e != hipSuccess) return fail(d, TFHE_ERR_OOM, "hipMalloc(bk)");
        e = hipMalloc((void **)d.d_ksk.make(d.device), d.ksk_bytes);
        if (e != hipSuccess) return fail(d, TFHE_ERR_OOM, "hipMalloc(ksk)");
    }
    return TFHE_OK;
}

// The gemm key switch's buffers for a batch of B where it is the form to run
// (ks_use_gemm): the MFMA-layout KSK, rebuilt on the stream after a key change,
// and the partial sums.  G stays empty for the other forms (launch_key_switch
// ignores it).
int ks_gemm_args(Frame &f, size_t B, KsGemm &G) {
    Device &d = f.d;
    G = KsGemm();
    if (!ks_use_gemm(d.opts, d.K.iks_t, d.K.basebit, B, nullptr)) return TFHE_OK;
    if (!d.d_ksk_gemm) {
        hipError_t e = hipMalloc((void **)d.d_ksk_gemm.make(d.device), ks_gemm_bytes(d.K, 1024, d.K.iks_t, d.K.basebit));
        if (e != hipSuccess) return fail(d, TFHE_ERR_OOM, "hipMalloc(ksk gemm layout)");
    }
    if (!d.ksk_gemm_ok) {
        HIPCHK(d, launch_ksk_to_gemm(d.K, d.d_ksk, d.d_ksk_gemm, 1024, d.K.iks_t, d.K.basebit, d.stream));
        d.ksk_gemm_ok = true;
    }
    G.kg = d.d_ksk_gemm;
    G.part = static_cast<uint32_t *>(f.bytes(ks_gemm_part_bytes(d.K, B, 1024, d.K.basebit)));
    return f.rc();
}

// Near-tie flags (KParams::tie_flags) for B items.  The flags are all zero between
// launches, so only a new buffer is zeroed (on the device's stream).
static int ensure_tie_flags(Device &d, size_t B) {
    if (d.ties_cap >= B) return TFHE_OK;
    d.ties_cap = 0;
    const size_t want = std::max<size_t>(B, 4096);
    const hipError_t e = hipMalloc((void **)d.s_ties.make(d.device), want);  // the old flags are freed first
    if (e != hipSuccess) return fail(d, TFHE_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e));
    d.ties_cap = want;
    HIPCHK(d, hipMemsetAsync(d.s_ties, 0, want, d.stream));
    return TFHE_OK;
}

// Blind rotation (+ key switch for RUN_BOOTSTRAP) over device buffers, async.
int run_bootstrap_dev(Device &d, const uint8_t *ops, const uint32_t *a, const uint32_t *b,
                      const uint32_t *testvec_dev, uint32_t *out, size_t B, int kind, const uint32_t *idx,
                      const uint32_t *tv_sel, const uint32_t *tv_each) {
    const bool key_switch = kind == RUN_BOOTSTRAP;
    const int out_mode = kind == RUN_BOOTSTRAP ? BR_OUT_LV1 : kind == RUN_TRLWE ? BR_OUT_TRLWE : BR_OUT_LV0_EXTRACT2;
    if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    if (B == 0) return TFHE_OK;
    Frame f(d);  // the extracted TLWELv1 between the two launches, and the key switch's sums
    uint32_t *lv1 = key_switch ? f.ks_input<uint32_t>(B * 1025) : out;
    int rc = f.rc();
    if (!rc) rc = ensure_tie_flags(d, B);
    if (rc) return rc;
    KParams K = d.K;
    K.tie_flags = d.s_ties;
    K.tv_sel = tv_sel;  // LUT circuits: B table indices into testvec_dev (device), or NULL
    set_tv_each(K, tv_each);  // select nodes: the base of the entries of tv_sel with TV_SEL_EACH set, or NULL
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (d.profiling) {
        while (d.events.size() < d.ev_used + 3) {
            Event e;
            HIPCHK(d, hipEventCreate(e.make(d.device)));
            d.events.push_back(std::move(e));
        }
        for (int i = 0; i < 3; i++) ev[i] = d.events[d.ev_used + i];
        d.ev_used += 3;
        HIPCHK(d, hipEventRecord(ev[0], d.stream));
    }
    const BrBatch batch{ops, a, b, idx, testvec_dev ? testvec_dev : d.d_testvec, d.d_bk, lv1, out_mode, B};
    HIPCHK(d, launch_blind_rotate(K, tables(d), batch, d.stream, d.opts, &d.last_br));
    d.bootstraps += B;
    if (ev[1]) HIPCHK(d, hipEventRecord(ev[1], d.stream));
    d.last_ks = "";
    if (key_switch) {
        KsGemm G;
        if ((rc = ks_gemm_args(f, B, G))) return rc;
        HIPCHK(d, launch_key_switch(d.K, lv1, d.d_ksk, out, B, d.stream, d.opts, &d.last_ks, &G));
    }
    if (ev[2]) HIPCHK(d, hipEventRecord(ev[2], d.stream));
    return TFHE_OK;
}

static bool staged(const Device &d) { return d.host_staging == TFHE_STAGING_PINNED; }

// Pinned host buffer of at least `bytes`; a new one has at least `floor` (nothing may be in flight from the old one).
static int ensure_pinned(Device &d, PinBuf &b, size_t bytes, size_t floor = 0) {
    if (b.bytes >= bytes) return TFHE_OK;
    b.bytes = 0;
    const size_t want = std::max(bytes, floor);
    HIPCHK(d, hipHostMalloc((void **)b.p.make(d.device), want, hipHostMallocDefault));
    b.bytes = want;
    return TFHE_OK;
}
constexpr size_t STAGE_FLOOR = (size_t)1 << 20;  // the staging arenas start at 1 MiB

// Host -> device memory at `dst`.  Pageable: one hipMemcpyAsync from the caller's buffer.  Staged
// (TFHE_OPT_HOST_STAGING): a host memcpy into this device's pinned arena, then the DMA from
// there, so concurrent devices' copies do not go through the runtime's pageable staging
// (for hosts where those serialise across host threads; on the MI355X box they do not and
// pageable copies are faster).  The arena is reused from
// offset 0 after every synchronisation of the stream (d2h_sync); when it is full the stream
// is synchronised first, so no copy in flight ever reads overwritten bytes.
int h2d_copy(Device &d, void *dst, const void *src, size_t bytes) {
    if (!staged(d) || !bytes) {
        HIPCHK(d, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, d.stream));
        return TFHE_OK;
    }
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (d.stage_used + need > d.stage_in.bytes) {
        HIPCHK(d, hipStreamSynchronize(d.stream));
        d.stage_used = 0;
        if (need > d.stage_in.bytes) {  // grow (doubling) only when one copy does not fit the empty arena
            const int rc = ensure_pinned(d, d.stage_in, std::max(need, 2 * d.stage_in.bytes), STAGE_FLOOR);
            if (rc) return rc;
        }
    }
    char *p = d.stage_in.p + d.stage_used;
    std::memcpy(p, src, bytes);
    HIPCHK(d, hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, d.stream));
    d.stage_used += need;
    return TFHE_OK;
}

// Synchronise the device's stream and fail the call if a kernel on it set the
// device error word (a slot-counter wait of the blind rotation gave up: its
// words are not the reference's).  The word is copied into pinned host memory
// on the stream, so the one synchronisation covers both; a reported error is
// cleared, and the context stays usable.
// Queue the copy of the device error word (and the recompute counter) into
// pinned host memory on the device's stream.
static int queue_err_copy(Device &d) {
    HIPCHK(d, hipMemcpyAsync(d.h_err, d.d_err, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
    return TFHE_OK;
}

// After a synchronisation that covered queue_err_copy: fail the call if a
// kernel set the error word (clearing it; the context stays usable).
static int check_err_word(Device &d) {
    d.near_tie_items = d.h_err[1];
    const uint32_t e = *d.h_err;
    if (!e) return TFHE_OK;
    *d.h_err = 0;
    HIPCHK(d, hipMemsetAsync(d.d_err, 0, sizeof(uint32_t), d.stream));
    HIPCHK(d, hipStreamSynchronize(d.stream));
    std::string what;
    if (e & DEV_ERR_GATE_WAIT) what += "slot-counter protocol failure: a gate wave's wait for a BK slot timed out";
    if (e & DEV_ERR_LOADER_WAIT)
        what += std::string(what.empty() ? "slot-counter protocol failure:" : " and") +
                " a loader wave's wait for a free BK slot timed out";
    if (e & DEV_ERR_LDS_LAYOUT) what += std::string(what.empty() ? "" : "; ") + "LDS array not at address 0, nothing computed";
    return fail(d, TFHE_ERR_DEVICE,
                "blind rotation: " + what + " (device error word 0x" +
                    [&] { char b[16]; std::snprintf(b, sizeof b, "%x", e); return std::string(b); }() +
                    "); the outputs of the work since the last synchronisation are invalid");
}

int sync_check(Device &d) {
    int rc = queue_err_copy(d);
    if (rc) return rc;
    HIPCHK(d, hipStreamSynchronize(d.stream));
    return check_err_word(d);
}

// 64-bit fingerprints of this device's BK and KSK (k_checksum), synchronous.
int key_fingerprint(Device &d, uint64_t &bk, uint64_t &ksk) {
    auto *dw = reinterpret_cast<unsigned long long *>(d.d_err + 2);
    auto *h = reinterpret_cast<volatile unsigned long long *>(d.h_err + 2);
    HIPCHK(d, hipSetDevice(d.device));
    HIPCHK(d, launch_checksum(d.d_bk, d.bk_bytes, dw, d.stream));
    HIPCHK(d, hipMemcpyAsync(d.h_err + 2, dw, 8, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(d, hipStreamSynchronize(d.stream));
    bk = *h;
    HIPCHK(d, launch_checksum(d.d_ksk, d.ksk_bytes, dw, d.stream));
    HIPCHK(d, hipMemcpyAsync(d.h_err + 2, dw, 8, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(d, hipStreamSynchronize(d.stream));
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
static int key_admission(Device &d) {
    // refused until measured: a failure below (absmax launch, copy, sync) must not
    // leave the previous key's admission in place
    d.opts.key_fused_ok = 0;
    auto *dw = reinterpret_cast<unsigned long long *>(d.d_err + 2);
    auto *h = reinterpret_cast<volatile unsigned long long *>(d.h_err + 2);
    HIPCHK(d, launch_absmax(d.d_bk, d.bk_bytes / sizeof(double), dw, d.stream));
    HIPCHK(d, launch_row_energy_max(d.d_bk, (size_t)d.P.n * 2 * d.P.L, dw + 1, d.stream));
    HIPCHK(d, hipMemcpyAsync(d.h_err + 2, dw, 16, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(d, hipStreamSynchronize(d.stream));
    const unsigned long long bits = h[0], ebits = h[1];
    double m, e;
    std::memcpy(&m, (const void *)&bits, 8);
    std::memcpy(&e, (const void *)&ebits, 8);
    d.bk_absmax = std::ldexp(m, 10);  // the device BK is the reference's spectrum x 2^-10 (k_bk_permute)
    // row energy: device spectrum energy x 2^20 = reference spectrum energy = 2048 x N x RMS^2
    d.bk_row_rms = std::sqrt(std::ldexp(e, 20) / (2048.0 * d.P.N)) / 2147483648.0;
    d.opts.key_fused_ok =
        d.bk_absmax <= FUSED_BK_SPECTRUM_MAX && d.bk_row_rms <= FUSED_BK_ROW_RMS_MAX ? 1 : 0;  // NaN fails
    return TFHE_OK;
}

// The outputs and the error word in one synchronisation: the word's copy is
// queued first, so it has landed when the outputs have (one round trip fewer
// than copying it after them: DESIGN.md §2.1).
int d2h_sync(Device &d, void *dst, const void *src, size_t bytes) {
    int rc = queue_err_copy(d);
    if (rc) return rc;
    if (staged(d) && bytes) {  // DMA into the pinned arena, one synchronisation, then a host memcpy
        rc = ensure_pinned(d, d.stage_out, bytes, STAGE_FLOOR);
        if (rc) return rc;
        HIPCHK(d, hipMemcpyAsync(d.stage_out.p, src, bytes, hipMemcpyDeviceToHost, d.stream));
        HIPCHK(d, hipStreamSynchronize(d.stream));
        d.stage_used = 0;  // every staged H2D of the call has landed
        std::memcpy(dst, d.stage_out.p, bytes);
        return check_err_word(d);
    }
    HIPCHK(d, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, d.stream));
    // a pageable destination makes the copy synchronous: the stream is idle by
    // now and hipStreamQuery says so at once, where hipStreamSynchronize on an
    // idle stream still took ~19 us (profiles/r03_host_path_trace.txt)
    const hipError_t q = hipStreamQuery(d.stream);
    if (q == hipErrorNotReady) HIPCHK(d, hipStreamSynchronize(d.stream));
    else HIPCHK(d, q);
    return check_err_word(d);
}

// FFT constant tables (fft.zig:92-106 twists, :590-616 recurrence) from the
// chosen cos/sin source (host_math.hpp), uploaded to the device.
static int build_tables(Device &d, int source) {
    std::vector<double> tre, tim, fre, fim, ire, iim;
    host::twist_table(d.P.N, tre, tim, source);
    host::stage_twiddles(d.P.N, false, fre, fim, source);
    host::stage_twiddles(d.P.N, true, ire, iim, source);
    // the inverse kernels use conj(forward): that must equal the inverse
    // recurrence bit for bit (both sources have an odd sin and an even cos)
    for (size_t i = 0; i < fre.size(); i++)
        if (std::memcmp(&fre[i], &ire[i], 8) != 0 || -fim[i] != iim[i])
            return fail(d, TFHE_ERR_INVALID, "inverse twiddle table is not the conjugate of the forward one");
    std::vector<C2> tw2(tre.size()), st2(fre.size());
    for (size_t i = 0; i < tre.size(); i++) tw2[i] = C2{tre[i], tim[i]};
    for (size_t i = 0; i < fre.size(); i++) st2[i] = C2{fre[i], fim[i]};
    // passA's bf_m1 (tfhe_kernels.hip) relies on W4[1].im == W8[2].im == -1.0 exactly
    if (st2[2].y != -1.0 || st2[5].y != -1.0)
        return fail(d, TFHE_ERR_INVALID, "twiddle table: W4[1] / W8[2] imaginary part is not exactly -1");
    HIPCHK(d, hipSetDevice(d.device));
    if (!d.d_twist) HIPCHK(d, hipMalloc((void **)d.d_twist.make(d.device), sizeof(C2) * tw2.size()));
    if (!d.d_tw) HIPCHK(d, hipMalloc((void **)d.d_tw.make(d.device), sizeof(C2) * st2.size()));
    HIPCHK(d, hipStreamSynchronize(d.stream));  // no launch may still read the old tables
    HIPCHK(d, hipMemcpy(d.d_twist, tw2.data(), sizeof(C2) * tw2.size(), hipMemcpyHostToDevice));
    HIPCHK(d, hipMemcpy(d.d_tw, st2.data(), sizeof(C2) * st2.size(), hipMemcpyHostToDevice));
    d.twa[0] = st2[2];
    d.twa[1] = st2[4];
    d.twa[2] = st2[5];
    d.twa[3] = st2[6];
    d.twiddle_source = source;
    return TFHE_OK;
}

// Every key load on device 0 ends here: admit the fused arithmetic or not.  An
// unmeasured key is not a loaded key.
int key_loaded(Device &d, bool from_keygen) {
    d.key_from_keygen = from_keygen;
    const int rc = key_admission(d);
    d.has_key = rc == TFHE_OK;
    return rc;
}

// A new context's device: its stream, error word and FFT tables.
static int init_device(Device &d, const tfhe_params &p, int device) {
    d.P = p;
    d.device = device;
    d.K = KParams{(int)p.n, (int)p.N, (int)p.L, (int)p.bgbit, (int)p.basebit,
                  (int)p.iks_t, 0, ks_stride_for((int)p.n), nullptr, 0u, 0u, nullptr, 0};
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(d, e, "hipSetDevice");
    e = hipStreamCreateWithFlags(d.own_stream.make(device), hipStreamNonBlocking);
    if (e != hipSuccess) return hip_fail(d, e, "hipStreamCreate");
    d.stream = d.own_stream;
    e = hipMalloc((void **)d.d_err.make(device), 64);
    if (e == hipSuccess) e = hipMemset(d.d_err, 0, 64);
    if (e == hipSuccess) e = hipHostMalloc((void **)d.h_err.make(device), 64, hipHostMallocDefault);
    if (e != hipSuccess) return hip_fail(d, e, "device error word");
    std::memset(d.h_err, 0, 64);
    d.K.err = d.d_err;
    d.scratch.set_allocator({scratch_alloc, scratch_free, &d});  // a context's devices stay where they are (tfhe_gpu_ctx::dev)
    return build_tables(d, TFHE_TWIDDLES_GLIBC);
}

}  // namespace tfhe

// a context under construction: destroyed like any other if a step fails
using Handle = std::unique_ptr<tfhe_gpu_ctx, void (*)(tfhe_gpu_ctx *)>;

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
    Handle c(new tfhe_gpu_ctx, tfhe_gpu_destroy);
    c->P = *params;
    c->dev.emplace_back();
    const int rc = init_device(c->dev[0], *params, device);
    if (rc) return create_fail(rc, "tfhe_gpu_create: " + c->dev[0].err);
    *out = c.release();
    return TFHE_OK;
}

void tfhe_gpu_destroy(tfhe_gpu_ctx *c) {
    if (!c) return;
    for (Device &d : c->dev) {
        (void)hipSetDevice(d.device);
        (void)hipStreamSynchronize(d.stream);  // NULL is a valid stream here (the device's null stream)
    }
    destroy_comms(c);  // before the streams they broadcast on
    while (!c->dev.empty()) c->dev.pop_back();  // last to first: the thread is left on device 0's GPU
    delete c;
}

const char *tfhe_gpu_last_error(const tfhe_gpu_ctx *c) {
    if (c) return c->err.c_str();
    return g_create_error.empty() ? "null context" : g_create_error.c_str();
}

int tfhe_gpu_key_fingerprint(tfhe_gpu_ctx *c, uint64_t *bk, uint64_t *ksk) {
    if (!c || !bk || !ksk) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (!c->dev[0].has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    uint64_t b = 0, k = 0;
    const int rc = key_fingerprint(c->dev[0], b, k);
    if (rc) return lift(c, 0, rc);
    *bk = b;
    *ksk = k;
    return TFHE_OK;
}

int tfhe_gpu_sync(tfhe_gpu_ctx *c) {
    if (!c) return TFHE_ERR_INVALID;
    return on_device0(c, sync_check);
}

// The device queues its own work on its stream too (the MFMA-layout KSK build,
// the near-tie flag and error-word clears): the new stream waits for everything
// queued on the old one, so a _dev call on the new stream never overtakes it.
static int switch_stream(Device &d, hipStream_t ns) {
    if (ns == d.stream) return TFHE_OK;
    if (!d.stream_ev) HIPCHK(d, hipEventCreateWithFlags(d.stream_ev.make(d.device), hipEventDisableTiming));
    HIPCHK(d, hipEventRecord(d.stream_ev, d.stream));
    HIPCHK(d, hipStreamWaitEvent(ns, d.stream_ev, 0));
    d.stream = ns;
    return TFHE_OK;
}

// ABI 7: NULL is the device's null stream (torch's default stream has handle 0),
// no longer "back to the context's own stream", which is tfhe_gpu_reset_stream.
// Up to ABI 6 a caller passing torch's default stream got the context's own
// non-blocking stream, unordered with torch's work.  Both act on device 0 only.
int tfhe_gpu_set_stream(tfhe_gpu_ctx *c, void *s) {
    if (!c) return TFHE_ERR_INVALID;
    return on_device0(c, [&](Device &d) { return switch_stream(d, (hipStream_t)s); });
}

int tfhe_gpu_reset_stream(tfhe_gpu_ctx *c) {
    if (!c) return TFHE_ERR_INVALID;
    return on_device0(c, [](Device &d) { return switch_stream(d, d.own_stream); });
}

int tfhe_gpu_load_cloud_key(tfhe_gpu_ctx *c, uint32_t offset, const uint32_t *tv_a, const uint32_t *tv_b,
                            const double *bsk, size_t bsk_len, const uint32_t *ksk, size_t ksk_len) {
    if (!c || !tv_a || !tv_b || !bsk || !ksk) return fail(c, TFHE_ERR_INVALID, "null argument");
    const size_t rows = bk_rows(c->P);
    if (bsk_len != rows * 2 * c->P.N) return fail(c, TFHE_ERR_INVALID, "bsk_len != n*2L*2*N");
    if (ksk_len != ksk_words(c->P)) return fail(c, TFHE_ERR_INVALID, "ksk_len != N*t*2^basebit*(n+1)");
    const int rc = on_device0(c, [&](Device &d) -> int {
        int rc = set_key_common(d, offset, tv_a, tv_b);
        if (rc) return rc;
        Frame f(d);
        const double *staged_bk = f.h2d(bsk, bsk_len * sizeof(double));
        if (f.rc()) return f.rc();
        HIPCHK(d, launch_bk_permute(d.K, staged_bk, d.d_bk, rows, d.stream));
        rc = upload_ksk(d, ksk);
        if (rc) return rc;
        HIPCHK(d, launch_ksk_zero_k0(d.K, d.d_ksk, d.stream));  // reference leaves k=0 rows undefined
        HIPCHK(d, hipStreamSynchronize(d.stream));
        return key_loaded(d, /*from_keygen*/ false);
    });
    return rc ? rc : broadcast_key(c);
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
    if (!c->dev[0].has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    return on_device0(c, [&](Device &d) -> int {
        HIPCHK(d, hipMemcpyAsync(bsk_dev, d.d_bk, d.bk_bytes, hipMemcpyDeviceToDevice, d.stream));
        HIPCHK(d, hipMemcpyAsync(ksk_dev, d.d_ksk, d.ksk_bytes, hipMemcpyDeviceToDevice, d.stream));
        HIPCHK(d, hipStreamSynchronize(d.stream));
        if (offset) *offset = d.offset;
        if (testvec) std::memcpy(testvec, d.testvec.data(), sizeof(uint32_t) * 2 * d.P.N);
        return TFHE_OK;
    });
}

int tfhe_gpu_import_key_device(tfhe_gpu_ctx *c, const void *bsk_dev, const void *ksk_dev, uint32_t offset,
                               const uint32_t *testvec) {
    if (!c || !bsk_dev || !ksk_dev || !testvec) return fail(c, TFHE_ERR_INVALID, "null argument");
    const int rc = on_device0(c, [&](Device &d) -> int {
        int rc = set_key_common(d, offset, testvec, testvec + d.P.N);
        if (rc) return rc;
        HIPCHK(d, hipMemcpyAsync(d.d_bk, bsk_dev, d.bk_bytes, hipMemcpyDeviceToDevice, d.stream));
        HIPCHK(d, hipMemcpyAsync(d.d_ksk, ksk_dev, d.ksk_bytes, hipMemcpyDeviceToDevice, d.stream));
        HIPCHK(d, launch_ksk_zero_k0(d.K, d.d_ksk, d.stream));
        d.ksk_gemm_ok = false;
        HIPCHK(d, hipStreamSynchronize(d.stream));
        return key_loaded(d, /*from_keygen*/ false);
    });
    return rc ? rc : broadcast_key(c);
}

// Device key -> reference host layout: BK un-permuted (and un-scaled) by
// k_bk_permute's inverse, KSK rows un-padded.
int tfhe_gpu_export_cloud_key(tfhe_gpu_ctx *c, uint32_t *offset, uint32_t *tv_a, uint32_t *tv_b, double *bsk,
                              uint32_t *ksk) {
    if (!c) return TFHE_ERR_INVALID;
    if (!c->dev[0].has_key) return fail(c, TFHE_ERR_NO_KEY, "no cloud key loaded");
    return on_device0(c, [&](Device &d) -> int {
        const size_t N = d.P.N;
        Frame f(d);  // open until the stream has been waited for
        if (offset) *offset = d.offset;
        if (tv_a) std::memcpy(tv_a, d.testvec.data(), N * sizeof(uint32_t));
        if (tv_b) std::memcpy(tv_b, d.testvec.data() + N, N * sizeof(uint32_t));
        if (bsk) {
            const size_t rows = bk_rows(d.P), bytes = rows * 2 * N * sizeof(double);
            double *staged_bk = static_cast<double *>(f.bytes(bytes));
            if (f.rc()) return f.rc();
            HIPCHK(d, launch_bk_unpermute(d.K, d.d_bk, staged_bk, rows, d.stream));
            HIPCHK(d, hipMemcpyAsync(bsk, staged_bk, bytes, hipMemcpyDeviceToHost, d.stream));
        }
        if (ksk) {
            const size_t w = d.P.n + 1;
            HIPCHK(d, hipMemcpy2DAsync(ksk, w * 4, d.d_ksk, (size_t)d.K.ks_stride * 4, w * 4, ksk_rows(d.P),
                                       hipMemcpyDeviceToHost, d.stream));
        }
        HIPCHK(d, hipStreamSynchronize(d.stream));
        return TFHE_OK;
    });
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

}  // extern "C"

namespace tfhe {

// Host-buffer bootstrap of B >= one whole-form round, pipelined (DESIGN.md
// §2.1): the batch is cut into chunks of #CUs items (a quarter round: #CUs/4
// workgroups of the whole form).  Worker s owns stream s and chunks s, s+S, ...;
// per chunk it copies the caller's inputs into pinned staging, then enqueues
// H2D -> blind rotation (whole form; the guard's recompute) -> key switch ->
// D2H on its stream, so chunk k+1's copies run while chunks <= k compute and
// the S streams' kernels share the CUs.  Each worker then waits for its stream
// and copies its chunks' outputs to the caller.  ops / b / tv_dev may be NULL.
static int pipelined_bootstrap(Frame &f, const uint8_t *ops, const uint32_t *a, const uint32_t *b,
                        const uint32_t *tv_dev, uint32_t *out, size_t B) {
    Device &d = f.d;
    const size_t w = tlwe0_words(d.P), wb = w * 4, chunk = device_cus();
    const size_t nch = (B + chunk - 1) / chunk;
    const int S = (int)std::min<size_t>(PIPE_STREAMS, nch);
    // staging layout per item: op byte region, then a, then b (all chunks contiguous)
    const size_t op_bytes = ops ? (B + 15) / 16 * 16 : 0, a_bytes = B * wb, b_bytes = b ? B * wb : 0;
    int rc = ensure_pinned(d, d.pin_in, op_bytes + a_bytes + b_bytes);
    if (!rc) rc = ensure_pinned(d, d.pin_out, B * wb);
    // every slice now: the workers never touch the frame
    uint8_t *d_ops = ops ? f.take<uint8_t>(B) : nullptr;
    uint32_t *d_a = f.take<uint32_t>(B * w), *d_b = b ? f.take<uint32_t>(B * w) : nullptr, *d_out = f.take<uint32_t>(B * w);
    uint32_t *d_lv1 = f.ks_input<uint32_t>(B * 1025);
    if (!rc) rc = f.rc();
    if (!rc) rc = ensure_tie_flags(d, B);
    if (rc) return rc;
    if (!d.pipe_ev) HIPCHK(d, hipEventCreateWithFlags(d.pipe_ev.make(d.device), hipEventDisableTiming));
    for (Stream &p : d.pipe)
        if (!p) HIPCHK(d, hipStreamCreateWithFlags(p.make(d.device), hipStreamNonBlocking));
    if (!d.workers) d.workers.reset(new WorkerPool(PIPE_STREAMS));
    // the GEMM key switch per chunk (the default form where it applies): its MFMA-layout
    // key is built once on the device's stream, and each stream gets its own
    // partial-sum buffer, so every chunk runs the same key-switch form as the
    // unpipelined path (last_kernels names it)
    KsGemm G;
    rc = ks_gemm_args(f, chunk, G);
    if (rc) return rc;
    std::vector<KsGemm> Gs(S, G);
    for (int s = 1; s < S && G.kg; s++)
        if ((rc = ks_gemm_args(f, chunk, Gs[s]))) return rc;
    // everything enqueued on the device's stream (key loads, the flags' memset) first
    HIPCHK(d, hipEventRecord(d.pipe_ev, d.stream));
    LaunchOpts o = d.opts;
    if (!o.br_form) o.br_form = 1;  // whole form for every chunk (a chunk is a quarter round)
    char *pin_ops = d.pin_in.p, *pin_a = pin_ops + op_bytes, *pin_b = pin_a + a_bytes;
    std::vector<hipError_t> err(S, hipSuccess);
    std::vector<const char *> where(S, "");
    d.workers->run(S, [&](int s) {
        hipStream_t st = d.pipe[s];
        auto chk = [&](hipError_t e, const char *what) {
            if (e != hipSuccess && err[s] == hipSuccess) {
                err[s] = e;
                where[s] = what;
            }
            return e == hipSuccess;
        };
        if (!chk(hipSetDevice(d.device), "hipSetDevice") || !chk(hipStreamWaitEvent(st, d.pipe_ev, 0), "hipStreamWaitEvent"))
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
            KParams K = d.K;
            K.tie_flags = d.s_ties + k0;
            const BrBatch batch{ops ? d_ops + k0 : nullptr, d_a + k0 * w, b ? d_b + k0 * w : nullptr, nullptr,
                                tv_dev ? tv_dev : d.d_testvec, d.d_bk, d_lv1 + k0 * 1025, BR_OUT_LV1, n};
            if (!chk(launch_blind_rotate(K, tables(d), batch, st, o, s == 0 && k == 0 ? &d.last_br : nullptr),
                     "blind rotation") ||
                !chk(launch_key_switch(d.K, d_lv1 + k0 * 1025, d.d_ksk, d_out + k0 * w, n, st, d.opts,
                                       s == 0 && k == 0 ? &d.last_ks : nullptr, &Gs[s]),
                     "key switch") ||
                !chk(hipMemcpyAsync(d.pin_out.p + k0 * wb, d_out + k0 * w, n * wb, hipMemcpyDeviceToHost, st), "D2H"))
                return;
        }
        if (!chk(hipStreamSynchronize(st), "hipStreamSynchronize")) return;
        for (size_t k = (size_t)s; k < nch; k += (size_t)S) {
            const size_t k0 = k * chunk, n = std::min(B, k0 + chunk) - k0;
            std::memcpy(out + k0 * w, d.pin_out.p + k0 * wb, n * wb);
        }
    });
    for (int s = 0; s < S; s++)
        if (err[s] != hipSuccess) {
            for (int t = 0; t < S; t++) (void)hipStreamSynchronize(d.pipe[t]);
            return hip_fail(d, err[s], where[s]);
        }
    d.bootstraps += B;
    return sync_check(d);  // the device error word (and the recompute counter) after all streams
}

// The pipeline serves host-buffer bootstraps of at least one whole-form round
// (4 x #CUs items) unless TFHE_OPT_HOST_PIPELINE = 0 or device timing is on
// (its events bracket single launches on the device's stream).
static bool use_pipeline(const Device &d, size_t B) {
    return d.pipeline && !d.profiling && B >= 4 * device_cus();
}

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
// Items [first, first + B) of the batch on one device.
static int host_batch_on(Device &d, const HostBatch &hb, size_t first, size_t B) {
    if (B == 0) return TFHE_OK;
    const size_t w = tlwe0_words(d.P), wo = hb.kind == RUN_TRLWE ? 2 * (size_t)d.P.N : w;
    const uint8_t *ops = hb.gate ? hb.ops + first : nullptr;
    const uint32_t *a = hb.a + first * w, *b = hb.gate ? hb.b + first * w : nullptr;
    uint32_t *out = hb.out + first * wo;
    if (hb.gate)
        for (size_t i = 0; i < B; i++)
            if (ops[i] > TFHE_GATE_ORYN && ops[i] != TFHE_GATE_COPY) return fail(d, TFHE_ERR_INVALID, "bad gate op");
    HIPCHK(d, hipSetDevice(d.device));
    if (hb.needs_key && !d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t in_bytes = B * w * 4;
    Frame f(d);
    Io io{f, /*dev*/ false};
    const uint32_t *tv = hb.testvec ? f.h2d(hb.testvec, 2 * d.P.N * 4) : nullptr;
    if (f.rc()) return f.rc();
    if (hb.may_pipeline && use_pipeline(d, B)) return pipelined_bootstrap(f, ops, a, b, tv, out, B);
    if (hb.gate) io.in(ops, B);
    io.in(a, in_bytes);
    if (hb.gate) io.in(b, in_bytes);
    int rc = io.out(out, B * wo * 4);
    if (!rc) rc = run_bootstrap_dev(d, ops, a, b, tv, out, B, hb.kind);
    return rc ? rc : io.finish();
}

}  // namespace tfhe

// ---- Proxy re-encryption ------------------------------------
struct tfhe_gpu_reenc_key {
    uint32_t basebit = 0, t = 0;
    struct Copy {
        int device = 0;
        DevPtr<uint32_t> key;       // padded rows like the KSK (K.ks_stride words) + zero tail
        DevPtr<uint32_t> key_gemm;  // the gemm key switch's layout of `key` (basebit 2, t 7..9), or NULL
    };
    std::vector<Copy> dev;  // one upload per device of the context that loaded it, in its order
};

namespace tfhe {

static int reenc_key_upload(Device &d, const uint32_t *key_encryptions, uint32_t basebit, uint32_t t,
                            tfhe_gpu_reenc_key::Copy &k) {
    const size_t n = d.P.n, rows = n * t * ((size_t)1 << basebit);
    HIPCHK(d, hipSetDevice(d.device));
    k.device = d.device;
    const size_t stride = d.K.ks_stride, bytes = (rows * stride + KS_TAIL_WORDS) * sizeof(uint32_t);
    hipError_t e = hipMalloc((void **)k.key.make(d.device), bytes);
    if (e != hipSuccess) return fail(d, TFHE_ERR_OOM, "hipMalloc(reencryption key)");
    e = hipMemsetAsync(k.key, 0, bytes, d.stream);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(k.key, stride * 4, key_encryptions, (n + 1) * 4, (n + 1) * 4, rows,
                             hipMemcpyHostToDevice, d.stream);
    if (e == hipSuccess) e = launch_key_zero_k0(d.K, k.key, (int)n, (int)t, (int)basebit, d.stream);
    if (e == hipSuccess && ks_gemm_supported((int)t, (int)basebit)) {  // §4.4b layout for the gemm form
        e = hipMalloc((void **)k.key_gemm.make(d.device), ks_gemm_bytes(d.K, (int)n, (int)t, (int)basebit));
        if (e == hipSuccess) e = launch_ksk_to_gemm(d.K, k.key, k.key_gemm, (int)n, (int)t, (int)basebit, d.stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
    if (e != hipSuccess) return hip_fail(d, e, "upload reencryption key");
    return TFHE_OK;
}

// dev: in and out are device pointers (tfhe_gpu_reencrypt_batch_dev): the input is copied
// device-to-device into the staging buffer, the kernel writes `out` directly, and the call
// returns without waiting (async on the device's stream, like the other _dev entries)
static int reencrypt_on(Device &d, const tfhe_gpu_reenc_key &key, size_t slot, const uint32_t *in, uint32_t *out,
                        size_t B, bool dev = false) {
    const tfhe_gpu_reenc_key::Copy &k = key.dev[slot];
    if (k.device != d.device) return fail(d, TFHE_ERR_INVALID, "key belongs to another device");
    if (B == 0) return TFHE_OK;
    HIPCHK(d, hipSetDevice(d.device));
    const size_t w = tlwe0_words(d.P);
    Frame f(d);
    Io io{f, dev};
    uint32_t *x = f.ks_input<uint32_t>(B * w);  // the gemm form reads whole blocks of 8
    int rc = io.out(out, B * w * 4);
    KsGemm G;
    if (k.key_gemm) {
        G.kg = k.key_gemm;
        G.part = static_cast<uint32_t *>(f.bytes(ks_gemm_part_bytes(d.K, B, (int)d.P.n, (int)key.basebit)));
        rc = f.rc();
    }
    if (rc) return rc;
    if (dev) HIPCHK(d, hipMemcpyAsync(x, in, B * w * 4, hipMemcpyDeviceToDevice, d.stream));
    else if ((rc = h2d_copy(d, x, in, B * w * 4))) return rc;
    HIPCHK(d, launch_reencrypt(d.K, (int)key.t, (int)key.basebit, x, k.key, out, B, d.stream, d.opts, &d.last_ks, &G));
    return io.finish();
}

}  // namespace tfhe

// Circuits (planner: tfhe_cpu.cpp).  The one context-free function here: it needs the launchers' cost model.
extern "C" int tfhe_circuit_schedule(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
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

namespace tfhe {

// Device side of a plan on one device: wire table with the inputs, the gather
// indices and op codes, uploaded on its stream.
int upload_plan(Frame &f, const CircuitPlan &pl, size_t W, size_t n_inputs, const uint32_t *inputs, PlanBufs &pb,
                bool inputs_on_device) {
    Device &d = f.d;
    const size_t w1 = tlwe0_words(d.P);
    HIPCHK(d, hipSetDevice(d.device));
    DescBlob blob;  // the gather indices, then the op bytes padded to words: one copy
    blob.add(pl.idx.data(), pl.idx.size());
    const size_t op_at = blob.add_bytes(pl.cops.data(), pl.cops.size());
    pb.wires = f.take<uint32_t>(W * w1);
    pb.idx = blob.upload(f);
    if (f.rc()) return f.rc();
    pb.ops = reinterpret_cast<const uint8_t *>(pb.idx + op_at);
    if (n_inputs)
        HIPCHK(d, hipMemcpyAsync(pb.wires, inputs, n_inputs * w1 * 4,
                                 inputs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, d.stream));
    return TFHE_OK;
}

// A whole circuit on one device.
// dev: inputs and outputs are device pointers (tfhe_gpu_circuit_eval_dev): the inputs are copied
// device-to-device into the wire table, the outputs gathered straight into `outputs`, and the call
// returns without waiting (async on the device's stream, like the other _dev entries)
int circuit_eval_one(Device &d, size_t n_inputs, const uint32_t *inputs, size_t n_gates, const uint8_t *ops,
                     const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires,
                     uint32_t *outputs, uint32_t *depth_out, bool dev) {
    if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    const size_t W = n_inputs + n_gates, w1 = tlwe0_words(d.P);
    HIPCHK(d, hipSetDevice(d.device));
    CircuitPlan pl;
    if (const char *why = plan_circuit(n_inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires, d.circuit_pack != 0,
                                       device_cus(), level_cost, pl))
        return fail(d, TFHE_ERR_INVALID, why);
    Frame f(d);
    Io io{f, dev};
    PlanBufs pb;
    int rc = upload_plan(f, pl, W, n_inputs, inputs, pb, dev);
    if (!rc && n_outputs) rc = io.out(outputs, n_outputs * w1 * 4);
    if (rc) return rc;
    const auto &bs = pl.bs;
    const auto &nots = pl.nots;
    const uint32_t max_level = pl.max_level;
    uint32_t *wires = pb.wires;
    const uint32_t *d_idx = pb.idx;
    const uint8_t *d_ops = pb.ops;
    size_t ip = 0, op_pos = 0, sp = n_inputs;
    for (uint32_t lv = 0; lv <= max_level; lv++) {
        const size_t nb = bs[lv].size(), nn = nots[lv].size();
        if (nb) {
            rc = run_bootstrap_dev(d, d_ops + op_pos, wires, wires, nullptr, wires + sp * w1, nb, RUN_BOOTSTRAP,
                                   d_idx + ip);
            if (rc) return rc;
            ip += 2 * nb;
            op_pos += nb;
            sp += nb;
        }
        if (nn) {
            HIPCHK(d, launch_tlwe_gather(d.K, wires, d_idx + ip, wires + sp * w1, nn, true, d.stream));
            ip += nn;
            sp += nn;
        }
    }
    if (n_outputs) HIPCHK(d, launch_tlwe_gather(d.K, wires, d_idx + ip, outputs, n_outputs, false, d.stream));
    if ((rc = io.finish())) return rc;
    if (depth_out) *depth_out = max_level;
    return TFHE_OK;
}

static int key_switch_on(Device &d, const uint32_t *in_lv1, uint32_t *out_lv0, size_t B) {
    if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
    if (B == 0) return TFHE_OK;
    HIPCHK(d, hipSetDevice(d.device));
    Frame f(d);
    Io io{f, /*dev*/ false};
    uint32_t *lv1 = f.ks_input<uint32_t>(B * 1025);
    int rc = io.out(out_lv0, B * tlwe0_words(d.P) * 4);
    if (!rc) rc = h2d_copy(d, lv1, in_lv1, B * 1025 * 4);
    if (rc) return rc;
    in_lv1 = lv1;
    KsGemm G;
    if ((rc = ks_gemm_args(f, B, G))) return rc;
    HIPCHK(d, launch_key_switch(d.K, in_lv1, d.d_ksk, out_lv0, B, d.stream, d.opts, &d.last_ks, &G));
    return io.finish();
}

}  // namespace tfhe

extern "C" {

int tfhe_gpu_gate_batch_dev(tfhe_gpu_ctx *c, const uint8_t *ops_dev, const uint32_t *a_dev, const uint32_t *b_dev,
                            uint32_t *out_dev, size_t B) {
    if (!c || (B && (!ops_dev || !a_dev || !b_dev || !out_dev))) return fail(c, TFHE_ERR_INVALID, "null argument");
    return on_device0(c, [&](Device &d) -> int {
        return run_bootstrap_dev(d, ops_dev, a_dev, b_dev, nullptr, out_dev, B, RUN_BOOTSTRAP);
    });
}

int tfhe_gpu_bootstrap_batch_dev(tfhe_gpu_ctx *c, const uint32_t *in_dev, uint32_t *out_dev, size_t B) {
    if (!c || (B && (!in_dev || !out_dev))) return fail(c, TFHE_ERR_INVALID, "null argument");
    return on_device0(c, [&](Device &d) -> int {
        return run_bootstrap_dev(d, nullptr, in_dev, nullptr, nullptr, out_dev, B, RUN_BOOTSTRAP);
    });
}

int tfhe_gpu_bootstrap_lut_batch_dev(tfhe_gpu_ctx *c, const uint32_t *in_dev, const uint32_t *testvec_dev,
                                     uint32_t *out_dev, size_t B) {
    if (!c || !testvec_dev || (B && (!in_dev || !out_dev))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    return on_device0(c, [&](Device &d) -> int {
        if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
        return run_bootstrap_dev(d, nullptr, in_dev, nullptr, testvec_dev, out_dev, B, RUN_BOOTSTRAP);
    });
}

int tfhe_gpu_profile_begin(tfhe_gpu_ctx *c) {
    if (!c) return TFHE_ERR_INVALID;
    c->dev[0].profiling = true;
    c->dev[0].ev_used = 0;
    return TFHE_OK;
}

int tfhe_gpu_profile_end(tfhe_gpu_ctx *c, double *br_ms, double *ks_ms, int *launches) {
    if (!c) return TFHE_ERR_INVALID;
    return on_device0(c, [&](Device &d) -> int {
        d.profiling = false;
        const int rc = sync_check(d);
        if (rc) {
            d.ev_used = 0;
            return rc;
        }
        double br = 0.0, ks = 0.0;
        for (size_t i = 0; i + 3 <= d.ev_used; i += 3) {
            float a = 0.f, b = 0.f;
            HIPCHK(d, hipEventElapsedTime(&a, d.events[i], d.events[i + 1]));
            HIPCHK(d, hipEventElapsedTime(&b, d.events[i + 1], d.events[i + 2]));
            br += a;
            ks += b;
        }
        if (br_ms) *br_ms = br;
        if (ks_ms) *ks_ms = ks;
        if (launches) *launches = (int)(d.ev_used / 3);
        d.ev_used = 0;
        return TFHE_OK;
    });
}

int tfhe_gpu_fft_forward_batch(tfhe_gpu_ctx *c, const uint32_t *in, double *out, size_t B) {
    if (!c || (B && (!in || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) -> int {
        Frame f(d);
        Io io{f, /*dev*/ false};
        int rc = io.in(in, B * 1024 * 4);
        if (!rc) rc = io.out(out, B * 1024 * 8);
        if (rc) return rc;
        HIPCHK(d, launch_fft_forward(tables(d), in, out, B, d.stream));
        return io.finish();
    });
}

int tfhe_gpu_fft_inverse_batch(tfhe_gpu_ctx *c, const double *in, uint32_t *out, size_t B) {
    if (!c || (B && (!in || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) -> int {
        Frame f(d);
        Io io{f, /*dev*/ false};
        int rc = io.in(in, B * 1024 * 8);
        if (!rc) rc = io.out(out, B * 1024 * 4);
        if (rc) return rc;
        HIPCHK(d, launch_fft_inverse(tables(d), in, out, B, d.stream));
        return io.finish();
    });
}

int tfhe_gpu_poly_mul_batch(tfhe_gpu_ctx *c, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t B) {
    if (!c || (B && (!a || !b || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) -> int {
        Frame f(d);
        Io io{f, /*dev*/ false};
        int rc = io.in(a, B * 1024 * 4);
        if (!rc) rc = io.in(b, B * 1024 * 4);
        if (!rc) rc = io.out(out, B * 1024 * 4);
        if (rc) return rc;
        HIPCHK(d, launch_poly_mul(tables(d), a, b, 1024, out, B, d.stream));
        return io.finish();
    });
}

int tfhe_gpu_external_product_batch(tfhe_gpu_ctx *c, const double *trgsw_fft, uint32_t bk_index,
                                    const uint32_t *in, uint32_t *out, size_t B) {
    if (!c || (B && (!in || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    if (B == 0) return TFHE_OK;
    return on_device0(c, [&](Device &d) -> int {
        const size_t row_d = (size_t)2 * d.P.L * 2048;  // doubles per TRGSW
        const double *row = nullptr;
        Frame f(d);
        Io io{f, /*dev*/ false};
        int rc = TFHE_OK;
        if (trgsw_fft) {
            rc = io.in(trgsw_fft, row_d * 8);
            double *permuted = f.take<double>(row_d);
            if ((rc = f.rc())) return rc;
            HIPCHK(d, launch_bk_permute(d.K, trgsw_fft, permuted, 2 * d.P.L, d.stream));
            row = permuted;
            if (d.K.offset == 0) d.K.offset = decomposition_offset(d.P);  // no key loaded yet: the parameter set's
        } else {
            if (!d.has_key) return fail(d, TFHE_ERR_NO_KEY, "no cloud key loaded");
            if (bk_index >= d.P.n) return fail(d, TFHE_ERR_INVALID, "bk_index >= n");
            row = d.d_bk + (size_t)bk_index * row_d;
        }
        rc = io.in(in, B * 2048 * 4);
        if (!rc) rc = io.out(out, B * 2048 * 4);
        if (rc) return rc;
        HIPCHK(d, launch_external_product(d.K, tables(d), row, in, out, B, d.stream));
        return io.finish();
    });
}

}  // extern "C"

// ---- Options ------------------------------------------------------------------
namespace tfhe {

// Range check of one option value, before anything is applied to any device.
static bool option_ok(const Device &d, int key, int64_t v, std::string &why) {
    bool ok = false;
    switch (key) {
    case TFHE_OPT_BR_FORM:
        // 2 split, 4 pair: removed in round 4; 6 duo, 7 split-transform latency
        // form, 8 the whole form without loader assist, 30 the latency form with row
        // counters: A/B libraries only (tools/ab/); 5 octo: L = 1 only
        ok = v == 0 || (v == 1 && whole_form_packs((int)d.P.L, (int)d.P.bgbit)) || v == 3 || (v == 5 && d.P.L == 1) ||
             ((v == 6 || v == 7 || v == 8 || v == 30) && ab_forms_linked());
        if (!ok && v == 1)
            why = "TFHE_OPT_BR_FORM 1 (whole form) does not exist at L = 3 with 4*bgbit > 32: its packed tmp words "
                  "need bgbit <= 8; the latency form runs there";
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
    case TFHE_OPT_CMUX_FORM: ok = v >= 0 && v <= 2; break;
    case TFHE_OPT_PACK_SCRATCH_MB:
    case TFHE_OPT_SCATTER_SCRATCH_MB: ok = v >= 1 && v <= 256; break;
    case TFHE_OPT_GRAPH_CHUNK_QUERIES: ok = v >= 0 && v <= 0x7FFFFFFFll; break;
    case TFHE_OPT_TWIDDLES:
        ok = v == TFHE_TWIDDLES_GLIBC || v == TFHE_TWIDDLES_FDLIBM;
        // tfhe_gpu_keygen transformed the resident BK with the current tables:
        // other tables would no longer match it (a loaded reference key is data
        // and may be paired with either table)
        if (ok && d.key_from_keygen && v != d.twiddle_source) {
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

// Apply a checked option to one device.
static int apply_option(Device &d, int key, int64_t v) {
    LaunchOpts &o = d.opts;
    switch (key) {
    case TFHE_OPT_BR_FORM: o.br_form = (int)v; break;
    case TFHE_OPT_BR_LOADER: break;
    case TFHE_OPT_KS_FORM: o.ks_form = (int)v; break;
    case TFHE_OPT_KS_NARROW: o.ks_narrow = (int)v; break;
    case TFHE_OPT_KS_ITEM_GROUPS: o.ks_groups = (int)v; break;
    case TFHE_OPT_KS_SEL_ITEMS: o.ks_sel_items = (int)v; break;
    case TFHE_OPT_CIRCUIT_PACK: d.circuit_pack = v; break;
    case TFHE_OPT_TWIDDLES: return v == d.twiddle_source ? TFHE_OK : build_tables(d, (int)v);
    case TFHE_OPT_BR_SYNC: break;
    case TFHE_OPT_ARITH: o.arith_strict = v == TFHE_ARITH_REFERENCE ? 1 : v == TFHE_ARITH_FUSED_FORCED ? 2 : 0; break;
    case TFHE_OPT_BR_SPIN_CAP: d.K.spin_cap = (uint32_t)v; break;
    case TFHE_OPT_HOST_PIPELINE: d.pipeline = v; break;
    case TFHE_OPT_CMUX_FORM: o.cmux_form = (int)v; break;
    case TFHE_OPT_PACK_SCRATCH_MB: d.pack_scratch_mb = v; break;
    case TFHE_OPT_SCATTER_SCRATCH_MB: d.scatter_scratch_mb = v; break;
    case TFHE_OPT_GRAPH_CHUNK_QUERIES: d.graph_chunk_queries = v; break;
    case TFHE_OPT_HOST_STAGING:
        if (d.stage_used) HIPCHK(d, hipStreamSynchronize(d.stream));  // nothing in flight from the arena
        d.stage_used = 0;
        d.host_staging = v;
        break;
    default: return TFHE_ERR_INVALID;
    }
    return TFHE_OK;
}

}  // namespace tfhe

extern "C" {

// Validated once, then applied to every device (the circuit split is the handle's own).
int tfhe_gpu_set_option(tfhe_gpu_ctx *c, int key, int64_t v) {
    if (!c) return TFHE_ERR_INVALID;
    std::string why;
    if (!option_ok(c->dev[0], key, v, why)) return fail(c, TFHE_ERR_INVALID, why);
    if (key == TFHE_OPT_CIRCUIT_SPLIT) {
        c->circuit_split = v;
        return TFHE_OK;
    }
    for (size_t d = 0; d < c->dev.size(); d++)
        if (const int rc = apply_option(c->dev[d], key, v)) return lift(c, d, rc);
    return TFHE_OK;
}

int tfhe_gpu_get_option(const tfhe_gpu_ctx *c, int key, int64_t *v) {
    if (!c || !v) return TFHE_ERR_INVALID;
    const Device &d = c->dev[0];
    const LaunchOpts &o = d.opts;
    switch (key) {
    case TFHE_OPT_BR_FORM: *v = o.br_form; break;
    case TFHE_OPT_BR_LOADER: *v = 1; break;
    case TFHE_OPT_KS_FORM: *v = o.ks_form; break;
    case TFHE_OPT_KS_NARROW: *v = o.ks_narrow; break;
    case TFHE_OPT_KS_ITEM_GROUPS: *v = o.ks_groups; break;
    case TFHE_OPT_KS_SEL_ITEMS: *v = o.ks_sel_items; break;
    case TFHE_OPT_CIRCUIT_PACK: *v = d.circuit_pack; break;
    case TFHE_OPT_TWIDDLES: *v = d.twiddle_source; break;
    case TFHE_OPT_ARITH: *v = o.arith_strict == 1 ? TFHE_ARITH_REFERENCE : o.arith_strict == 2 ? TFHE_ARITH_FUSED_FORCED : TFHE_ARITH_AUTO; break;
    case TFHE_OPT_FUSED_ADMITTED: *v = o.key_fused_ok; break;
    case TFHE_OPT_LEVEL_ISSUE_US: *v = c->level_issue_us; break;
    case TFHE_OPT_KEY_ROW_RMS_PPM: *v = (int64_t)std::llround(d.bk_row_rms * 1e6); break;
    case TFHE_OPT_BR_SYNC: *v = 1; break;
    case TFHE_OPT_BR_SPIN_CAP: *v = d.K.spin_cap; break;
    case TFHE_OPT_HOST_PIPELINE: *v = d.pipeline; break;
    case TFHE_OPT_CIRCUIT_SPLIT: *v = c->circuit_split; break;
    case TFHE_OPT_HOST_STAGING: *v = d.host_staging; break;
    case TFHE_OPT_CMUX_FORM: *v = o.cmux_form; break;
    case TFHE_OPT_PACK_SCRATCH_MB: *v = d.pack_scratch_mb; break;
    case TFHE_OPT_SCATTER_SCRATCH_MB: *v = d.scatter_scratch_mb; break;
    case TFHE_OPT_GRAPH_CHUNK_QUERIES: *v = d.graph_chunk_queries; break;
    default: return TFHE_ERR_INVALID;
    }
    return TFHE_OK;
}

const char *tfhe_gpu_last_kernels(tfhe_gpu_ctx *c) {
    if (!c) return "";
    const Device &d = c->dev[0];
    c->last_kernels = d.last_br;
    if (d.last_ks && d.last_ks[0]) c->last_kernels += std::string(" + ") + d.last_ks;
    return c->last_kernels.c_str();
}

// ---- Contexts over several devices, and the batch entry points -----------------

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
    Handle c(new tfhe_gpu_ctx, tfhe_gpu_destroy);
    c->P = *params;
    c->multi = true;
    c->dev.reserve(devs.size());
    for (int d : devs) {
        c->dev.emplace_back();
        const int rc = init_device(c->dev.back(), *params, d);
        if (rc) return create_fail(rc, "tfhe_gpu_create: " + c->dev.back().err);
    }
    std::vector<int> sorted = devs;
    std::sort(sorted.begin(), sorted.end());
    c->distinct_devices = std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
    if (c->distinct_devices) {
        const int rc = enable_peer_access(devs, why);
        if (rc) return create_fail(rc, why);
    }
    *out = c.release();
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

int tfhe_gpu_num_devices(const tfhe_gpu_ctx *c) { return c ? (int)c->dev.size() : 0; }

int tfhe_gpu_near_tie_items(const tfhe_gpu_ctx *c, uint64_t *count) {
    if (!c || !count) return TFHE_ERR_INVALID;
    *count = 0;
    for (const Device &d : c->dev) *count += d.near_tie_items;
    return TFHE_OK;
}

int tfhe_gpu_device_bootstraps(const tfhe_gpu_ctx *c, uint64_t *counts, int max_devices) {
    if (!c || !counts || max_devices < 1) return TFHE_ERR_INVALID;
    const int D = (int)c->dev.size();
    for (int d = 0; d < D && d < max_devices; d++) counts[d] = c->dev[d].bootstraps;
    return D;
}

// The batch on the context's one device, or every device's slice of it.
static int host_batch(tfhe_gpu_ctx *c, const HostBatch &hb, size_t B) {
    if (!c || (B && !(hb.a && hb.out && (!hb.gate || (hb.ops && hb.b))))) return fail(c, TFHE_ERR_INVALID, "null argument");
    return for_each_slice(c, B, [&](Device &d, size_t, size_t first, size_t n) { return host_batch_on(d, hb, first, n); });
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
    if (!c || (B && (!in_lv1 || !out_lv0))) return fail(c, TFHE_ERR_INVALID, "null argument");
    const size_t w = tlwe0_words(c->P), wi = (size_t)c->P.N + 1;
    return for_each_slice(c, B, [&](Device &d, size_t, size_t first, size_t n) {
        return key_switch_on(d, in_lv1 + first * wi, out_lv0 + first * w, n);
    });
}

int tfhe_gpu_reenc_key_load(tfhe_gpu_ctx *c, const uint32_t *key_encryptions, size_t len, uint32_t basebit,
                            uint32_t t, tfhe_gpu_reenc_key **out) {
    if (!c || !key_encryptions || !out) return fail(c, TFHE_ERR_INVALID, "null argument");
    const size_t n = c->P.n, rows = n * t * ((size_t)1 << basebit);
    if (basebit < 1 || basebit > 8 || t < 1 || basebit * t >= 31 || !reencrypt_supported((int)t, (int)basebit))
        return fail(c, TFHE_ERR_INVALID, "unsupported re-encryption base/levels");
    if (len != rows * (n + 1)) return fail(c, TFHE_ERR_INVALID, "len != n*t*2^basebit*(n+1)");
    std::unique_ptr<tfhe_gpu_reenc_key> k(new tfhe_gpu_reenc_key);
    k->basebit = basebit;
    k->t = t;
    k->dev.resize(c->dev.size());
    for (size_t d = 0; d < c->dev.size(); d++)  // one upload per device (host -> each HBM)
        if (const int rc = reenc_key_upload(c->dev[d], key_encryptions, basebit, t, k->dev[d])) return lift(c, d, rc);
    *out = k.release();
    return TFHE_OK;
}

void tfhe_gpu_reenc_key_destroy(tfhe_gpu_reenc_key *k) {
    if (!k) return;
    while (!k->dev.empty()) k->dev.pop_back();  // last to first, like a context's devices
    delete k;
}

int tfhe_gpu_reencrypt_batch(tfhe_gpu_ctx *c, const tfhe_gpu_reenc_key *k, const uint32_t *in, uint32_t *out,
                             size_t B) {
    if (!c || !k || (B && (!in || !out))) return fail(c, TFHE_ERR_INVALID, "null argument");
    // a context of one device takes any key's first copy (on the same device: reencrypt_on)
    if (is_multi(c) && k->dev.size() != c->dev.size()) return fail(c, TFHE_ERR_INVALID, "key was not loaded on this context");
    const size_t w = tlwe0_words(c->P);
    return for_each_slice(c, B, [&](Device &d, size_t slot, size_t first, size_t n) {
        return reencrypt_on(d, *k, slot, in + first * w, out + first * w, n);
    });
}

int tfhe_gpu_reencrypt_batch_dev(tfhe_gpu_ctx *c, const tfhe_gpu_reenc_key *k, const uint32_t *in_dev,
                                 uint32_t *out_dev, size_t B) {
    if (is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (!c || !k || (B && (!in_dev || !out_dev))) return fail(c, TFHE_ERR_INVALID, "null argument");
    return lift(c, 0, reencrypt_on(c->dev[0], *k, 0, in_dev, out_dev, B, true));
}

static bool circuit_args_ok(size_t n_inputs, const uint32_t *inputs, size_t n_gates, const uint8_t *ops,
                            const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires,
                            const uint32_t *outputs) {
    return (!n_inputs || inputs) && (!n_gates || (ops && in_a && in_b)) && (!n_outputs || (out_wires && outputs));
}

int tfhe_gpu_circuit_eval_dev(tfhe_gpu_ctx *c, size_t n_inputs, const uint32_t *inputs_dev, size_t n_gates,
                              const uint8_t *ops, const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs,
                              const uint32_t *out_wires, uint32_t *outputs_dev, uint32_t *levels) {
    if (is_multi(c)) return fail(c, TFHE_ERR_INVALID, "device-resident calls take a single-device context");
    if (!c || !circuit_args_ok(n_inputs, inputs_dev, n_gates, ops, in_a, in_b, n_outputs, out_wires, outputs_dev))
        return fail(c, TFHE_ERR_INVALID, "null argument");
    return lift(c, 0, circuit_eval_one(c->dev[0], n_inputs, inputs_dev, n_gates, ops, in_a, in_b, n_outputs, out_wires,
                                       outputs_dev, levels, true));
}

int tfhe_gpu_circuit_eval(tfhe_gpu_ctx *c, size_t n_inputs, const uint32_t *inputs, size_t n_gates, const uint8_t *ops,
                          const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs, const uint32_t *out_wires,
                          uint32_t *outputs, uint32_t *levels) {
    if (!c || !circuit_args_ok(n_inputs, inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires, outputs))
        return fail(c, TFHE_ERR_INVALID, "null argument");
    if (!is_multi(c))
        return lift(c, 0, circuit_eval_one(c->dev[0], n_inputs, inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires,
                                           outputs, levels));
    return circuit_eval_multi(c, n_inputs, inputs, n_gates, ops, in_a, in_b, n_outputs, out_wires, outputs, levels);
}

}  // extern "C"
