/*
 * tfhe_gpu.h — C ABI of the MI355X TFHE gate-bootstrap engine.
 *
 * This is the drop-in boundary for zig-tfhe's bootstrap strategy plug point
 * (src/bootstrap.zig:30-47, src/bootstrap/vanilla.zig:38-69, callers
 * src/gates.zig:48-129).  A Zig `bootstrap/hip.zig` strategy would declare
 * these functions `extern fn` and map a negative status to a Zig error
 * (INTEGRATION.md shows the binding).  Plain pointers and sizes only; the
 * library owns all device memory; one context = one HIP device (+ one stream).
 *
 * Layouts are the reference's in-memory layouts:
 *   TLWELv0      = uint32_t[n+1]            (tlwe.zig:11-12, b is the last word)
 *   TLWELv1      = uint32_t[N+1]            (tlwe.zig:243-244)
 *   TRLWELv1     = uint32_t[2][N]  a then b (trlwe.zig:15-17)
 *   BootstrappingKey  = double[n][2L][2][N] (key.zig:31, trgsw.zig:75-77,
 *                        trlwe.zig:104-106: each N = re[N/2] ++ im[N/2])
 *   KeySwitchingKey   = uint32_t[N*t*2^basebit][n+1]  (key.zig:28, :148-172)
 * Status: 0 = OK, negative = error (tfhe_gpu_last_error has the text).
 * Calls on one context are serialised by the caller (as the reference's
 * single-threaded Gates); distinct contexts are independent.
 */
#ifndef TFHE_GPU_H
#define TFHE_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFHE_GPU_ABI_VERSION 7  /* 7: tfhe_gpu_set_stream(NULL) = the null stream, tfhe_gpu_reset_stream; later
                                   additions that change no existing entry keep the number: the leveled
                                   entries (TRLWE / TRGSW encryption, selector sets, CMUX, table lookup,
                                   sample extraction, tfhe_lookup_table_pack_bits), TFHE_OPT_CMUX_FORM, the
                                   LUT-circuit entries (LUT sets, tfhe_gpu_lut_apply_*, tfhe_gpu_lut_circuit_eval*,
                                   tfhe_lut_circuit_schedule) and the packed lookup (tfhe_gpu_rotate_by_bits_*,
                                   tfhe_gpu_packed_lookup_*, tfhe_packed_lookup_plan, tfhe_lookup_table_pack_slots)
                                   and the packing key switch (tfhe_gpu_packing_key_*, tfhe_gpu_pack_tlwe_*,
                                   tfhe_pack_tlwe, TFHE_OPT_PACK_SCRATCH_MB) and the multi-output LUT bootstrap
                                   (tfhe_lut_round_tlwe, tfhe_lut_interleave, tfhe_gpu_lut_apply_multi_*,
                                   tfhe_gpu_lut_circuit_eval_multi*, tfhe_lut_circuit_schedule_multi) and the
                                   packed scatter-add (tfhe_gpu_packed_scatter_add_*, TFHE_OPT_SCATTER_SCRATCH_MB)
                                   and the bivariate LUT bootstrap (tfhe_lut_spread, tfhe_gpu_lut_spread_*,
                                   tfhe_gpu_bootstrap_lut_each_*, tfhe_gpu_lut_apply2_*) and the CMUX graphs
                                   (tfhe_cmux_graph_plan, tfhe_gpu_cmux_graph_*, TFHE_OPT_GRAPH_CHUNK_QUERIES)
                                   and the select nodes (tfhe_gpu_lut_circuit_eval_select*, tfhe_gpu_lut_select_*,
                                   tfhe_lut_circuit_schedule_select, TFHE_LUT_ENTRY_CONST) and the extended LUT
                                   bootstrap (tfhe_lut_generate_ext, tfhe_lut_ext_rotate, tfhe_lut_ext_mod_switch,
                                   tfhe_gpu_blind_rotate_ext_batch, tfhe_gpu_lut_apply_ext_*);
                                   6: tfhe_gpu_build_kind, tfhe_lut_generate_scaled / _full; BR forms 6-40
                                   A/B-only, BR_LOADER / BR_SYNC = 1 only;
                                   5: _dev LUT / re-encryption / circuit entries; BR forms 2 and 4 removed */

enum {
    TFHE_OK = 0,
    TFHE_ERR_INVALID = -1,     /* bad argument / unsupported parameter set      */
    TFHE_ERR_HIP = -2,         /* HIP runtime error (no device, launch failure) */
    TFHE_ERR_NO_KEY = -3,      /* bootstrap requested before a cloud key loaded */
    TFHE_ERR_OOM = -4,         /* device allocation failed                      */
    TFHE_ERR_IO = -5,          /* key file cannot be opened, read or written    */
    TFHE_ERR_DEVICE = -6       /* a kernel reported a failure through the context's device
                                  error word (the blind rotation's BK-slot protocol: a wait
                                  timed out); the outputs since the last synchronisation are
                                  invalid; the word is cleared and the context stays usable */
};

/* Gate op codes — gates.zig:48-121 (pre-combination constants SURVEY §8a A2). */
enum {
    TFHE_GATE_NAND = 0, TFHE_GATE_OR = 1, TFHE_GATE_AND = 2, TFHE_GATE_XOR = 3,
    TFHE_GATE_XNOR = 4, TFHE_GATE_NOR = 5, TFHE_GATE_ANDNY = 6, TFHE_GATE_ANDYN = 7,
    TFHE_GATE_ORNY = 8, TFHE_GATE_ORYN = 9,
    TFHE_GATE_NOT = 254,       /* circuits only: negation, no bootstrap (gates.zig:132-135) */
    TFHE_GATE_COPY = 255       /* no pre-combination: bootstrap input a as is */
};

/* Runtime form of params.zig SecurityParams (:36-67).  N must be 1024.
 * The parameter check (every tfhe_gpu_create*, and the host-only calls that take params): N = 1024,
 * nbit = 10, n in [1, 1024], L in {1, 2, 3}, bgbit in [1, 31] with L * bgbit <= 32, and a key switch
 * of basebit 2 with 7..9 levels or basebit 3..8 with 2..4 levels, basebit * iks_t < 31.  Anything
 * else: TFHE_ERR_INVALID, the reason in tfhe_gpu_last_error(NULL) after a create.
 *  - bgbit = 32 (L = 1) is refused: Bg = 2^32 does not fit the 32-bit words the decomposition offset
 *    and the digit mask are computed in (1u << 32 is undefined), and the device's bit-field extract
 *    reads a width of 32 as 0.
 *  - L = 1 with bgbit 29..31 is accepted, but the values the external product rounds (typically around
 *    2^(34 + bgbit) under a generated key; at most 2 N Bg/2 2^31) reach 2^63 there, beyond the i64
 *    range of the reference's @intFromFloat: the reference's result is undefined at such values and
 *    this library reproduces the x86-64 behaviour (low word 0; torus_from_f64, tfhe_device.hpp), so
 *    parity with the reference is platform-defined in that region.
 *  - L = 3 with bgbit 9 or 10 (4 * bgbit > 32) has no whole-form blind rotation: every batch runs the
 *    latency form, and TFHE_OPT_BR_FORM 1 is refused. */
typedef struct {
    uint32_t n;        /* TLWE lv0 dimension (tlwe_lv0.n)   */
    uint32_t N;        /* polynomial size (trgsw_lv1.n)     */
    uint32_t nbit;     /* log2 N                             */
    uint32_t L;        /* gadget levels                      */
    uint32_t bgbit;    /* log2 Bg                            */
    uint32_t basebit;  /* key-switch base bits               */
    uint32_t iks_t;    /* key-switch levels                  */
    uint32_t _pad;
    double alpha_lv0;  /* tlwe_lv0.alpha                     */
    double alpha_lv1;  /* trlwe_lv1.alpha                    */
    double alpha_ksk;  /* KSK_ALPHA (params.zig:419-420)     */
    double alpha_bsk;  /* BSK_ALPHA (params.zig:421-422)     */
} tfhe_params;

typedef struct tfhe_gpu_ctx tfhe_gpu_ctx;

int         tfhe_gpu_abi_version(void);
/* TFHE_BUILD_PRODUCT for the product library; TFHE_BUILD_AB for a development
 * build (knock-out, timing or losing-form variants: tools/ab_forms.sh,
 * tools/libvar_build.sh, a Makefile EXTRA), which every tfhe_gpu_create*
 * refuses (TFHE_ERR_INVALID) unless the environment sets
 * TFHE_ALLOW_AB_BUILD=1.  (ABI 6) */
enum { TFHE_BUILD_PRODUCT = 0, TFHE_BUILD_AB = 1 };
int         tfhe_gpu_build_kind(void);
/* 16 hex digits of the sha256 of the kernels object this library was linked
 * from (its gfx950 code): measurements (PMC records) are tagged with it. */
const char *tfhe_gpu_build_id(void);
/* Context over HIP devices 0..num_devices-1 of this node:
 * num_devices = 1 is a plain single-device context on device 0, more is the
 * multi-device context of tfhe_gpu_create_multi below.  Replaces the implicit
 * per-thread FFT plan (fft.zig:983-992) and owns the device copy of the
 * CloudKey.  TFHE_ERR_HIP if the node has fewer devices. */
int         tfhe_gpu_create(const tfhe_params *params, int num_devices, tfhe_gpu_ctx **out);
/* Context on the one HIP device `device` (ABI 2's tfhe_gpu_create). */
int         tfhe_gpu_create_on_device(const tfhe_params *params, int device, tfhe_gpu_ctx **out);
void        tfhe_gpu_destroy(tfhe_gpu_ctx *ctx);
/* Text of the context's last failure; with ctx = NULL, the calling thread's
 * last failed tfhe_gpu_create / _create_on_device / _create_multi (ABI 4). */
const char *tfhe_gpu_last_error(const tfhe_gpu_ctx *ctx);
/* Wait for the context's work; TFHE_ERR_DEVICE if a kernel set the device
 * error word since the last synchronisation.  Every host-buffer entry point
 * performs the same check before it returns; after the asynchronous _dev
 * entry points, this (or tfhe_gpu_profile_end) is where a failure surfaces. */
int         tfhe_gpu_sync(tfhe_gpu_ctx *ctx);
/* Run this context's work on a caller-owned hipStream_t of its device; NULL is
 * that device's null stream (torch's default stream has handle 0).  The new
 * stream first waits for everything queued on the old one.  (ABI 7: before,
 * NULL meant the context's own stream, so torch's default stream silently got
 * an unordered non-blocking stream.)  Multi-device context: its first device. */
int         tfhe_gpu_set_stream(tfhe_gpu_ctx *ctx, void *hip_stream);
/* Back to the context's own (non-blocking) stream, ordered after the current one.  (ABI 7) */
int         tfhe_gpu_reset_stream(tfhe_gpu_ctx *ctx);

/* ---- Multi-device context (bootstrap.zig:30-47 strategy over
 * the 8 GPUs of one node) ---------------------------------------------------
 * One context over `num_devices` HIP devices (`devices` = their ids, NULL =
 * 0..num_devices-1).  Key loads (load_cloud_key, keygen, the key file and
 * device-blob imports) land on the first device and are broadcast once to
 * the others with ncclBroadcast over RCCL (xGMI; librccl is loaded at that
 * point); a device listed twice (a test of the sharding on one GPU) gets a
 * device-to-device copy instead.  The host-buffer batch entry points
 * (bootstrap / gate / blind-rotate / LUT / key-switch / re-encryption) split
 * the batch into contiguous slices of ceil(B/num_devices) items, one per
 * device, run them concurrently (one host thread and one stream per device)
 * and copy each slice's results into the caller's buffer; circuit_eval
 * replicates the primary inputs to every device that reads them and places
 * the connected components of the gate DAG (gates joined by gate-to-gate
 * wires) on the devices, largest first onto the least-loaded device, so no
 * gate output crosses a device; when one component dominates it splits every
 * level's gates over the devices instead and all-gathers each level's outputs
 * (peer copies over xGMI) before the next (TFHE_OPT_CIRCUIT_SPLIT).  Device-pointer
 * (_dev) and stage entry points and the profile timers use the first device.
 * Nothing is exchanged between devices after the key broadcast. */
/* Distinct devices must reach each other's memory: create_multi checks
 * hipDeviceCanAccessPeer for every ordered pair and enables peer access (the
 * level split's peer copies then go over xGMI, not through the host); a pair
 * without it fails the create with TFHE_ERR_DEVICE and the pair named in
 * tfhe_gpu_last_error(NULL).  A device id the node does not have fails with
 * TFHE_ERR_HIP. */
int tfhe_gpu_create_multi(const tfhe_params *params, int num_devices, const int *devices, tfhe_gpu_ctx **out);
int tfhe_gpu_num_devices(const tfhe_gpu_ctx *ctx);
/* 64-bit fingerprints of the resident device key (BK and KSK in the device
 * layout; the order-independent k_checksum sum, ~35 us each), the values the
 * multi-device broadcast compares.  Processes that import a broadcast key
 * (tfhe_gpu_import_key_device) compare them across ranks (tfhe_dist.py).
 * TFHE_ERR_NO_KEY without a key.  (ABI 4) */
int tfhe_gpu_key_fingerprint(tfhe_gpu_ctx *ctx, uint64_t *bk, uint64_t *ksk);
/* Blind rotations each device of the context has launched since it was
 * created (counts[d] for device d < max_devices, in create order); returns the
 * number of devices.  Shows where a sharded batch or circuit ran. */
int tfhe_gpu_device_bootstraps(const tfhe_gpu_ctx *ctx, uint64_t *counts, int max_devices);
/* Items whose blind rotation the fused arithmetic's margin guard sent to the
 * reference-tree recompute since the context was created (a value 1/4 or
 * more off its integer), as of the last synchronisation. */
int tfhe_gpu_near_tie_items(const tfhe_gpu_ctx *ctx, uint64_t *count);

/* ---- Options (kernel forms and table sources; default = the measured-
 * fastest forms).  Set on a context before use; a multi-device context
 * passes them to every device.  TFHE_ERR_INVALID for an unknown key or value. */
enum {
    TFHE_OPT_BR_FORM = 1,         /* blind rotation: 0 auto (default), 1 whole (refused at L = 3 with
                                     4 * bgbit > 32, where it does not exist), 3 latency, 5 octo (8 items
                                     per workgroup, two gate waves per SIMD; L = 1 only).  2 split and 4
                                     pair were removed in round 4; 6 duo, 7 the split-transform latency
                                     form, 8 round 4's whole form and 9-40 development copies of the L = 3
                                     whole form (all measured slower) exist
                                     only in A/B libraries since round 5 (tools/ab/): TFHE_ERR_INVALID here */
    TFHE_OPT_BR_LOADER = 2,       /* whole form: 1 loader waves issue the BK DMAs (the only value since
                                     round 5; 0, the gate waves issuing them, was removed) */
    TFHE_OPT_KS_FORM = 3,         /* key switch: 3 auto (default: the one-hot GEMM on the matrix
                                     cores for basebit 2 and 5, else lanes), 0 lanes / ring,
                                     1 select / gather, 2 the GEMM at any batch (basebit 2; other
                                     parameter sets fall back to lanes) */
    TFHE_OPT_KS_NARROW = 4,       /* basebit 2: 0 auto (default), 1 32-word x 4-wave blocks */
    TFHE_OPT_KS_ITEM_GROUPS = 5,  /* basebit >= 5: 0 auto (above 64 items the ring form: 4 item groups
                                     share a 4-deep DMA ring), 1, 2, 4, 8 forces the lane form with
                                     that many item groups per block */
    TFHE_OPT_KS_SEL_ITEMS = 6,    /* select / gather form: items per block, 8 (default), 16, 32; any other
                                     value is refused (TFHE_ERR_INVALID) and the option keeps its value.
                                     tfhe_gpu_last_kernels names k_key_switch_sel / _gather at 8 and
                                     k_key_switch_sel<t,16>, <t,32> (_gather alike) at the others */
    TFHE_OPT_CIRCUIT_PACK = 7,    /* circuit_eval round packing: 1 (default), 0 off */
    TFHE_OPT_TWIDDLES = 8,        /* cos/sin source of the FFT tables: TFHE_TWIDDLES_* (set before a key
                                     is generated: keygen transforms the key with these tables) */
    TFHE_OPT_ARITH = 9,           /* blind-rotation f64 arithmetic: TFHE_ARITH_* */
    TFHE_OPT_BR_SYNC = 10,        /* whole form: 1 per-slot LDS counters (gate waves wait for their data,
                                     not for each other; the only value since round 5: 0, a workgroup
                                     barrier per BK row pair, was removed) */
    TFHE_OPT_BR_SPIN_CAP = 11,    /* polls before one slot-counter wait gives up and sets the device
                                     error word (0 = default, 2^22 sleep units; fault-injection tests
                                     set a few polls to see TFHE_ERR_DEVICE come back) */
    TFHE_OPT_HOST_PIPELINE = 12,  /* host-buffer bootstrap / gate / LUT batches of >= 4 x #CUs items:
                                     0 (default) one H2D -> kernels -> D2H sequence, 1 chunked through
                                     pinned staging on 4 streams (measured slower on the MI355X box,
                                     whose pageable copies run at ~50 GB/s: DESIGN.md §2.1) */
    TFHE_OPT_CIRCUIT_SPLIT = 13,  /* multi-device circuit_eval: 0 auto (default: connected components
                                     on devices, or by levels when one component dominates), 1
                                     components, 2 levels (each level's gates split over the devices,
                                     outputs all-gathered by peer copies before the next level) */
    TFHE_OPT_FUSED_ADMITTED = 14, /* read-only (get_option): 1 if the resident cloud key passed the fused
                                     arithmetic's admission check at load (largest BK spectrum component
                                     <= 2^39 and every TRGSW row's RMS <= 0.65 x 2^31), 0
                                     if it was refused and TFHE_ARITH_AUTO runs the reference's expression
                                     trees for it */
    TFHE_OPT_LEVEL_ISSUE_US = 15, /* read-only: host microseconds the last level-split circuit_eval spent
                                     issuing its per-level launches, peer copies and event waits (one
                                     host thread for all devices) */
    TFHE_OPT_KEY_ROW_RMS_PPM = 16, /* read-only: the resident key's largest TRGSW row RMS / 2^31, in
                                     millionths (the admission's row-energy rule admits <= 650000;
                                     keygen'd keys ~600000; ABI 6) */
    TFHE_OPT_HOST_STAGING = 17,   /* host-buffer copies: 0 pageable hipMemcpyAsync from / to the caller's buffers
                                     (default), 1 through per-device pinned staging (host memcpy + DMA).  Same
                                     words either way.  Measured: 8 concurrent shards'
                                     pageable copies 52.9 GB/s in total against 47.2 staged, and the one-card
                                     8-shard step 54.5 vs 56.6 ms, so staging is for hosts whose pageable
                                     copies serialise */
    TFHE_OPT_CMUX_FORM = 18,      /* table lookup's CMUX levels: 0 auto (default: the measured-faster form, which
                                     is 2: 4.8 vs 9.6 ms per 1,024 lookups of a 256-entry table, DESIGN.md
                                     §4.8), 1 one wavefront per CMUX, each reading its selector from L2, 2 where
                                     a level has >= 4 pairs per query, workgroups of 4 CMUXes that stage their
                                     shared selector's rows in LDS once.  Same words either way;
                                     tfhe_gpu_last_kernels names what the last lookup ran */
    TFHE_OPT_PACK_SCRATCH_MB = 19,/* packing key switch: bound in MB on the context scratch that holds a chunk's
                                     GEMM sums, 1..256 (default 256).  Same words at any value; tests lower it to
                                     run a small batch in several chunks */
    TFHE_OPT_SCATTER_SCRATCH_MB = 20,/* packed scatter-add: bound in MB on the context scratch that holds a chunk's
                                     leaves, 1..256 (default 256): max(1, bound / (2^v * 8 KB)) queries per chunk.
                                     Same words at any value; tests lower it to run a small batch in several
                                     chunks */
    TFHE_OPT_GRAPH_CHUNK_QUERIES = 21 /* CMUX graphs: 0 (default) as many queries per chunk as keep their slots
                                     (n_slots * 8 KB each) within 256 MB of context scratch; 1 .. 2^31-1: at most
                                     that many as well.  Same words at any value; tests lower it to run a small
                                     batch in several chunks */
};
enum { TFHE_STAGING_PAGEABLE = 0, TFHE_STAGING_PINNED = 1 };  /* TFHE_OPT_HOST_STAGING */
/* TFHE_ARITH_AUTO (default): at the L=3 / Bg=2^6 sets the blind rotation
 * runs fused multiply-adds in the reference's operation order, with a margin
 * guard: every value it rounds must lie within 1/4 of an integer; an item
 * that rounded anything further off is recomputed in the reference's
 * expression trees in the same stream (tfhe_gpu_near_tie_items counts them).
 * Both round to the same integers while the fused and the reference's values
 * differ by less than 1/4: an EMPIRICAL bound (measured max 0.094 on keygen'd
 * keys), so a key is admitted to the fused arithmetic only
 * when its BK lies in the measured regime (TFHE_OPT_FUSED_ADMITTED); other
 * keys run the reference's trees.  UINT4: the reference's trees.
 * TFHE_ARITH_REFERENCE: the reference's expression trees everywhere.
 * TFHE_ARITH_FUSED_FORCED: fused (with the guard) even on a refused key —
 * for tests of the margin guard only. */
enum { TFHE_ARITH_AUTO = 0, TFHE_ARITH_REFERENCE = 1, TFHE_ARITH_FUSED_FORCED = 2 };
/* The two libm candidates a Zig build of the reference can bind @cos/@sin to
 * (fft.zig:98-106, :591-593): glibc (linkLibC on Linux) or Zig's compiler_rt
 * port of the fdlibm/musl kernels.  DESIGN.md §6 lists the entries where the
 * two tables differ. */
enum { TFHE_TWIDDLES_GLIBC = 0, TFHE_TWIDDLES_FDLIBM = 1 };
int tfhe_gpu_set_option(tfhe_gpu_ctx *ctx, int key, int64_t value);
int tfhe_gpu_get_option(const tfhe_gpu_ctx *ctx, int key, int64_t *value);
/* Names of the kernels the last bootstrap launch of this context ran
 * ("<blind rotation> + <key switch>"; first device of a multi-device context). */
const char *tfhe_gpu_last_kernels(tfhe_gpu_ctx *ctx);
/* The FFT constant tables for N (twist N/2 entries, forward stage twiddles
 * N/2-1 entries, fft.zig:92-106 and :590-616) from `source`; host only. */
int tfhe_fft_tables(uint32_t N, int source, double *twist_re, double *twist_im, double *stage_re,
                    double *stage_im);

/* ---- Cloud key (key.zig:61-118) -------------------------------------- */
/* Upload a CloudKey held in host memory in the reference layout
 * (CloudKey.decomposition_offset, .blind_rotate_testvec, .bootstrapping_key
 * .items, .key_switching_key.items).  bsk_len / ksk_len are element counts. */
int tfhe_gpu_load_cloud_key(tfhe_gpu_ctx *ctx, uint32_t decomposition_offset,
                            const uint32_t *testvec_a, const uint32_t *testvec_b,
                            const double *bsk, size_t bsk_len,
                            const uint32_t *ksk, size_t ksk_len);
/* Generate SecretKey.new (key.zig:41-57) + CloudKey.new (key.zig:70-77) with
 * a seeded RNG (Zig DefaultPrng restated; `seed` replaces getUniqueSeed()),
 * FFTs on the device, and load it.  key_lv0/key_lv1 receive the secret key
 * (n / N words); bsk_out / ksk_out (may be NULL) receive the host copy in the
 * reference layout. */
int tfhe_gpu_keygen(tfhe_gpu_ctx *ctx, uint64_t secret_seed, uint64_t cloud_seed,
                    uint32_t *key_lv0, uint32_t *key_lv1, double *bsk_out, uint32_t *ksk_out);
/* Device-resident key blob, for the one-time RCCL broadcast across ranks:
 * export copies the context's device key into caller device buffers of the
 * reported sizes; import loads a blob another context exported. */
int tfhe_gpu_key_blob_bytes(const tfhe_gpu_ctx *ctx, size_t *bsk_bytes, size_t *ksk_bytes);
int tfhe_gpu_export_key_device(tfhe_gpu_ctx *ctx, void *bsk_dev, void *ksk_dev,
                               uint32_t *decomposition_offset, uint32_t *testvec /*2N host*/);
int tfhe_gpu_import_key_device(tfhe_gpu_ctx *ctx, const void *bsk_dev, const void *ksk_dev,
                               uint32_t decomposition_offset, const uint32_t *testvec /*2N host*/);
/* The loaded CloudKey back in the reference's host layout (the inverse of
 * tfhe_gpu_load_cloud_key; bsk: n*2L*2*N doubles, ksk: N*t*2^basebit*(n+1)
 * words, the never-read k = 0 slots as zeros).  NULL outputs are skipped. */
int tfhe_gpu_export_cloud_key(tfhe_gpu_ctx *ctx, uint32_t *decomposition_offset, uint32_t *testvec_a,
                              uint32_t *testvec_b, double *bsk, uint32_t *ksk);

/* ---- Cloud-key files (SURVEY §5 checkpoint row, §8f N3) -----------------
 * The reference has no key serialization: every process regenerates its
 * CloudKey (key.zig:70-77, ~30 s on a CPU).  A key file is a 64-byte header
 * {char magic[8] = "ZTFHECK1"; u32 version = 1, n, N, L, bgbit, basebit,
 * iks_t, decomposition_offset; u64 bsk_len, ksk_len, checksum} followed by
 * testvec a (N u32), testvec b (N u32), the BootstrappingKey (bsk_len f64)
 * and the KeySwitchingKey (ksk_len u32), all little-endian in the layouts
 * above.  checksum = FNV-1a-64 over the four sections in 8-byte words.
 * Reading checks the magic, the parameter set against `params` and the
 * checksum (TFHE_ERR_INVALID); TFHE_ERR_IO: cannot open, short read/write. */
int tfhe_cloud_key_write(const char *path, const tfhe_params *params, uint32_t decomposition_offset,
                         const uint32_t *testvec_a, const uint32_t *testvec_b, const double *bsk, size_t bsk_len,
                         const uint32_t *ksk, size_t ksk_len);
int tfhe_cloud_key_read(const char *path, const tfhe_params *params, uint32_t *decomposition_offset,
                        uint32_t *testvec_a, uint32_t *testvec_b, double *bsk, size_t bsk_len, uint32_t *ksk,
                        size_t ksk_len);
/* Export + write, and read + load, for a context (host memory for one key). */
int tfhe_gpu_save_cloud_key(tfhe_gpu_ctx *ctx, const char *path);
int tfhe_gpu_load_cloud_key_file(tfhe_gpu_ctx *ctx, const char *path);

/* ---- Bootstrap / gates (host buffers, synchronous) ---------------------- */
/* VanillaBootstrap.bootstrap (vanilla.zig:38-52) over B TLWELv0. */
int tfhe_gpu_bootstrap_batch(tfhe_gpu_ctx *ctx, const uint32_t *in, uint32_t *out, size_t B);
/* VanillaBootstrap.bootstrapWithoutKeySwitch (vanilla.zig:58-69): blind
 * rotation + sampleExtractIndex2(acc, 0) (trlwe.zig:165-180), n+1 words per
 * item in the reference's hybrid form (p[0]=a[0], p[i]=-a[n-i], p[n]=b[0]). */
int tfhe_gpu_bootstrap_without_key_switch_batch(tfhe_gpu_ctx *ctx, const uint32_t *in, uint32_t *out,
                                                size_t B);
/* Gates.*Gate (gates.zig:48-121): per-item op + pre-combination + bootstrap. */
int tfhe_gpu_gate_batch(tfhe_gpu_ctx *ctx, const uint8_t *ops, const uint32_t *a,
                        const uint32_t *b, uint32_t *out, size_t B);
/* trgsw.blindRotate (trgsw.zig:290-333) / blindRotateWithTestvec (:336-400):
 * testvec = NULL uses the cloud key's; out = B TRLWELv1. */
int tfhe_gpu_blind_rotate_batch(tfhe_gpu_ctx *ctx, const uint32_t *in, const uint32_t *testvec,
                                uint32_t *trlwe_out, size_t B);
/* Programmable bootstrap: blindRotateWithTestvec + sampleExtractIndex(0) +
 * identityKeySwitching with a LUT test vector (lut/generator.zig:85-135). */
int tfhe_gpu_bootstrap_lut_batch(tfhe_gpu_ctx *ctx, const uint32_t *in, const uint32_t *testvec,
                                 uint32_t *out, size_t B);

/* ---- Circuits: level-scheduled gate DAG ----------------
 * Replaces gate-by-gate evaluation of a circuit (examples/add_two_numbers.zig:
 * 24-73, Gates.muxNaive gates.zig:124-129).  Wires 0..n_inputs-1 are the
 * inputs (TLWELv0 each); gate g drives wire n_inputs+g from wires in_a[g],
 * in_b[g] (both < n_inputs+g; in_b ignored for NOT/COPY).  ops: TFHE_GATE_*
 * (bootstrapped) or TFHE_GATE_NOT (free).  Each dependency level is one
 * batched bootstrap launch; every wire stays in HBM.  Gates with slack may
 * run one level later than their earliest level when that avoids a ragged
 * partial round (depth unchanged; TFHE_OPT_CIRCUIT_PACK = 0 disables it).
 * outputs receives the n_outputs wires out_wires[]; *levels (may be NULL)
 * the bootstrap depth. */
int tfhe_gpu_circuit_eval(tfhe_gpu_ctx *ctx, size_t n_inputs, const uint32_t *inputs, size_t n_gates,
                          const uint8_t *ops, const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs,
                          const uint32_t *out_wires, uint32_t *outputs, uint32_t *levels);
/* The same with the inputs and outputs in HBM (the circuit itself, ops / in_a /
 * in_b / out_wires, stays a host description), single-device contexts, async on
 * the context stream (tfhe_gpu_sync reports device errors). */
int tfhe_gpu_circuit_eval_dev(tfhe_gpu_ctx *ctx, size_t n_inputs, const uint32_t *inputs_dev, size_t n_gates,
                              const uint8_t *ops, const uint32_t *in_a, const uint32_t *in_b, size_t n_outputs,
                              const uint32_t *out_wires, uint32_t *outputs_dev, uint32_t *levels);

/* The schedule tfhe_gpu_circuit_eval runs, host only (no device): levels[g]
 * = the level gate g runs at (NOT: the level of its input), *depth (may be
 * NULL) = the bootstrap depth, for a device with `cus` compute units (256 on
 * the MI355X), with round packing when pack != 0. */
int tfhe_circuit_schedule(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                          const uint32_t *in_b, uint32_t cus, int pack, uint32_t *levels, uint32_t *depth);

/* The device placement a multi-device tfhe_gpu_circuit_eval uses, host only:
 * device_of_gate[g] < num_devices.  Gates joined by gate-to-gate wires share a
 * device; primary inputs are replicated and join nothing. */
int tfhe_circuit_partition(size_t n_inputs, size_t n_gates, const uint8_t *ops, const uint32_t *in_a,
                           const uint32_t *in_b, int num_devices, uint32_t *device_of_gate);

/* ---- Proxy re-encryption (proxy_reenc.zig) -------------
 * reencryptTLWELv0 is the identity key switch over a TLWELv0 input (n
 * coefficients instead of N), so it runs on the same lane-per-item kernel.
 * The key is ProxyReencryptionKey.key_encryptions: n*t*2^basebit TLWELv0 at
 * index (2^basebit*t*i) + (2^basebit*j) + k (proxy_reenc.zig:150-196). */
typedef struct tfhe_gpu_reenc_key tfhe_gpu_reenc_key;
int  tfhe_gpu_reenc_key_load(tfhe_gpu_ctx *ctx, const uint32_t *key_encryptions, size_t len /* words */,
                             uint32_t basebit, uint32_t t, tfhe_gpu_reenc_key **out);
void tfhe_gpu_reenc_key_destroy(tfhe_gpu_reenc_key *key);
int  tfhe_gpu_reencrypt_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_reenc_key *key, const uint32_t *in,
                              uint32_t *out, size_t B);

/* ---- Same, on device-resident buffers (async on the context stream) ---- */
int tfhe_gpu_gate_batch_dev(tfhe_gpu_ctx *ctx, const uint8_t *ops_dev, const uint32_t *a_dev,
                            const uint32_t *b_dev, uint32_t *out_dev, size_t B);
int tfhe_gpu_bootstrap_batch_dev(tfhe_gpu_ctx *ctx, const uint32_t *in_dev, uint32_t *out_dev,
                                 size_t B);
/* tfhe_gpu_bootstrap_lut_batch on device buffers (the test vector too: 2N
 * words of a TRLWE), single-device contexts (TFHE_ERR_INVALID on a multi-device one). */
int tfhe_gpu_bootstrap_lut_batch_dev(tfhe_gpu_ctx *ctx, const uint32_t *in_dev, const uint32_t *testvec_dev,
                                     uint32_t *out_dev, size_t B);
/* tfhe_gpu_reencrypt_batch on device buffers (B TLWELv0 of n + 1 words each),
 * single-device contexts; replaces the same reencryptTLWELv0 loop
 * (proxy_reenc.zig:267-306) without the PCIe copies. */
int tfhe_gpu_reencrypt_batch_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_reenc_key *key, const uint32_t *in_dev,
                                 uint32_t *out_dev, size_t B);

/* ---- Device timing (HIP events on the context stream, around each kernel) */
/* Between begin and end every bootstrap launch records events around its
 * blind-rotation and key-switch kernels; end synchronises and returns the
 * summed kernel milliseconds and the number of bootstrap launches. */
int tfhe_gpu_profile_begin(tfhe_gpu_ctx *ctx);
int tfhe_gpu_profile_end(tfhe_gpu_ctx *ctx, double *blind_rotate_ms, double *key_switch_ms,
                         int *launches);

/* ---- Stage entry points (parity tests; same kernels as the path) ------- */
/* KlemsaProcessor.ifft1024 (fft.zig:293-366): B×N u32 -> B×N f64. */
int tfhe_gpu_fft_forward_batch(tfhe_gpu_ctx *ctx, const uint32_t *in, double *out, size_t B);
/* KlemsaProcessor.fft1024 (fft.zig:370-443): B×N f64 -> B×N u32. */
int tfhe_gpu_fft_inverse_batch(tfhe_gpu_ctx *ctx, const double *in, uint32_t *out, size_t B);
/* KlemsaProcessor.poly_mul (fft.zig:458-492): B pairs. */
int tfhe_gpu_poly_mul_batch(tfhe_gpu_ctx *ctx, const uint32_t *a, const uint32_t *b,
                            uint32_t *out, size_t B);
/* trgsw.externalProductWithFft (trgsw.zig:111-154) against BK row `bk_index`
 * of the loaded key (or `trgsw_fft` = one TRGSWLv1FFT, 2L*2*N doubles, if non-NULL). */
int tfhe_gpu_external_product_batch(tfhe_gpu_ctx *ctx, const double *trgsw_fft, uint32_t bk_index,
                                    const uint32_t *trlwe_in, uint32_t *trlwe_out, size_t B);
/* trgsw.identityKeySwitching (trgsw.zig:471-502): B TLWELv1 -> B TLWELv0. */
int tfhe_gpu_key_switch_batch(tfhe_gpu_ctx *ctx, const uint32_t *in_lv1, uint32_t *out_lv0, size_t B);

/* ---- Leveled operations: CMUX, TRGSW selectors, encrypted table lookup -----
 * The leveled half of the reference (no bootstrap): a CMUX costs one external
 * product where a gate costs n.  All of these run on the context's first
 * device; CMUX, lookup and the encryptions need no cloud key and take the
 * decomposition offset from the parameter set (key.zig:121-131).  They always
 * run the reference's f64 expression trees (TFHE_OPT_ARITH does not apply: a
 * caller's selector is not a keygen'd BK row).  TRLWELv1 = 2N words (a then b). */
/* TRLWELv1.encryptF64 (trlwe.zig:30-64); item i uses DefaultPrng(seed0 + i); poly_mul on the device as keygen does. */
int tfhe_gpu_trlwe_encrypt_batch(tfhe_gpu_ctx *ctx, const uint32_t *key_lv1, const double *mu /*B*N*/, double alpha,
                                 uint64_t seed0, uint32_t *out /*B*2N*/, size_t B);
/* TRLWELv1.decryptBool (trlwe.zig:85-98). */
int tfhe_gpu_trlwe_decrypt_bool_batch(tfhe_gpu_ctx *ctx, const uint32_t *key_lv1, const uint32_t *ct,
                                      uint8_t *bits /*B*N*/, size_t B);
/* TRGSWLv1.encryptTorus + TRGSWLv1FFT.new (trgsw.zig:35-91); TRGSW s: a master DefaultPrng(seed0 + s) supplies
 * its 2L row seeds in order.  out_fft: S*2L*2*N doubles in the reference layout (one BootstrappingKey entry each). */
int tfhe_gpu_trgsw_encrypt_batch(tfhe_gpu_ctx *ctx, const uint32_t *key_lv1, const uint32_t *mu /*S*/, double alpha,
                                 uint64_t seed0, double *out_fft, size_t S);
/* S selectors (TRGSWLv1FFT, reference layout) resident on the device in the device layout of the
 * bootstrapping key's rows.  S >= 1.  A set serves the context that loaded it. */
typedef struct tfhe_gpu_trgsw_set tfhe_gpu_trgsw_set;
int  tfhe_gpu_trgsw_set_load(tfhe_gpu_ctx *ctx, const double *trgsw_fft, size_t S, tfhe_gpu_trgsw_set **out);
void tfhe_gpu_trgsw_set_destroy(tfhe_gpu_trgsw_set *set);
/* trgsw.cmux (trgsw.zig:260-284): out[i] = cmux(in0[i], in1[i], set[sel[i]]) = ExtProd(set[sel[i]], in1[i] - in0[i])
 * + in0[i], i.e. in1[i] where the selector encrypts 1.  sel is a HOST array in both variants; the _dev one takes
 * the ciphertexts in HBM and is asynchronous on the context stream. */
int tfhe_gpu_cmux_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_trgsw_set *set, const uint32_t *sel, const uint32_t *in0,
                        const uint32_t *in1, uint32_t *out, size_t B);
int tfhe_gpu_cmux_batch_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_trgsw_set *set, const uint32_t *sel,
                            const uint32_t *in0_dev, const uint32_t *in1_dev, uint32_t *out_dev, size_t B);
/* Table lookup by a CMUX tree (a chain of trgsw.cmux, trgsw.zig:260-284; "vertical packing"): table = 2^k
 * TRLWELv1 shared by the Q queries; bit j of query q's address is set[addr[q*k + j]] (j = 0 the least significant:
 * level j pairs entries 2i, 2i+1 of the previous level); out[q] = table[address_q], 2^k - 1 CMUXes per query, one
 * launch per level.  1 <= k <= 12.  addr is a HOST array.  Queries run in chunks whose level buffers stay within
 * a fixed 256 MB (+ half of it) of context scratch. */
int tfhe_gpu_table_lookup_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k,
                                const uint32_t *table, uint32_t *out_trlwe /*Q*2N*/, size_t Q);
int tfhe_gpu_table_lookup_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_trgsw_set *set, const uint32_t *addr, uint32_t k,
                              const uint32_t *table_dev, uint32_t *out_dev, size_t Q);
/* Rotation by encrypted bits ("horizontal packing"): h CMUX steps on each of B TRLWELv1.  With acc_0 = in[b],
 *     acc_{j+1} = trgsw.cmux(acc_j, X^rot[j] * acc_j, set[sel[b*h + j]])     (polyMulWithXK, trgsw.zig:442-466)
 * for j = 0 .. h-1 in this order, and out[b] = acc_h: the accumulator is multiplied by X^rot[j] where selector j
 * encrypts 1.  One launch; the accumulator stays on chip for the whole chain.  1 <= h <= TFHE_ROTATE_MAX_STEPS,
 * every rot[j] <= 2N (shared by the batch); sel and rot are HOST arrays in both variants.  The _dev one takes the
 * ciphertexts in HBM, is asynchronous on the context stream and refuses a multi-device context; out_dev must not
 * overlap in_dev. */
#define TFHE_ROTATE_MAX_STEPS 32
int tfhe_gpu_rotate_by_bits_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_trgsw_set *set, const uint32_t *sel /*B*h*/,
                                  const uint32_t *rot /*h*/, uint32_t h, const uint32_t *in /*B*2N*/,
                                  uint32_t *out /*B*2N*/, size_t B);
int tfhe_gpu_rotate_by_bits_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_trgsw_set *set, const uint32_t *sel /*B*h*/,
                                const uint32_t *rot /*h*/, uint32_t h, const uint32_t *in_dev, uint32_t *out_dev,
                                size_t B);
/* Packed table lookup: 2^k entries of `width` bits (1 <= width <= N), `slots` = N / stride of them side by side in
 * one TRLWELv1 (stride = the next power of two >= width).  Entry e lives in TRLWE e >> h, bit c of it at
 * coefficient (e & (2^h - 1)) * stride + c, h = min(k, log2 slots); the table is 2^v TRLWELv1, v = k - h <= 12
 * (TFHE_ERR_INVALID beyond), shared by the Q queries.  Address bits as in tfhe_gpu_table_lookup_*.  The CMUX tree
 * over the 2^v TRLWEs runs under bits h .. k-1, then the rotation above under bits 0 .. h-1 with
 * rot[j] = 2N - stride * 2^j: coefficient c < width of out[q] is bit c of table[address_q], (2^v - 1) + h CMUXes
 * per query where the tree alone needs 2^k - 1.  tfhe_gpu_sample_extract_* at coefficients 0 .. width-1 makes
 * gate inputs of it.  tfhe_packed_lookup_plan (host only) gives the shape; rot[j] = 0 for j >= h. */
typedef struct {
    uint32_t stride, slots, h, v, trlwes, cmuxes;
    uint32_t rot[10];
} tfhe_packed_plan;
int tfhe_packed_lookup_plan(const tfhe_params *params, uint32_t k, uint32_t width, tfhe_packed_plan *out);
int tfhe_gpu_packed_lookup_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_trgsw_set *set, const uint32_t *addr /*Q*k*/,
                                 uint32_t k, uint32_t width, const uint32_t *table /*2^v*2N*/,
                                 uint32_t *out_trlwe /*Q*2N*/, size_t Q);
int tfhe_gpu_packed_lookup_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_trgsw_set *set, const uint32_t *addr /*Q*k*/,
                               uint32_t k, uint32_t width, const uint32_t *table_dev, uint32_t *out_dev, size_t Q);
/* Packed scatter-add, the write beside the packed lookup: table (shape and address bits as above) takes Q
 * TRLWELv1 delta[q], each moved to the slot its address names and added there.  With d = delta[q]:
 *   rotate: for j = 0 .. h-1 in this order, d <- trgsw.cmux(d, X^(stride * 2^j) * d, set[addr[q*k + j]]), i.e.
 *           tfhe_gpu_rotate_by_bits_* with rot[j] = stride << j, the inverse of the lookup's rotation;
 *   demux:  level l = 0 .. v-1 runs under address bit k-1-l (most significant first); level 0 has the one node
 *           d; node i of level l with value x has the children 2i + 1 = hi = externalProductWithFft(selector, x)
 *           (trgsw.zig:111-154, the words of tfhe_gpu_external_product_batch) and 2i = lo = x - hi; leaf i of
 *           level v belongs to table TRLWE i: leaf address_q >> h carries d, every other leaf noise only;
 *   add:    table[i] += the sum over q of leaf i of query q.
 * Every add and subtraction is a wrapping u32 one on all 2N words, so the order of the sum, the chunking of the
 * queries and the launch shape change no word.  The phase of coefficients 0 .. width-1 of entry address_q grows by
 * the phase of coefficients 0 .. width-1 of delta[q]; queries with the same address all add.  h + (2^v - 1)
 * external products per query; width > N/2 gives stride = N, h = 0: the scatter into a table of whole TRLWEs.
 * Runs on the context's first device and needs no cloud key.  k >= 1, 1 <= width <= N, v <= 12, every addr[] < the
 * set's size (TFHE_ERR_INVALID otherwise, before any upload or launch); Q = 0 leaves the table as it is.  addr is a
 * HOST array in both variants; the _dev one takes delta and the table in HBM, updates the table in place, is
 * asynchronous on the context stream and refuses a multi-device context.  delta must not overlap table.  Queries
 * run in chunks whose leaves (2^v TRLWELv1 per query) stay within TFHE_OPT_SCATTER_SCRATCH_MB of context scratch
 * (+ half of it for the level before). */
int tfhe_gpu_packed_scatter_add_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_trgsw_set *set, const uint32_t *addr /*Q*k*/,
                                      uint32_t k, uint32_t width, const uint32_t *delta /*Q*2N*/,
                                      uint32_t *table /*2^v*2N, in and out*/, size_t Q);
int tfhe_gpu_packed_scatter_add_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_trgsw_set *set, const uint32_t *addr /*Q*k*/,
                                    uint32_t k, uint32_t width, const uint32_t *delta_dev,
                                    uint32_t *table_dev /*in place*/, size_t Q);
/* CMUX graphs: decision diagrams and (weighted) automata over TRGSW-encrypted bits, the leveled mode of the TFHE
 * paper.  One graph is shared by the Q queries of a call:
 *   nL >= 1 leaves, TRLWELv1 leaves[nL*2N] (usually trivial), and V >= 0 inner nodes.  Value ids: 0 .. nL-1 are the
 *   leaves, nL + v is node v.  Node v has var[v] < k, lo[v], hi[v] < nL + v (topological order) and rotations
 *   rlo[v], rhi[v] <= 2N.  For query q, with mulxk = polyMulWithXK (trgsw.zig:442-466),
 *       value[nL + v] = trgsw.cmux(mulxk(value[lo[v]], rlo[v]), mulxk(value[hi[v]], rhi[v]), set[addr[q*k + var[v]]])
 *   so hi (rotated) is chosen where the bit is 1.  roots[R] are value ids (a leaf id is allowed) and
 *   out[q*R + r] = value[roots[r]] of query q.
 * Word for word this is tfhe_gpu_cmux_batch node by node on inputs rotated on the host by polyMulWithXK: the rotations
 * are exact index and sign arithmetic, the CMUX is k_cmux's arithmetic in k_cmux's order (the reference's expression
 * trees; TFHE_OPT_ARITH does not apply and the near-tie counter is untouched).  The rotations add up in the exponent
 * along a path, so a leaf that is a test vector turns "the sum of the weights along the path" into any function of
 * that sum (weighted automata: popcount thresholds, small additions), and several roots give several functions
 * from one graph.
 * Noise: every CMUX on the path from a root to its chosen leaf adds one external product's error, whatever the
 * graph's width and however many nodes share a child, so a root's error grows with its depth only.  Two terms, both
 * measured at the 128-bit set on ladders of up to 64 levels (tests/test_cmux_graph.py):
 *   random: sigma = 2.1e-5 on the phase per CMUX, growing with the square root of the depth (1.6e-4 after 64 levels
 *     under selectors of 0);
 *   truncation: the reference's decomposition offset (key.zig:121-131) has no rounding half, so a CMUX whose selector
 *     encrypts 1 hands on its input less r, 0 <= r < 2^(32 - L*bgbit), on every word.  On the phase of coefficient i
 *     that is 2^-(L*bgbit + 1) * ((1 * s)[i] - 1) on average, 1 * s being the negacyclic product of the all-ones
 *     polynomial and the level-1 key: about -2^-(L*bgbit + 1) * N/2 at coefficient 0, the same at every such CMUX, so
 *     it adds up LINEARLY in the number of one-bits on the path.  128-bit set (L*bgbit = 18): -9.4e-4 per one-bit at
 *     coefficient 0, 3.1e-2 after 32 one-bits, a quarter of the +-1/8 of a bit; 64 one-bits take half of it.  A CMUX
 *     whose two inputs are the same words (a pass-through) adds exactly nothing: its digits are all zero.
 * Keep a path's one-bits below 1/8 over that step (about 130 at the 128-bit set), less what the leaves' own noise
 * and the key switch need.
 * tfhe_cmux_graph_plan (host only) checks a graph and gives level[v] = 1 + the largest level among node v's
 * non-leaf children (leaves are level 0, a node on two leaves is level 1), depth = the largest level, and
 * slot[v] < n_slots, the TRLWELv1 of per-query scratch node v is written to.  One level is one launch, within which
 * reads and writes are unordered: a slot is taken again by a node of level l only when its occupant and every reader
 * of it have levels < l, and a root's slot never is.  TFHE_ERR_INVALID, and nothing written: nL = 0, a child id >= the
 * node's own, var >= k, a rotation > 2N, a root >= nL + V, a null array with a non-zero count (level / slot with
 * V > 0 included; depth and n_slots may be NULL).
 * tfhe_gpu_cmux_graph_*: addr, the node arrays and roots are HOST arrays in both variants.  extract = 0: out = Q*R
 * TRLWELv1; 1: sampleExtractIndex(., 0) of each (trlwe.zig:146-162), Q*R TLWELv1 of N + 1 words; 2: that plus
 * identityKeySwitching (trgsw.zig:471-502), Q*R TLWELv0, what tfhe_gpu_sample_extract_* with coef = {0} and
 * key_switch gives: ordinary gate or LUT inputs (TFHE_ERR_NO_KEY without a cloud key).  One launch per level over all
 * queries of a chunk; queries run in chunks whose slots (n_slots * 8 KB per query) stay within the lookup's 256 MB,
 * or of at most TFHE_OPT_GRAPH_CHUNK_QUERIES queries; chunking changes no word.  TFHE_ERR_INVALID before any upload
 * or launch: the plan's refusals, an addr[] >= the set's size, a set of another context, a null argument, extract
 * outside 0..2, k = 0 with V > 0.  Q = 0 is TFHE_OK; V = 0 is legal (the roots are leaves).  Runs on the context's
 * first device.  The _dev variant takes leaves and out in HBM, is asynchronous on the context stream, refuses a
 * multi-device context and requires out not to overlap leaves. */
int tfhe_cmux_graph_plan(uint32_t nL, uint32_t V, uint32_t k, const uint32_t *var, const uint32_t *lo,
                         const uint32_t *hi, const uint32_t *rlo, const uint32_t *rhi, uint32_t R, const uint32_t *roots,
                         uint32_t N, uint32_t *level /*V*/, uint32_t *slot /*V*/, uint32_t *depth, uint32_t *n_slots);
int tfhe_gpu_cmux_graph_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_trgsw_set *set, const uint32_t *addr /*Q*k*/, uint32_t k,
                              const uint32_t *leaves /*nL*2N*/, uint32_t nL, uint32_t V, const uint32_t *var,
                              const uint32_t *lo, const uint32_t *hi, const uint32_t *rlo, const uint32_t *rhi,
                              uint32_t R, const uint32_t *roots, int extract, uint32_t *out, size_t Q);
int tfhe_gpu_cmux_graph_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_trgsw_set *set, const uint32_t *addr /*Q*k*/, uint32_t k,
                            const uint32_t *leaves_dev, uint32_t nL, uint32_t V, const uint32_t *var,
                            const uint32_t *lo, const uint32_t *hi, const uint32_t *rlo, const uint32_t *rhi,
                            uint32_t R, const uint32_t *roots, int extract, uint32_t *out_dev, size_t Q);
/* sampleExtractIndex (trlwe.zig:146-162) at the C coefficients coef[] (host, each < N) of each of B TRLWELv1,
 * TRLWE-major; key_switch != 0 adds identityKeySwitching (trgsw.zig:471-502; TFHE_ERR_NO_KEY without a cloud
 * key): out = B*C*(N+1) or B*C*(n+1) words, ordinary TLWELv1 / TLWELv0 (gate inputs). */
int tfhe_gpu_sample_extract_batch(tfhe_gpu_ctx *ctx, const uint32_t *trlwe, const uint32_t *coef, size_t C,
                                  int key_switch, uint32_t *out, size_t B);
int tfhe_gpu_sample_extract_dev(tfhe_gpu_ctx *ctx, const uint32_t *trlwe_dev, const uint32_t *coef, size_t C,
                                int key_switch, uint32_t *out_dev, size_t B);

/* ---- Packing key switch: TLWELv0 -> a coefficient slot of a TRLWELv1 --------
 * The way from the bootstrapped half (gates, circuits, LUT bootstraps: TLWELv0) into the leveled half (CMUX, table
 * lookup, packed lookup: TRLWELv1 tables): the public key switch of identityKeySwitching (trgsw.zig:471-502) and
 * reencryptTLWELv0 with a key whose rows are TRLWELv1.  Shape (basebit, t), base = 2^basebit: n*t*base rows of 2N
 * words, row[base*t*i + base*j + k] for k >= 1 = TRLWELv1.encryptF64 (trlwe.zig:30-64) under key_lv1 of the
 * polynomial whose coefficient 0 is (f64)k * (f64)key_lv0[i] / (f64)(1 << ((j+1)*basebit)) (key.zig:164) and whose
 * other coefficients are 0.0, with alpha and DefaultPrng(seed0 + idx): the words tfhe_gpu_trlwe_encrypt_batch gives
 * for that mu and seed.  Rows with k = 0 are zero.
 * Pack: B*C TLWELv0 in[b*C + c] and C distinct coefficients coef[] (HOST array, each < N, shared by the batch, as in
 * tfhe_gpu_sample_extract_*) give B TRLWELv1.  With PREC = 1 << (32 - (1 + basebit*t)), a'_i = a_i + PREC and
 * d_ij = (a'_i >> (32 - (j+1)*basebit)) & (base - 1), in wrapping u32 arithmetic on all 2N words,
 *     R    = (a = 0, b = (in.b, 0, ..., 0)) - sum_{i<n, j<t} row[base*t*i + base*j + d_ij]
 *     out[b] = sum_c X^coef[c] * R_{b,c}     (polyMulWithXK, trgsw.zig:442-466, on the a half and on the b half)
 * so the phase of out[b] at coefficient coef[c] is that of in[b*C + c] plus key-switch noise, and the other
 * coefficients hold noise only: a gate output (+-1/8) becomes a table bit in the encoding of
 * tfhe_lookup_table_pack_bits / _pack_slots, a LUT output keeps its message.  Integer-exact: one defined word pattern.
 * Shapes: those with the one-hot GEMM form, basebit 2 with t 7..9 and basebit 5 with t 2..3; TFHE_ERR_INVALID
 * otherwise, and TFHE_OPT_KS_FORM does not apply (there is one form).  TFHE_ERR_INVALID too, before any launch or
 * upload: len != n*t*base*2N, C = 0 or > N, a coef >= N or listed twice, a key of another context, a null argument.
 * B = 0 is TFHE_OK.  Like the leveled entries these run on the context's first device and need no cloud key; _dev
 * takes in / out in HBM, is asynchronous on the context stream and refuses a multi-device context.
 * After tfhe_gpu_packing_key_load only the matrix-core layout of the key stays resident (n'*t*base*2N*4 bytes with
 * n' = n rounded up to blocks of 8 (basebit 2) or 4 (basebit 5): 184.5 MB at the 128-bit set with (2, 8), 644.9 MB at
 * UINT4 with (5, 3)); the u32 rows are staged in HBM and freed.  The
 * per-item GEMM sums (K splits x items x 2N words) live in context scratch: a batch runs in chunks of items that
 * keep them within TFHE_OPT_PACK_SCRATCH_MB (default 256 MB, the table lookup's bound). */
/* host rows: n*t*2^basebit*2N words; needs a context for the poly_mul of each TRLWE encryption */
int  tfhe_gpu_packing_key_gen(tfhe_gpu_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha,
                              uint32_t basebit, uint32_t t, uint64_t seed0, uint32_t *rows);
typedef struct tfhe_gpu_packing_key tfhe_gpu_packing_key;
int  tfhe_gpu_packing_key_load(tfhe_gpu_ctx *ctx, const uint32_t *rows, size_t len /*words*/, uint32_t basebit,
                               uint32_t t, tfhe_gpu_packing_key **out);
void tfhe_gpu_packing_key_destroy(tfhe_gpu_packing_key *key);
int  tfhe_gpu_pack_tlwe_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_packing_key *key, const uint32_t *in /*B*C*(n+1)*/,
                              const uint32_t *coef /*C, host*/, size_t C, uint32_t *out_trlwe /*B*2N*/, size_t B);
int  tfhe_gpu_pack_tlwe_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_packing_key *key, const uint32_t *in_dev,
                            const uint32_t *coef /*C, host*/, size_t C, uint32_t *out_dev, size_t B);
/* host only, no device: the definition above, for callers without a GPU */
int  tfhe_pack_tlwe(const tfhe_params *params, const uint32_t *rows, uint32_t basebit, uint32_t t, const uint32_t *in,
                    const uint32_t *coef, size_t C, uint32_t *out_trlwe, size_t B);

/* ---- LUT circuits: per-item tables and linear combinations on the device ----
 * The unit of work of multi-bit arithmetic (radix digits, comparisons, bivariate functions through a + m*b; two
 * full-width digits: "Bivariate LUT bootstrap" below): a small
 * integer combination of ciphertexts, then a programmable bootstrap whose table is chosen per item.  Node i over a
 * pool of P TLWELv0 computes, in wrapping u32 arithmetic on all n+1 words (TLWELv0.add / neg / addMul / subMul,
 * tlwe.zig:120-240; term_coef is an int32 used as a Torus word in two's complement),
 *     x_i = sum_{k in [term_off[i], term_off[i+1])} term_coef[k] * pool[term_src[k]] + (0, ..., 0, konst[i])
 * (no terms: the trivial ciphertext of konst[i]) and out_i = exactly the words tfhe_gpu_bootstrap_lut_batch returns
 * for the input x_i and the test vector set[lut[i]] (blindRotateWithTestvec, sampleExtractIndex(0),
 * identityKeySwitching).  Encoder.encode is message * scale (encoder.zig:66-73), so an integer combination of
 * ciphertexts encodes the same combination of messages.  All of these run on the context's first device.
 * The descriptors (term_off, term_src / term_wire, term_coef, konst, lut) are HOST arrays in both variants and are
 * checked before any launch: TFHE_ERR_INVALID unless term_off[0] == 0 and term_off is monotone, every source is
 * < P (in a circuit: an earlier wire), every lut[i] < T and the set belongs to this context.  TFHE_ERR_NO_KEY
 * without a cloud key; B == 0 / n_nodes == 0 is TFHE_OK.  The _dev variants take the ciphertexts in HBM, are
 * asynchronous on the context stream and refuse a multi-device context. */
typedef struct tfhe_gpu_lut_set tfhe_gpu_lut_set;
/* T >= 1 test vectors (TRLWELv1, 2N words each, any a) resident on the context's first device. */
int  tfhe_gpu_lut_set_load(tfhe_gpu_ctx *ctx, const uint32_t *testvecs /*T*2N*/, size_t T, tfhe_gpu_lut_set **out);
void tfhe_gpu_lut_set_destroy(tfhe_gpu_lut_set *set);
/* B nodes over a pool of P ciphertexts: out = B*(n+1) words. */
int tfhe_gpu_lut_apply_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, const uint32_t *pool, size_t P,
                             const uint32_t *term_off /*B+1*/, const uint32_t *term_src, const int32_t *term_coef,
                             const uint32_t *konst /*B*/, const uint32_t *lut /*B*/, uint32_t *out, size_t B);
int tfhe_gpu_lut_apply_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, const uint32_t *pool_dev, size_t P,
                           const uint32_t *term_off /*B+1*/, const uint32_t *term_src, const int32_t *term_coef,
                           const uint32_t *konst /*B*/, const uint32_t *lut /*B*/, uint32_t *out_dev, size_t B);
/* A DAG of such nodes: wires 0..n_inputs-1 are the inputs, node g drives wire n_inputs+g, every term wire of node g
 * is < n_inputs+g.  Each dependency level is one combination launch and one bootstrap launch; every wire stays in
 * HBM.  outputs receives the n_outputs wires out_wires[] (an input wire is allowed); *levels (may be NULL) the
 * bootstrap depth. */
int tfhe_gpu_lut_circuit_eval(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, size_t n_inputs, const uint32_t *inputs,
                              size_t n_nodes, const uint32_t *term_off, const uint32_t *term_wire,
                              const int32_t *term_coef, const uint32_t *konst, const uint32_t *lut, size_t n_outputs,
                              const uint32_t *out_wires, uint32_t *outputs, uint32_t *levels);
int tfhe_gpu_lut_circuit_eval_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, size_t n_inputs,
                                  const uint32_t *inputs_dev, size_t n_nodes, const uint32_t *term_off,
                                  const uint32_t *term_wire, const int32_t *term_coef, const uint32_t *konst,
                                  const uint32_t *lut, size_t n_outputs, const uint32_t *out_wires,
                                  uint32_t *outputs_dev, uint32_t *levels);
/* The schedule tfhe_gpu_lut_circuit_eval runs, host only: levels[g] = 1 + the largest level of node g's term wires
 * (inputs are level 0; a node without terms is level 1), *depth (may be NULL) the largest. */
int tfhe_lut_circuit_schedule(size_t n_inputs, size_t n_nodes, const uint32_t *term_off, const uint32_t *term_wire,
                              uint32_t *levels, uint32_t *depth);

/* ---- Multi-output LUT bootstrap: 2^theta tables from one blind rotation ----
 * Several functions of one combined input (message and carry of a radix digit, < and ==, quotient and remainder) for
 * the price of one blind rotation and theta bits of message room.  Integer-exact; with nbit = log2 N,
 * s = 32 - (nbit + 1) + theta and 0 <= theta <= TFHE_LUT_MULTI_MAX_LOG:
 *   round_theta(w) = (w + (1 << (s-1))) & ~((1 << s) - 1) in wrapping u32 on all n+1 words of a TLWELv0 for
 *     theta >= 1, and the identity for theta = 0.  A rounded word is a multiple of 2^(21+theta) (N = 1024), so the
 *     blind rotation's own mod switch (w + 2^20) >> 21 (trgsw.zig:290-333) returns exactly w >> 21, a multiple of
 *     2^theta: the accumulator is rotated by a multiple of nu = 2^theta.
 *   interleave: from nu test vectors tv_0 .. tv_{nu-1} (TRLWELv1, any a), on both halves h,
 *     TV[h][q] = tv_{q mod nu}[h][q - (q mod nu)]; after a rotation by a multiple of nu, coefficient j of the
 *     accumulator holds what tv_j holds at the rounded phase.
 *   node: with x the node's combination exactly as tfhe_gpu_lut_apply_* defines it, output j < 2^theta is, word for
 *     word, identityKeySwitching(sampleExtractIndex(blindRotateWithTestvec(round_theta(x), set[lut]), j)): what
 *     tfhe_gpu_blind_rotate_batch, then tfhe_gpu_sample_extract_* with coef = 0 .. nu-1 and key_switch = 1 give.
 *     A theta = 0 node gives exactly the words of tfhe_gpu_lut_apply_batch.
 * Noise rule: the rounding's phase error, in positions of 2N, has sigma ~ 2^theta * sqrt((n/2 + 1) / 12) for a
 * binary key.  A message block of Encoder.new(m) is N/m positions wide and read at its centre (generator.zig:94-112):
 * the margin is N/(2m) positions, so each theta costs exactly one bit of m at equal margin.  UINT4 (n = 820):
 * m = 16, theta = 0: 32 / 5.86 = 5.5 sigma (today's); m = 8, theta = 1: 64 / 11.7 = 5.5 sigma; m = 4, theta = 2 the
 * same; m = 16, theta = 1: 2.7 sigma, wrong about once in 150 -- do not use it.  The library never sees m and does
 * not police it. */
#define TFHE_LUT_MULTI_MAX_LOG 3
/* host only, no device: round_theta over B TLWELv0 (in == out is allowed); TFHE_ERR_INVALID for theta > 3 */
int tfhe_lut_round_tlwe(const tfhe_params *params, uint32_t theta, const uint32_t *in, uint32_t *out, size_t B);
int tfhe_lut_interleave(const tfhe_params *params, const uint32_t *testvecs /*2^theta*2N*/, uint32_t theta,
                        uint32_t *out /*2N*/);
/* tfhe_gpu_lut_apply_* with theta[i] per node (HOST array of B; NULL = all 0, the existing entry): out holds
 * sum_i 2^theta[i] ciphertexts of n+1 words, node-major, node i's outputs consecutive.  A call whose thetas are all 0
 * runs exactly what tfhe_gpu_lut_apply_* runs.  Checked before any launch: a theta > TFHE_LUT_MULTI_MAX_LOG and
 * everything tfhe_gpu_lut_apply_* checks (TFHE_ERR_INVALID). */
int tfhe_gpu_lut_apply_multi_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, const uint32_t *pool, size_t P,
                                   const uint32_t *term_off /*B+1*/, const uint32_t *term_src, const int32_t *term_coef,
                                   const uint32_t *konst /*B*/, const uint32_t *lut /*B*/, const uint32_t *theta /*B*/,
                                   uint32_t *out, size_t B);
int tfhe_gpu_lut_apply_multi_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, const uint32_t *pool_dev, size_t P,
                                 const uint32_t *term_off /*B+1*/, const uint32_t *term_src, const int32_t *term_coef,
                                 const uint32_t *konst /*B*/, const uint32_t *lut /*B*/, const uint32_t *theta /*B*/,
                                 uint32_t *out_dev, size_t B);
/* tfhe_gpu_lut_circuit_eval* with theta[g] per node (NULL = the existing entries): node g drives the 2^theta[g] wires
 * n_inputs + o_g + j, o_g = sum_{g' < g} 2^theta[g'], and every term wire of node g is < n_inputs + o_g.  A level
 * with a theta > 0 runs combine-and-round, one blind rotation per node, the fan-out extraction and one key switch
 * over the level's outputs; a level whose thetas are all 0 runs what tfhe_gpu_lut_circuit_eval runs. */
int tfhe_gpu_lut_circuit_eval_multi(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, size_t n_inputs,
                                    const uint32_t *inputs, size_t n_nodes, const uint32_t *term_off,
                                    const uint32_t *term_wire, const int32_t *term_coef, const uint32_t *konst,
                                    const uint32_t *lut, const uint32_t *theta /*n_nodes*/, size_t n_outputs,
                                    const uint32_t *out_wires, uint32_t *outputs, uint32_t *levels);
int tfhe_gpu_lut_circuit_eval_multi_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, size_t n_inputs,
                                        const uint32_t *inputs_dev, size_t n_nodes, const uint32_t *term_off,
                                        const uint32_t *term_wire, const int32_t *term_coef, const uint32_t *konst,
                                        const uint32_t *lut, const uint32_t *theta /*n_nodes*/, size_t n_outputs,
                                        const uint32_t *out_wires, uint32_t *outputs_dev, uint32_t *levels);
/* host only: tfhe_lut_circuit_schedule for the multi-output wire numbering (levels has n_nodes entries) */
int tfhe_lut_circuit_schedule_multi(size_t n_inputs, size_t n_nodes, const uint32_t *term_off,
                                    const uint32_t *term_wire, const uint32_t *theta /*n_nodes*/, uint32_t *levels,
                                    uint32_t *depth);

/* ---- Extended LUT bootstrap: 5- and 6-bit digits on the N = 1024 key ----
 * The mirror image of the multi-output bootstrap: eta extra bits of message room for 2^eta external products per
 * step, with the key and the transforms as they are (Lee, Yoon, "Discretization error reduction for TFHE").  The
 * blind rotation runs in Z[X]/(X^(N E) + 1), E = 2^eta, 0 <= eta <= TFHE_LUT_EXT_MAX_LOG, so its mod switch rounds to
 * 2N E positions.  A polynomial of that ring is kept as E components over the ring of the key,
 *     P(X) = sum_{j<E} X^j P_j(Y),  Y = X^E,  Y^N = -1,
 * each an ordinary TRLWELv1 of 2N words; BK_i, a TRGSW over Z[Y]/(Y^N + 1), acts on every component separately.
 * Word-exact, with nbit = log2 N, sh = 32 - (nbit + 1) - eta, mulxk = polyMulWithXK (trgsw.zig:442-466) with its
 * exponent taken mod 2N, cmux = trgsw.cmux (trgsw.zig:260-284) in the reference's expression trees:
 *   extended test vector: TV = Generator.generateLookupTableAssign at polynomial degree N E (the function of
 *     (degree, m) tfhe_lut_generate is), stored as E TRLWELv1 tv_j with tv_j.a = 0, tv_j.b[k] = TV.b[k E + j].  In a
 *     tfhe_gpu_lut_set the extended table t is the E consecutive entries set[t E + j].
 *   ext_rotate(c_0 .. c_{E-1}, a) for 0 <= a <= 2N E, a = q E + r: output component k is
 *     mulxk(c_{(k - r) mod E}, q + [k < r]) on both halves; a = 2N E is the identity.
 *   blind rotation of the TLWELv0 (a_0 .. a_{n-1}, b): b~ = 2N E - ((b + 2^(sh-1)) >> sh),
 *     a~_i = (a_i + 2^(sh-1)) >> sh, the adds in 64 bits (trgsw.zig:297, :312); acc = ext_rotate(tv, b~); for i < n:
 *     rot = ext_rotate(acc, a~_i), acc_k = cmux(BK_i; in0 = acc_k, in1 = rot_k) for every k.
 *   output: identityKeySwitching(sampleExtractIndex(acc_0, 0)).
 * eta = 0 is the ordinary bootstrap: a call with eta = 0 runs exactly what the entry without eta runs.
 * Noise rule: the mod switch's phase error, in positions of 2N E, has sigma ~ sqrt((n/2 + 1) / 12) for a binary key
 * whatever eta is, and a message block of Encoder.new(m) is read N E / (2m) positions from its edge: each eta buys
 * exactly one bit of m at equal margin.  UINT4 (n = 820, sigma = 5.86): m = 16, eta = 0: 32 / 5.86 = 5.5 sigma
 * (today's); m = 32, eta = 1 and m = 64, eta = 2 the same; m = 64 at eta = 0 has 1.4 sigma (one input in six is
 * read wrong) and at eta = 1 2.7 sigma -- do not use them.  The accumulator's own error and the key switch's do not
 * shrink with eta: at UINT4 they leave the output a phase error of sigma 7.5e-4 (measured) against
 * the half-spacing 1/(4m) = 3.9e-3 at m = 64, 5.2 sigma.  The library never sees m and does not police it. */
#define TFHE_LUT_EXT_MAX_LOG 2
/* host only, no device; TFHE_ERR_INVALID for eta > TFHE_LUT_EXT_MAX_LOG.  The E = 2^eta components of the extended
 * test vector of f (f_table[x], x < m, as tfhe_lut_generate takes it); eta = 0 gives tfhe_lut_generate's words. */
int tfhe_lut_generate_ext(const tfhe_params *params, uint32_t eta, uint32_t m, const uint32_t *f_table,
                          uint32_t *out /*E*2N*/);
/* ext_rotate on E components (in != out); a > 2N E is TFHE_ERR_INVALID. */
int tfhe_lut_ext_rotate(const tfhe_params *params, uint32_t eta, const uint32_t *in /*E*2N*/, uint32_t a,
                        uint32_t *out /*E*2N*/);
/* (word + 2^(sh-1)) >> sh, a position in [0, 2N E]; a negative status on a refusal. */
int tfhe_lut_ext_mod_switch(const tfhe_params *params, uint32_t eta, uint32_t word);
/* Stage entry (parity tests): the blind rotation alone, all E accumulators of each of B TLWELv0 inputs under one
 * shared extended test vector, item-major (out[(i E + k) 2N ..] is acc_k of item i).  First device only; eta = 0 is
 * tfhe_gpu_blind_rotate_batch. */
int tfhe_gpu_blind_rotate_ext_batch(tfhe_gpu_ctx *ctx, uint32_t eta, const uint32_t *in, const uint32_t *testvecs /*E*2N*/,
                                    uint32_t *out /*B*E*2N*/, size_t B);
/* tfhe_gpu_lut_apply_* with the extended bootstrap: x_i exactly as tfhe_gpu_lut_apply_* defines it (the same
 * combination launch), out_i the extended bootstrap of x_i with the extended table lut[i] of the set.  Checked before
 * any launch (TFHE_ERR_INVALID): eta > TFHE_LUT_EXT_MAX_LOG, a lut[i] E + E beyond the set, and everything
 * tfhe_gpu_lut_apply_* checks; TFHE_ERR_NO_KEY and B == 0 as there.  First device only; the _dev form is asynchronous
 * on the context stream and refuses a multi-device context. */
int tfhe_gpu_lut_apply_ext_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, uint32_t eta, const uint32_t *pool,
                                 size_t P, const uint32_t *term_off /*B+1*/, const uint32_t *term_src,
                                 const int32_t *term_coef, const uint32_t *konst /*B*/, const uint32_t *lut /*B*/,
                                 uint32_t *out, size_t B);
int tfhe_gpu_lut_apply_ext_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, uint32_t eta, const uint32_t *pool_dev,
                               size_t P, const uint32_t *term_off /*B+1*/, const uint32_t *term_src,
                               const int32_t *term_coef, const uint32_t *konst /*B*/, const uint32_t *lut /*B*/,
                               uint32_t *out_dev, size_t B);

/* ---- Bivariate LUT bootstrap: a test vector built on the device per item ----
 * Any function f(x, y) of two digits at the full message modulus m of the parameter set (UINT4: 4 + 4 bits in), where
 * a + m*b spends half of the message room: the tree-based functional bootstrap (Guimaraes, Borin, Aranha, "Revisiting
 * the functional bootstrap in TFHE").  y goes through the m tables f(i, .), the m results are packed into the
 * coefficient slots of one TRLWELv1, the slots are spread into a test vector in the generator's layout, and x is
 * bootstrapped with that encrypted test vector: m + 1 blind rotations per output digit.  Integer-exact from its second
 * step on; with w = N/m, off = N/(2m), mulxk = polyMulWithXK (trgsw.zig:442-466) and wrapping u32 arithmetic:
 *   spread: on each half h of a TRLWELv1 separately,
 *       S[h] = sum_{j=0}^{w-1} mulxk(in[h], j)     (the negacyclic window sum of width w)
 *       out[h] = mulxk(S[h], rot)
 *     with 1 <= w <= N and 0 <= rot <= 2N (it knows nothing of m).  For in.a = 0, in.b[x*w] = Encoder.encode(f(x)),
 *     the other coefficients 0 and rot = 2N - off, out is exactly Generator.generateLookupTableAssign's table
 *     (lut/generator.zig:85-135), the words of tfhe_lut_generate.  w = 1, rot = 0 is the identity.
 *   each: output i of tfhe_gpu_bootstrap_lut_each_* is, word for word, what tfhe_gpu_bootstrap_lut_batch returns for
 *     in[i] with the test vector testvecs[i] (any a): the per-item instantiations of the blind rotation that a LUT
 *     set runs, reading one TRLWELv1 per item from the caller's buffer.
 *   node b of tfhe_gpu_lut_apply2_*, over a pool of P TLWELv0 and a set of F*m tables, set[fn*m + i] = the table of
 *     y -> f_fn(i, y):
 *       1. g[b][i] = the tfhe_gpu_lut_apply_* output of the one-term node (pool[y_src[b]], coefficient 1, konst 0,
 *          lut = fn[b]*m + i), for i < m;
 *       2. P_b = tfhe_pack_tlwe(g[b][0 .. m), coef[i] = i*w, C = m);
 *       3. TV_b = spread(P_b, w, 2N - off);
 *       4. out[b] = the tfhe_gpu_bootstrap_lut_each_* output for pool[x_src[b]] with TV_b,
 *     so out[b] decrypts to f_fn(x, y).  Everything stays in HBM; the nodes run in chunks whose m intermediate
 *     ciphertexts per node and whose GEMM sums stay within TFHE_OPT_PACK_SCRATCH_MB, and chunking changes no word.
 * Noise rule (the library does not police it): the error of TV_b at the coefficient that is read is the level-1
 * output's own noise, plus the pack's digit rounding, variance ~ (n/2) * 2^(-2*basebit*t) / 12, plus
 * w*m*n*t*alpha_rows^2 from the packing key's rows over the summed window (N*n*t of them: w per slot, m slots).  With
 * the packing key's default alpha (alpha_lv1) the last term vanishes at the UINT sets (2^-52 rounds to nothing in a
 * 32-bit torus), and at UINT4 with the default pack shape (5, 3) the rounding term is sigma ~ 2e-4 against a
 * half-spacing of 1/64 ~ 1.6e-2.  A packing key generated with alpha_lv0 instead would put sigma near 4e-3, a quarter
 * of the half-spacing: unsafe, do not use one here.  Measured figures: DESIGN.md §4.9c.
 * Checked before any launch or upload (TFHE_ERR_INVALID): w = 0, w > N, rot > 2N; m not a power of two, m < 2 or
 * 2m > N; a set size that is no multiple of m; an fn[b]*m + m beyond the set; a source >= P; a set or a key of
 * another context; a null argument.  TFHE_ERR_NO_KEY without a cloud key (spread needs none); B = 0 is TFHE_OK.  All
 * of these run on the context's first device; fn / x_src / y_src are HOST arrays in both variants; the _dev ones take
 * the ciphertexts in HBM, are asynchronous on the context stream and refuse a multi-device context.  spread may run
 * in place (out == in). */
/* host only, no device: the definition of spread over B TRLWELv1 (in == out is allowed) */
int tfhe_lut_spread(const tfhe_params *params, const uint32_t *in /*B*2N*/, uint32_t w, uint32_t rot,
                    uint32_t *out /*B*2N*/, size_t B);
int tfhe_gpu_lut_spread_batch(tfhe_gpu_ctx *ctx, const uint32_t *in /*B*2N*/, uint32_t w, uint32_t rot,
                              uint32_t *out /*B*2N*/, size_t B);
int tfhe_gpu_lut_spread_dev(tfhe_gpu_ctx *ctx, const uint32_t *in_dev, uint32_t w, uint32_t rot, uint32_t *out_dev,
                            size_t B);
int tfhe_gpu_bootstrap_lut_each_batch(tfhe_gpu_ctx *ctx, const uint32_t *in /*B*(n+1)*/,
                                      const uint32_t *testvecs /*B*2N*/, uint32_t *out /*B*(n+1)*/, size_t B);
int tfhe_gpu_bootstrap_lut_each_dev(tfhe_gpu_ctx *ctx, const uint32_t *in_dev, const uint32_t *testvecs_dev,
                                    uint32_t *out_dev, size_t B);
int tfhe_gpu_lut_apply2_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk,
                              uint32_t m, const uint32_t *pool, size_t P, const uint32_t *fn /*B*/,
                              const uint32_t *x_src /*B*/, const uint32_t *y_src /*B*/, uint32_t *out /*B*(n+1)*/,
                              size_t B);
int tfhe_gpu_lut_apply2_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk,
                            uint32_t m, const uint32_t *pool_dev, size_t P, const uint32_t *fn /*B*/,
                            const uint32_t *x_src /*B*/, const uint32_t *y_src /*B*/, uint32_t *out_dev, size_t B);

/* ---- Select nodes: LUT-circuit nodes whose table is made of wires ----
 * The bivariate bootstrap as a node kind of the circuit evaluator, and with it trees over three or more digits and
 * reads of a client-encrypted table by an address the server computed.  With m a power of two, 2 <= m, 2m <= N,
 * w = N/m and off = N/(2m) as in tfhe_gpu_lut_apply2_*, a select node g has a combination x_g, exactly as
 * tfhe_gpu_lut_apply_* defines it (terms, coefficients, konst), and m entries e_g[0 .. m), each either the words of
 * an earlier wire or the trivial TLWELv0 (0, ..., 0, c) of a torus word c.  Its output is, word for word,
 *       1. P_g  = tfhe_pack_tlwe(e_g[0 .. m), coef[i] = i*w, C = m);
 *       2. TV_g = tfhe_lut_spread(P_g, w, 2N - off);
 *       3. out_g = the tfhe_gpu_bootstrap_lut_each_* output for x_g with TV_g,
 * so out_g decrypts to what entry number x_g decrypts to.  Consequences: entries that are all constants
 * Encoder.encode(f(i)) give exactly the words of an ordinary node with the table tfhe_lut_generate(m, f) (the pack of
 * trivial inputs leaves a = 0 and b[i*w] = c_i, and spread of that is the generator's table, above); m ordinary
 * one-term nodes with the tables set[fn*m + i] over y feeding a select node over x give exactly the words of
 * tfhe_gpu_lut_apply2_* for (fn, x, y); a k-digit tree is nested select nodes.
 * In a circuit, node g is a select node iff sel_off[g+1] - sel_off[g] == m (any other non-zero count is invalid);
 * entry j is the constant sel_konst[j] where sel_wire[j] == TFHE_LUT_ENTRY_CONST, and the wire sel_wire[j] otherwise.
 * A select node is single-output (theta = 0) and ignores lut, which must be 0.  Its level is 1 + the largest level
 * among its x-term wires and its entry wires, and it counts as one bootstrap level.  Wires are numbered as in
 * tfhe_gpu_lut_circuit_eval_multi.  A level stages its select nodes' entries, packs and spreads them (in chunks
 * within TFHE_OPT_PACK_SCRATCH_MB), and runs ONE blind-rotation launch over its ordinary and its select nodes: item by
 * item the test vector comes from the set or from the level's own.  A level that also holds theta > 0 nodes runs
 * those and its other ordinary nodes as tfhe_gpu_lut_circuit_eval_multi does, and its select nodes in one launch of
 * their own.  Chunking and launch grouping change no word.  sel_off == NULL runs exactly what the _multi entry runs
 * (pk and m are not looked at).
 * The flat form runs B select nodes over a pool of P ciphertexts, as tfhe_gpu_lut_apply_* stands beside the circuit:
 * node b has the terms term_off[b] .. term_off[b+1] and the m entries sel_src[b*m + i], a pool index or
 * TFHE_LUT_ENTRY_CONST with the constant sel_konst[b*m + i].  It needs no LUT set.
 * Noise rule (the library does not police it): the error of TV_g at the coefficient that is read is the selected
 * entry's own error plus the pack's terms (the bivariate section's: sigma ~ 2e-4 at UINT4 with the default key shape
 * and alpha_lv1); that sum is added to the OUTPUT's error, not to the input rounding, so a chain of k select nodes
 * accumulates k such terms linearly, against a message spacing of 1/(2m), that is, a decision margin of 1/(4m).
 * The warning about packing keys made with alpha_lv0 applies unchanged.  Measured figures: DESIGN.md §4.9d.
 * Checked before any launch or upload (TFHE_ERR_INVALID): everything tfhe_gpu_lut_circuit_eval_multi checks; m not a
 * power of two, m < 2 or 2m > N; a set or a packing key of another context; a null argument; an entry count other
 * than 0 or m; an entry wire that is not an earlier wire (flat form: not in the pool); theta != 0 or lut != 0 on a
 * select node; sel_off not monotone from 0.  TFHE_ERR_NO_KEY without a cloud key; zero nodes is TFHE_OK.  All
 * descriptors are HOST arrays in both variants; the _dev ones take the ciphertexts in HBM, are asynchronous on the
 * context stream and refuse a multi-device context. */
#define TFHE_LUT_ENTRY_CONST 0xFFFFFFFFu
int tfhe_gpu_lut_circuit_eval_select(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk,
                                     uint32_t m, size_t n_inputs, const uint32_t *inputs, size_t n_nodes,
                                     const uint32_t *term_off, const uint32_t *term_wire, const int32_t *term_coef,
                                     const uint32_t *konst, const uint32_t *lut, const uint32_t *theta /*n_nodes or NULL*/,
                                     const uint32_t *sel_off /*n_nodes+1*/, const uint32_t *sel_wire,
                                     const uint32_t *sel_konst, size_t n_outputs, const uint32_t *out_wires,
                                     uint32_t *outputs, uint32_t *levels);
int tfhe_gpu_lut_circuit_eval_select_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk,
                                         uint32_t m, size_t n_inputs, const uint32_t *inputs_dev, size_t n_nodes,
                                         const uint32_t *term_off, const uint32_t *term_wire, const int32_t *term_coef,
                                         const uint32_t *konst, const uint32_t *lut, const uint32_t *theta,
                                         const uint32_t *sel_off, const uint32_t *sel_wire, const uint32_t *sel_konst,
                                         size_t n_outputs, const uint32_t *out_wires, uint32_t *outputs_dev,
                                         uint32_t *levels);
int tfhe_gpu_lut_select_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_packing_key *pk, uint32_t m, const uint32_t *pool,
                              size_t P, const uint32_t *term_off /*B+1*/, const uint32_t *term_src,
                              const int32_t *term_coef, const uint32_t *konst /*B*/, const uint32_t *sel_src /*B*m*/,
                              const uint32_t *sel_konst /*B*m*/, uint32_t *out /*B*(n+1)*/, size_t B);
int tfhe_gpu_lut_select_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_packing_key *pk, uint32_t m, const uint32_t *pool_dev,
                            size_t P, const uint32_t *term_off /*B+1*/, const uint32_t *term_src,
                            const int32_t *term_coef, const uint32_t *konst /*B*/, const uint32_t *sel_src /*B*m*/,
                            const uint32_t *sel_konst /*B*m*/, uint32_t *out_dev, size_t B);
/* host only: the levels and depth of tfhe_gpu_lut_circuit_eval_select under the rule above (levels has n_nodes
 * entries); it checks the wires, the offsets, the entry counts against m (a power of two >= 2) and theta on select
 * nodes.  sel_off == NULL is tfhe_lut_circuit_schedule_multi. */
int tfhe_lut_circuit_schedule_select(size_t n_inputs, size_t n_nodes, const uint32_t *term_off,
                                     const uint32_t *term_wire, const uint32_t *theta /*n_nodes or NULL*/, uint32_t m,
                                     const uint32_t *sel_off /*n_nodes+1*/, const uint32_t *sel_wire, uint32_t *levels,
                                     uint32_t *depth);

/* ---- Extended nodes: an eta per LUT-circuit node, select nodes of up to N/2 entries ----
 * The extended bootstrap as a property of a circuit node, ordinary or select, so that radix-32 and radix-64 digits
 * and reads of a 32- or 64-entry encrypted table share a circuit's per-level launches.
 * The identity the select form rests on: where 2m <= N, every component of tfhe_lut_generate_ext(eta, m, f) equals
 * tfhe_lut_generate(m, f) word for word (a block of N E / m positions covers whole groups of E; at m = N and 2N it does
 * not hold).  The same algebra holds for an encrypted table: m entries packed at the coefficients i*w of component 0
 * and spread in the extended ring, with the generator's window (w = N/m, off_ext = (w/2) E, a multiple of E), put the
 * window sum into every component, and the extended rotation by 2N E - off_ext is polyMulWithXK(., 2N - w/2) on each.
 * So the extended test vector of a select node is E copies of the ordinary tfhe_lut_spread(P, w, 2N - off).
 *   each_ext: output i of tfhe_gpu_bootstrap_lut_each_ext_* is, word for word, the extended bootstrap of "Extended LUT
 *     bootstrap" for in[i] with tv_j = testvecs[i] (one TRLWELv1, any a) for every j < E: the blind rotation, then
 *     sampleExtractIndex(acc_0, 0), then identityKeySwitching.  eta = 0 runs exactly tfhe_gpu_bootstrap_lut_each_*.
 *   select_ext: node b of tfhe_gpu_lut_select_ext_*, with x_b, the entries and m as tfhe_gpu_lut_select_* has them:
 *       1. P_b  = tfhe_pack_tlwe(e_b[0 .. m), coef[i] = i*w, C = m);
 *       2. TV_b = tfhe_lut_spread(P_b, w, 2N - off);
 *       3. out_b = the tfhe_gpu_bootstrap_lut_each_ext_* output for x_b with TV_b.
 *     eta = 0 runs exactly tfhe_gpu_lut_select_*.
 *   circuit: tfhe_gpu_lut_circuit_eval_ext* is tfhe_gpu_lut_circuit_eval_select* with one more HOST array, eta[g] per
 *     node (NULL: exactly what the _select entry runs).  An ordinary node with eta[g] > 0 gives the words of
 *     tfhe_gpu_lut_apply_ext_* for its combination and the extended table lut[g], the entries set[lut[g] E_g + j]; a
 *     select node with eta[g] > 0 gives the words of tfhe_gpu_lut_select_ext_*.  Levels, wire numbering and the
 *     outputs' order are the _select entry's: eta does not change a node's level.  A level runs one staging, pack and
 *     spread over all of its select nodes whatever their eta (chunked within TFHE_OPT_PACK_SCRATCH_MB), its eta = 0
 *     nodes exactly as the _select entry runs them (the theta > 0 handling included), one combination launch over the
 *     rest of its nodes, ONE extended blind rotation per eta in {1, 2} present, over that eta's ordinary and select
 *     nodes together (item by item the test vector is the set's extended table or the level's own), one extraction of
 *     those accumulators (acc_0 only, 2N words per item) and ONE key switch over them into the level's output slots.
 *     A group with no nodes launches nothing; grouping and chunking change no word.
 * Noise rule: "Extended LUT bootstrap" for the input side, "Select nodes" for the table's own error; at UINT4, m = 64
 * leaves an output 5.2 sigma and a chained input about 3.8 sigma: feed m = 64 nodes fresh inputs.
 * Checked before any launch or upload (TFHE_ERR_INVALID): an eta > TFHE_LUT_EXT_MAX_LOG; eta > 0 with theta > 0 on one
 * node; a lut[g] E_g + E_g beyond the set on an ordinary node; everything the entry without eta checks.
 * TFHE_ERR_NO_KEY, zero nodes and the multi-device refusal as there. */
int tfhe_gpu_bootstrap_lut_each_ext_batch(tfhe_gpu_ctx *ctx, uint32_t eta, const uint32_t *in /*B*(n+1)*/,
                                          const uint32_t *testvecs /*B*2N*/, uint32_t *out /*B*(n+1)*/, size_t B);
int tfhe_gpu_bootstrap_lut_each_ext_dev(tfhe_gpu_ctx *ctx, uint32_t eta, const uint32_t *in_dev,
                                        const uint32_t *testvecs_dev, uint32_t *out_dev, size_t B);
int tfhe_gpu_lut_select_ext_batch(tfhe_gpu_ctx *ctx, const tfhe_gpu_packing_key *pk, uint32_t m, uint32_t eta,
                                  const uint32_t *pool, size_t P, const uint32_t *term_off /*B+1*/,
                                  const uint32_t *term_src, const int32_t *term_coef, const uint32_t *konst /*B*/,
                                  const uint32_t *sel_src /*B*m*/, const uint32_t *sel_konst /*B*m*/,
                                  uint32_t *out /*B*(n+1)*/, size_t B);
int tfhe_gpu_lut_select_ext_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_packing_key *pk, uint32_t m, uint32_t eta,
                                const uint32_t *pool_dev, size_t P, const uint32_t *term_off /*B+1*/,
                                const uint32_t *term_src, const int32_t *term_coef, const uint32_t *konst /*B*/,
                                const uint32_t *sel_src /*B*m*/, const uint32_t *sel_konst /*B*m*/, uint32_t *out_dev,
                                size_t B);
int tfhe_gpu_lut_circuit_eval_ext(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk,
                                  uint32_t m, size_t n_inputs, const uint32_t *inputs, size_t n_nodes,
                                  const uint32_t *term_off, const uint32_t *term_wire, const int32_t *term_coef,
                                  const uint32_t *konst, const uint32_t *lut, const uint32_t *theta /*n_nodes or NULL*/,
                                  const uint32_t *sel_off /*n_nodes+1 or NULL*/, const uint32_t *sel_wire,
                                  const uint32_t *sel_konst, const uint32_t *eta /*n_nodes or NULL*/, size_t n_outputs,
                                  const uint32_t *out_wires, uint32_t *outputs, uint32_t *levels);
int tfhe_gpu_lut_circuit_eval_ext_dev(tfhe_gpu_ctx *ctx, const tfhe_gpu_lut_set *set, const tfhe_gpu_packing_key *pk,
                                      uint32_t m, size_t n_inputs, const uint32_t *inputs_dev, size_t n_nodes,
                                      const uint32_t *term_off, const uint32_t *term_wire, const int32_t *term_coef,
                                      const uint32_t *konst, const uint32_t *lut, const uint32_t *theta,
                                      const uint32_t *sel_off, const uint32_t *sel_wire, const uint32_t *sel_konst,
                                      const uint32_t *eta, size_t n_outputs, const uint32_t *out_wires,
                                      uint32_t *outputs_dev, uint32_t *levels);
/* host only: tfhe_lut_circuit_schedule_select plus eta (NULL: exactly that call's levels and depth).  group_nodes
 * (may be NULL; room for 3 * n_nodes words, 3 * depth are written) receives, per level lv = 1 .. depth, the node
 * counts of its eta = 0, 1 and 2 groups at [3 (lv-1) + eta]: the grouping tfhe_gpu_lut_circuit_eval_ext runs.
 * TFHE_ERR_INVALID for an eta > TFHE_LUT_EXT_MAX_LOG, eta > 0 with theta > 0 on one node, and what the _select
 * schedule refuses. */
int tfhe_lut_circuit_schedule_ext(size_t n_inputs, size_t n_nodes, const uint32_t *term_off, const uint32_t *term_wire,
                                  const uint32_t *theta /*n_nodes or NULL*/, uint32_t m,
                                  const uint32_t *sel_off /*n_nodes+1 or NULL*/, const uint32_t *sel_wire,
                                  const uint32_t *eta /*n_nodes or NULL*/, uint32_t *levels, uint32_t *depth,
                                  uint32_t *group_nodes);

/* ---- Host-side TLWELv0 helpers (no device needed) ---------------------- */
/* Host only: entry e of a lookup table as a trivial TRLWELv1 (a = 0, the form of the reference's test vectors,
 * key.zig:134-145): coefficient c < width = +1/8 if bit c of values[e] is set, else -1/8; coefficients >= width
 * are 0.  width <= N (bits past 63 read as clear). */
int tfhe_lookup_table_pack_bits(const tfhe_params *params, const uint64_t *values, size_t entries, uint32_t width,
                                uint32_t *table /*entries*2N*/);
/* Host only: the packed table of tfhe_gpu_packed_lookup_* from 2^k values of `width` <= 64 bits: trlwes * 2N
 * words (tfhe_packed_lookup_plan), trivial TRLWELv1 (a = 0), +-1/8 per bit as above, unused coefficients 0. */
int tfhe_lookup_table_pack_slots(const tfhe_params *params, const uint64_t *values /*2^k*/, uint32_t k, uint32_t width,
                                 uint32_t *table /*trlwes*2N*/);
/* genDecompositionOffset (key.zig:121-131): sum over l < L of Bg/2 * 2^(32 - (l+1) bgbit), the
 * CloudKey.decomposition_offset that tfhe_gpu_load_cloud_key takes. */
int tfhe_decomposition_offset(const tfhe_params *params, uint32_t *offset);
/* SecretKey.new (key.zig:41-57) from DefaultPrng(seed): n lv0 bits, then N lv1 bits. */
int tfhe_secret_key_new(const tfhe_params *params, uint64_t seed, uint32_t *key_lv0, uint32_t *key_lv1);
/* TLWELv0.encryptBool (tlwe.zig:52-55 -> encryptF64 :34-49); item i uses
 * DefaultPrng(seed0 + i) in place of getUniqueSeed(). */
int tfhe_encrypt_bool_batch(const tfhe_params *params, const uint32_t *key_lv0, const uint8_t *bits,
                            uint64_t seed0, uint32_t *out, size_t B);
/* TLWELv0.decryptBool (tlwe.zig:58-68). */
int tfhe_decrypt_bool_batch(const tfhe_params *params, const uint32_t *key_lv0, const uint32_t *ct,
                            uint8_t *bits, size_t B);
/* encryptLweMessage / decryptLweMessage (tlwe.zig:74-117), message modulus m. */
int tfhe_encrypt_lwe_message_batch(const tfhe_params *params, const uint32_t *key_lv0,
                                   const uint32_t *msgs, uint32_t m, uint64_t seed0, uint32_t *out,
                                   size_t B);
int tfhe_decrypt_lwe_message_batch(const tfhe_params *params, const uint32_t *key_lv0,
                                   const uint32_t *ct, uint32_t m, uint32_t *msgs, size_t B);
/* Proxy re-encryption key material (host, seeded; the reference's
 * getUniqueSeed() for the k-th encryptF64 call of a routine becomes seed0 + k).
 * PublicKeyLv0.newWithParams (proxy_reenc.zig:57-76): `size` encryptions of 0. */
int tfhe_public_key_gen(const tfhe_params *params, const uint32_t *key_lv0, size_t size, double alpha,
                        uint64_t seed0, uint32_t *pk /* size*(n+1) */);
/* PublicKeyLv0.encryptBool (proxy_reenc.zig:83-120), one DefaultPrng(seed0 + i) per item. */
int tfhe_public_key_encrypt_bool_batch(const tfhe_params *params, const uint32_t *pk, size_t pk_size,
                                       const uint8_t *bits, double alpha, uint64_t seed0, uint32_t *out,
                                       size_t B);
/* ProxyReencryptionKey.newSymmetricWithParams (:214-256) / newAsymmetricWithParams
 * (:150-196); out: n*t*2^basebit*(n+1) words, k = 0 entries zero. */
int tfhe_reenc_key_gen_symmetric(const tfhe_params *params, const uint32_t *key_from, const uint32_t *key_to,
                                 double alpha, uint32_t basebit, uint32_t t, uint64_t seed0, uint32_t *out);
int tfhe_reenc_key_gen_asymmetric(const tfhe_params *params, const uint32_t *key_from, const uint32_t *pk,
                                  size_t pk_size, double alpha, uint32_t basebit, uint32_t t, uint64_t seed0,
                                  uint32_t *out);
/* Generator.generateLookupTableAssign (lut/generator.zig:85-135): testvec
 * (2N words, a = 0) for f given as a table f_table[x], x < m, encoded by
 * Encoder.new(m) (scale 1/(2m), encoder.zig:29-42).  1 <= m <= TFHE_LUT_MAX_M
 * (TFHE_ERR_INVALID outside; m > N leaves some messages' ranges empty, as the
 * reference's divRound ranges do).  testvec must hold 2N words. */
#define TFHE_LUT_MAX_M (1u << 24)
int tfhe_lut_generate(const tfhe_params *params, uint32_t m, const uint32_t *f_table,
                      uint32_t *testvec);
/* The same with Encoder.withScale(m, scale) (Generator.withScale, generateLookupTableCustom;
 * generator.zig:47-56, :202-213).  (ABI 6) */
int tfhe_lut_generate_scaled(const tfhe_params *params, uint32_t m, double scale, const uint32_t *f_table,
                             uint32_t *testvec);
/* generateLookupTableFull (generator.zig:144-191): values[x] is message x's Torus value as is.  (ABI 6) */
int tfhe_lut_generate_full(const tfhe_params *params, uint32_t m, const uint32_t *values, uint32_t *testvec);

#ifdef __cplusplus
}
#endif
#endif /* TFHE_GPU_H */
