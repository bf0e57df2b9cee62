// tfhe.hpp — C++ host-side mirror of zig-tfhe's public surface for the gate
// bootstrap path, over the C ABI (include/tfhe_gpu.h).  Header-only; link
// libtfhe_gpu.so.  Names and argument meaning follow the reference:
//   params.zig        -> tfhe::params::SECURITY_128_BIT() / SECURITY_80_BIT() / SECURITY_UINT4()
//   tlwe.zig TLWELv0  -> tfhe::TLWELv0 (p[n+1], b() last; encryptBool / decryptBool / neg / add / sub)
//   key.zig           -> tfhe::SecretKey, tfhe::CloudKey (device resident; keygen or load of host arrays)
//   bootstrap.zig     -> tfhe::HipBootstrap (bootstrap / bootstrapWithoutKeySwitch / name)
//   gates.zig Gates   -> tfhe::Gates (nandGate ... orYnGate, muxNaive, notGate, copy, constant,
//                        batchNand ... batchXnor — placeholders in the reference, implemented here)
//   proxy_reenc.zig   -> tfhe::PublicKeyLv0, tfhe::ProxyReencryptionKey, tfhe::HipReencryptor
//                        (reencryptTLWELv0 on the GPU)
//   trlwe.zig         -> tfhe::TRLWELv1 (encryptF64 / encryptBool / decryptBool, sampleExtractIndex)
//   trgsw.zig         -> tfhe::TRGSWLv1FFT::encryptTorus (encryptTorus + TRGSWLv1FFT.new), tfhe::cmux, tfhe::rotateByBits,
//                        tfhe::TrgswSet and tfhe::TableLookup (a table addressed by TRGSW-encrypted bits),
//                        tfhe::PackingKey / tfhe::packTlwe (identityKeySwitching's arithmetic with TRLWE rows),
//                        tfhe::packedScatterAdd / tfhe::packedWrite (writes into a tfhe::PackedTableLookup)
//   lut/generator.zig -> tfhe::lutGenerate, tfhe::LutSet / tfhe::LutCircuit (per-item tables), tfhe::lutInterleave
//                        (several tables from one blind rotation; LutCircuit::select / node2 and tfhe::lutSelect:
//                        nodes whose table is made of wires), tfhe::lutGenerate2 / tfhe::lutApply2 /
//                        tfhe::lutSpread / tfhe::bootstrapLutEach (functions of two digits: a test vector
//                        packed and spread on the device per item), tfhe::lutGenerateExt / tfhe::blindRotateExt /
//                        tfhe::lutApplyExt (5- and 6-bit digits: the blind rotation on 2^eta components)
// Zig error unions become tfhe::Error exceptions carrying the C status.
// There is no CPU path: every bootstrap runs on the GPU through the C ABI.
#pragma once

#include <tfhe_gpu.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace tfhe {

using Torus = uint32_t;

class Error : public std::runtime_error {
  public:
    Error(int status, const std::string &what) : std::runtime_error(what), status(status) {}
    int status;
};

inline void check(int rc, const char *what, const tfhe_gpu_ctx *ctx = nullptr) {
    if (rc != TFHE_OK)
        throw Error(rc, std::string(what) + ": status " + std::to_string(rc) +
                            (ctx ? std::string(": ") + tfhe_gpu_last_error(ctx) : std::string()));
}

// params.zig:70-95, 350-375, 210-235; KSK/BSK alphas as the Python mirror
// (tfhe_amd.SECURITY_*): the 128-bit constants params.zig:419-422, and BSK
// noise 0 for UINT4
namespace params {
inline tfhe_params SECURITY_128_BIT() {
    return tfhe_params{700, 1024, 10, 3, 6, 2, 9, 0, 2.0e-5, 2.0e-8, 2.0e-5, 2.0e-8};
}
inline tfhe_params SECURITY_80_BIT() {
    return tfhe_params{550, 1024, 10, 3, 6, 2, 7, 0, 5.0e-5, 3.73e-8, 2.0e-5, 2.0e-8};
}
inline tfhe_params SECURITY_UINT4() {
    return tfhe_params{820, 1024, 10, 1, 22, 5, 3, 0, 0.00000251676160959795544987084234,
                       0.00000000000000022204460492503131, 0.00000251676160959795544987084234, 0.0};
}
}  // namespace params

// tlwe.zig:11-239
struct TLWELv0 {
    std::vector<Torus> p;  // a[0..n) then b
    TLWELv0() = default;
    explicit TLWELv0(size_t n) : p(n + 1, 0u) {}
    size_t n() const { return p.size() - 1; }
    Torus b() const { return p.back(); }
    Torus &bMut() { return p.back(); }
    TLWELv0 neg() const {  // tlwe.zig:160-177
        TLWELv0 r(n());
        for (size_t i = 0; i < p.size(); i++) r.p[i] = 0u - p[i];
        return r;
    }
    TLWELv0 add(const TLWELv0 &o) const {
        TLWELv0 r(n());
        for (size_t i = 0; i < p.size(); i++) r.p[i] = p[i] + o.p[i];
        return r;
    }
    TLWELv0 sub(const TLWELv0 &o) const {
        TLWELv0 r(n());
        for (size_t i = 0; i < p.size(); i++) r.p[i] = p[i] - o.p[i];
        return r;
    }
};

// key.zig:33-57: binary lv0 / lv1 keys
struct SecretKey {
    tfhe_params params{};
    std::vector<Torus> key_lv0, key_lv1;

    // TLWELv0.encryptBool (tlwe.zig:52-56) with a seeded DefaultPrng
    TLWELv0 encryptBool(bool bit, uint64_t seed) const {
        TLWELv0 ct(params.n);
        const uint8_t v = bit ? 1 : 0;
        check(tfhe_encrypt_bool_batch(&params, key_lv0.data(), &v, seed, ct.p.data(), 1), "encryptBool");
        return ct;
    }
    bool decryptBool(const TLWELv0 &ct) const {  // tlwe.zig:58-68
        uint8_t v = 0;
        check(tfhe_decrypt_bool_batch(&params, key_lv0.data(), ct.p.data(), &v, 1), "decryptBool");
        return v != 0;
    }
    TLWELv0 encryptLweMessage(uint32_t msg, uint32_t m, uint64_t seed) const {  // tlwe.zig:74-97
        TLWELv0 ct(params.n);
        check(tfhe_encrypt_lwe_message_batch(&params, key_lv0.data(), &msg, m, seed, ct.p.data(), 1),
              "encryptLweMessage");
        return ct;
    }
    uint32_t decryptLweMessage(const TLWELv0 &ct, uint32_t m) const {  // tlwe.zig:100-117
        uint32_t v = 0;
        check(tfhe_decrypt_lwe_message_batch(&params, key_lv0.data(), ct.p.data(), m, &v, 1), "decryptLweMessage");
        return v;
    }
    // SecretKey.new (key.zig:41-57) from DefaultPrng(seed)
    static SecretKey newWithSeed(const tfhe_params &p, uint64_t seed) {
        SecretKey sk;
        sk.params = p;
        sk.key_lv0.assign(p.n, 0u);
        sk.key_lv1.assign(p.N, 0u);
        check(tfhe_secret_key_new(&p, seed, sk.key_lv0.data(), sk.key_lv1.data()), "SecretKey.new");
        return sk;
    }
};

// proxy_reenc.zig:35-121.  Encryption e of newWithParams uses DefaultPrng(seed0 + e).
struct PublicKeyLv0 {
    tfhe_params params{};
    size_t size = 0;
    std::vector<Torus> encryptions;  // size x (n+1)

    static PublicKeyLv0 newWithParams(const SecretKey &sk, size_t size, double alpha, uint64_t seed0) {
        PublicKeyLv0 pk;
        pk.params = sk.params;
        pk.size = size;
        pk.encryptions.assign(size * (sk.params.n + 1), 0u);
        check(tfhe_public_key_gen(&sk.params, sk.key_lv0.data(), size, alpha, seed0, pk.encryptions.data()),
              "PublicKeyLv0.new");
        return pk;
    }
    static PublicKeyLv0 create(const SecretKey &sk, uint64_t seed0) {  // PublicKeyLv0.new: 2n, tlwe_lv0.ALPHA
        return newWithParams(sk, 2 * (size_t)sk.params.n, sk.params.alpha_lv0, seed0);
    }
    TLWELv0 encryptBool(bool bit, double alpha, uint64_t seed) const {  // :116-120
        TLWELv0 ct(params.n);
        const uint8_t v = bit ? 1 : 0;
        check(tfhe_public_key_encrypt_bool_batch(&params, encryptions.data(), size, &v, alpha, seed, ct.p.data(), 1),
              "PublicKeyLv0.encryptBool");
        return ct;
    }
};

// proxy_reenc.zig:124-257: key_encryptions[(base*t*i)+(base*j)+k]; the c-th encryption uses seed0 + c.
struct ProxyReencryptionKey {
    std::vector<Torus> key_encryptions;
    uint32_t basebit = 0, t = 0;
    size_t base() const { return (size_t)1 << basebit; }

    static ProxyReencryptionKey newSymmetricWithParams(const SecretKey &from, const SecretKey &to, double alpha,
                                                       uint32_t basebit, uint32_t t, uint64_t seed0) {
        ProxyReencryptionKey k = shaped(from.params, basebit, t);
        check(tfhe_reenc_key_gen_symmetric(&from.params, from.key_lv0.data(), to.key_lv0.data(), alpha, basebit, t,
                                           seed0, k.key_encryptions.data()),
              "ProxyReencryptionKey.newSymmetric");
        return k;
    }
    static ProxyReencryptionKey newAsymmetricWithParams(const SecretKey &from, const PublicKeyLv0 &to, double alpha,
                                                        uint32_t basebit, uint32_t t, uint64_t seed0) {
        ProxyReencryptionKey k = shaped(from.params, basebit, t);
        check(tfhe_reenc_key_gen_asymmetric(&from.params, from.key_lv0.data(), to.encryptions.data(), to.size, alpha,
                                            basebit, t, seed0, k.key_encryptions.data()),
              "ProxyReencryptionKey.newAsymmetric");
        return k;
    }
    // newSymmetric / newAsymmetric: KSK_ALPHA and the set's BASEBIT / IKS_T (:131-147, :199-212)
    static ProxyReencryptionKey newSymmetric(const SecretKey &from, const SecretKey &to, uint64_t seed0) {
        return newSymmetricWithParams(from, to, from.params.alpha_ksk, from.params.basebit, from.params.iks_t, seed0);
    }
    static ProxyReencryptionKey newAsymmetric(const SecretKey &from, const PublicKeyLv0 &to, uint64_t seed0) {
        return newAsymmetricWithParams(from, to, from.params.alpha_ksk, from.params.basebit, from.params.iks_t, seed0);
    }

  private:
    static ProxyReencryptionKey shaped(const tfhe_params &p, uint32_t basebit, uint32_t t) {
        ProxyReencryptionKey k;
        k.basebit = basebit;
        k.t = t;
        k.key_encryptions.assign(((size_t)p.n * t << basebit) * (p.n + 1), 0u);
        return k;
    }
};

// key.zig:61-118.  The cloud key lives in HBM inside one GPU context.
class CloudKey {
  public:
    // CloudKey.new (key.zig:70-77) from a seeded SecretKey.new: keys generated
    // with the restated DefaultPrng order, FFTs on the GPU.
    static std::pair<SecretKey, CloudKey> generate(const tfhe_params &p, uint64_t secret_seed, uint64_t cloud_seed,
                                                   int device = 0) {
        CloudKey ck(p, device);
        SecretKey sk;
        sk.params = p;
        sk.key_lv0.assign(p.n, 0u);
        sk.key_lv1.assign(p.N, 0u);
        check(tfhe_gpu_keygen(ck.ctx(), secret_seed, cloud_seed, sk.key_lv0.data(), sk.key_lv1.data(), nullptr,
                              nullptr),
              "CloudKey.generate", ck.ctx());
        return {std::move(sk), std::move(ck)};
    }
    // An existing CloudKey in the reference's host layout (decomposition_offset,
    // blind_rotate_testvec, bootstrapping_key.items, key_switching_key.items).
    static CloudKey load(const tfhe_params &p, Torus offset, const std::vector<Torus> &testvec_a,
                         const std::vector<Torus> &testvec_b, const std::vector<double> &bsk,
                         const std::vector<Torus> &ksk, int device = 0) {
        CloudKey ck(p, device);
        check(tfhe_gpu_load_cloud_key(ck.ctx(), offset, testvec_a.data(), testvec_b.data(), bsk.data(), bsk.size(),
                                      ksk.data(), ksk.size()),
              "CloudKey.load", ck.ctx());
        return ck;
    }
    // Key files (include/tfhe_gpu.h "Cloud-key files"): the reference has no
    // serialization; a saved key reloads bit-exact on any device.
    static CloudKey loadFile(const tfhe_params &p, const std::string &path, int device = 0) {
        CloudKey ck(p, device);
        check(tfhe_gpu_load_cloud_key_file(ck.ctx(), path.c_str()), "CloudKey.loadFile", ck.ctx());
        return ck;
    }
    // The same key resident on several GPUs (tfhe_gpu_create_multi): loaded on the
    // first, broadcast over RCCL; every batch call through it is sharded over them.
    static CloudKey loadFile(const tfhe_params &p, const std::string &path, const std::vector<int> &devices) {
        CloudKey ck(p, devices);
        check(tfhe_gpu_load_cloud_key_file(ck.ctx(), path.c_str()), "CloudKey.loadFile", ck.ctx());
        return ck;
    }
    static std::pair<SecretKey, CloudKey> generate(const tfhe_params &p, uint64_t secret_seed, uint64_t cloud_seed,
                                                   const std::vector<int> &devices) {
        CloudKey ck(p, devices);
        SecretKey sk;
        sk.params = p;
        sk.key_lv0.assign(p.n, 0u);
        sk.key_lv1.assign(p.N, 0u);
        check(tfhe_gpu_keygen(ck.ctx(), secret_seed, cloud_seed, sk.key_lv0.data(), sk.key_lv1.data(), nullptr,
                              nullptr),
              "CloudKey.generate", ck.ctx());
        return {std::move(sk), std::move(ck)};
    }
    // CloudKey.newNoKsk (key.zig:80-89): no bootstrapping or key-switching key; what the leveled
    // operations (cmux, TableLookup, the TRLWE / TRGSW encryptions) need, the decomposition offset,
    // comes from the parameter set.
    static CloudKey newNoKsk(const tfhe_params &p, int device = 0) { return CloudKey(p, device); }
    int numDevices() const { return tfhe_gpu_num_devices(ctx()); }
    void save(const std::string &path) const {
        check(tfhe_gpu_save_cloud_key(ctx(), path.c_str()), "CloudKey.save", ctx());
    }
    tfhe_gpu_ctx *ctx() const { return ctx_.get(); }
    const tfhe_params &params() const { return p_; }

  private:
    struct Del {
        void operator()(tfhe_gpu_ctx *c) const { tfhe_gpu_destroy(c); }
    };
    CloudKey(const tfhe_params &p, int device) : p_(p) {
        tfhe_gpu_ctx *c = nullptr;
        check(tfhe_gpu_create_on_device(&p, device, &c), "tfhe_gpu_create_on_device");
        ctx_.reset(c);
    }
    CloudKey(const tfhe_params &p, const std::vector<int> &devices) : p_(p) {
        tfhe_gpu_ctx *c = nullptr;
        check(tfhe_gpu_create_multi(&p, (int)devices.size(), devices.data(), &c), "tfhe_gpu_create_multi");
        ctx_.reset(c);
    }
    tfhe_params p_{};
    std::unique_ptr<tfhe_gpu_ctx, Del> ctx_;
};

// trlwe.zig:15-162.  Polynomial products run on the GPU of `ck`'s context (the reference passes an FFT plan).
struct TRLWELv1 {
    std::vector<Torus> p;  // a[N] then b[N]
    TRLWELv1() : p(2 * 1024, 0u) {}
    // encryptF64 (trlwe.zig:30-64) with DefaultPrng(seed)
    static TRLWELv1 encryptF64(const std::vector<double> &mu, double alpha, const std::vector<Torus> &key_lv1,
                               const CloudKey &ck, uint64_t seed) {
        TRLWELv1 ct;
        if (mu.size() != ck.params().N) throw Error(TFHE_ERR_INVALID, "TRLWELv1.encryptF64: N plaintext values");
        check(tfhe_gpu_trlwe_encrypt_batch(ck.ctx(), key_lv1.data(), mu.data(), alpha, seed, ct.p.data(), 1),
              "TRLWELv1.encryptF64", ck.ctx());
        return ct;
    }
    // encryptBool (trlwe.zig:67-79): +-1/8 per coefficient
    static TRLWELv1 encryptBool(const std::vector<bool> &bits, double alpha, const std::vector<Torus> &key_lv1,
                                const CloudKey &ck, uint64_t seed) {
        std::vector<double> mu(bits.size());
        for (size_t i = 0; i < bits.size(); i++) mu[i] = bits[i] ? 0.125 : -0.125;
        return encryptF64(mu, alpha, key_lv1, ck, seed);
    }
    std::vector<bool> decryptBool(const std::vector<Torus> &key_lv1, const CloudKey &ck) const {  // trlwe.zig:85-98
        std::vector<uint8_t> v(ck.params().N);
        check(tfhe_gpu_trlwe_decrypt_bool_batch(ck.ctx(), key_lv1.data(), p.data(), v.data(), 1), "TRLWELv1.decryptBool",
              ck.ctx());
        return std::vector<bool>(v.begin(), v.end());
    }
    // sampleExtractIndex (trlwe.zig:146-162): the TLWELv1 (N + 1 words) of coefficient k
    std::vector<Torus> sampleExtractIndex(uint32_t k, const CloudKey &ck) const {
        std::vector<Torus> out(ck.params().N + 1);
        check(tfhe_gpu_sample_extract_batch(ck.ctx(), p.data(), &k, 1, 0, out.data(), 1), "sampleExtractIndex", ck.ctx());
        return out;
    }
};

// Selectors resident in HBM (tfhe_gpu_trgsw_set): S TRGSWLv1FFT in the reference layout, 2L*2*N doubles each.
class TrgswSet {
  public:
    TrgswSet(const CloudKey &ck, const std::vector<double> &trgsw_fft, size_t S) : size_(S) {
        tfhe_gpu_trgsw_set *h = nullptr;
        const tfhe_params &p = ck.params();
        if (trgsw_fft.size() != S * 2 * p.L * 2 * p.N) throw Error(TFHE_ERR_INVALID, "TrgswSet: S*2L*2*N doubles");
        check(tfhe_gpu_trgsw_set_load(ck.ctx(), trgsw_fft.data(), S, &h), "trgsw_set_load", ck.ctx());
        set_.reset(h, tfhe_gpu_trgsw_set_destroy);
    }
    const tfhe_gpu_trgsw_set *get() const { return set_.get(); }
    size_t size() const { return size_; }

  private:
    std::shared_ptr<tfhe_gpu_trgsw_set> set_;
    size_t size_ = 0;
};

// trgsw.zig:75-91: a TRGSW in the frequency domain; here also resident on the GPU as a set of one.
struct TRGSWLv1FFT {
    std::vector<double> fft;  // [2L][2][N], trgsw.zig:75-77
    std::shared_ptr<TrgswSet> resident;
    // TRGSWLv1.encryptTorus (trgsw.zig:35-71) + TRGSWLv1FFT.new (:81-91); DefaultPrng(seed) supplies the row seeds
    static TRGSWLv1FFT encryptTorus(Torus mu, double alpha, const std::vector<Torus> &key_lv1, const CloudKey &ck,
                                    uint64_t seed) {
        TRGSWLv1FFT t;
        const tfhe_params &p = ck.params();
        t.fft.assign((size_t)2 * p.L * 2 * p.N, 0.0);
        check(tfhe_gpu_trgsw_encrypt_batch(ck.ctx(), key_lv1.data(), &mu, alpha, seed, t.fft.data(), 1),
              "TRGSWLv1.encryptTorus", ck.ctx());
        t.resident = std::make_shared<TrgswSet>(ck, t.fft, 1);
        return t;
    }
};

// trgsw.cmux (trgsw.zig:260-284): if cond == 0 then in1 else in2.
inline TRLWELv1 cmux(const TRLWELv1 &in1, const TRLWELv1 &in2, const TRGSWLv1FFT &cond, const CloudKey &ck) {
    TRLWELv1 out;
    const uint32_t sel = 0;
    check(tfhe_gpu_cmux_batch(ck.ctx(), cond.resident->get(), &sel, in1.p.data(), in2.p.data(), out.p.data(), 1), "cmux",
          ck.ctx());
    return out;
}

// A table of 2^k TRLWELv1 addressed by k TRGSW-encrypted bits per query (tfhe_gpu_table_lookup_batch: a tree
// of trgsw.cmux), and the extraction of its outputs' coefficients as gate inputs.
struct TableLookup {
    std::vector<Torus> table;  // 2^k x 2N
    uint32_t k = 0;
    // entry e = values[e]'s low `width` bits as +-1/8 coefficients of a trivial TRLWE (tfhe_lookup_table_pack_bits)
    static TableLookup fromBits(const tfhe_params &p, const std::vector<uint64_t> &values, uint32_t width) {
        TableLookup t;
        while (((size_t)1 << t.k) < values.size()) t.k++;
        if (values.size() != (size_t)1 << t.k || t.k < 1) throw Error(TFHE_ERR_INVALID, "TableLookup: 2^k entries, k >= 1");
        t.table.assign(values.size() * 2 * p.N, 0u);
        check(tfhe_lookup_table_pack_bits(&p, values.data(), values.size(), width, t.table.data()), "pack_bits");
        return t;
    }
    // addr[q * k + j]: the selector of `set` that encrypts bit j (least significant first) of query q's address
    std::vector<TRLWELv1> lookup(const CloudKey &ck, const TrgswSet &set, const std::vector<uint32_t> &addr) const {
        const size_t Q = addr.size() / k, w = 2 * (size_t)ck.params().N;
        std::vector<Torus> out(Q * w);
        check(tfhe_gpu_table_lookup_batch(ck.ctx(), set.get(), addr.data(), k, table.data(), out.data(), Q), "table_lookup",
              ck.ctx());
        std::vector<TRLWELv1> r(Q);
        for (size_t q = 0; q < Q; q++) std::copy(out.begin() + q * w, out.begin() + (q + 1) * w, r[q].p.begin());
        return r;
    }
    // coefficients coef[] of one output as TLWELv0 (sampleExtractIndex + identityKeySwitching; needs the cloud key)
    static std::vector<TLWELv0> extractBits(const CloudKey &ck, const TRLWELv1 &ct, const std::vector<uint32_t> &coef) {
        const size_t w = ck.params().n + 1;
        std::vector<Torus> out(coef.size() * w);
        check(tfhe_gpu_sample_extract_batch(ck.ctx(), ct.p.data(), coef.data(), coef.size(), 1, out.data(), 1),
              "sample_extract", ck.ctx());
        std::vector<TLWELv0> r(coef.size(), TLWELv0(ck.params().n));
        for (size_t c = 0; c < coef.size(); c++) std::copy(out.begin() + c * w, out.begin() + (c + 1) * w, r[c].p.begin());
        return r;
    }
};

// Rotation by encrypted bits (tfhe_gpu_rotate_by_bits_batch): for j = 0 .. h-1 in order,
// acc = cmux(acc, (polyMulWithXK(acc.a, rot[j]), polyMulWithXK(acc.b, rot[j])), set[sel[j]]) (trgsw.zig:260-284, :442-466).
inline TRLWELv1 rotateByBits(const TRLWELv1 &in, const std::vector<uint32_t> &rot, const TrgswSet &set,
                             const std::vector<uint32_t> &sel, const CloudKey &ck) {
    TRLWELv1 out;
    if (sel.size() != rot.size()) throw Error(TFHE_ERR_INVALID, "rotateByBits: one selector per exponent");
    check(tfhe_gpu_rotate_by_bits_batch(ck.ctx(), set.get(), sel.data(), rot.data(), (uint32_t)rot.size(), in.p.data(),
                                        out.p.data(), 1),
          "rotate_by_bits", ck.ctx());
    return out;
}

// A CMUX graph (tfhe_gpu.h "CMUX graphs"): nLeaves leaves (value ids 0 .. nLeaves-1) and nodes over k encrypted bits,
// node v (id nLeaves + v) = cmux(X^rlo value[lo], X^rhi value[hi], bit var), hi where the bit is 1; children are
// earlier values.  lessThan is the comparator of two nbits-bit numbers over the leaves {0: false, 1: true}
// (boolLeaves): variable 2i is bit nbits-1-i of a, variable 2i+1 that bit of b.
struct CmuxGraph {
    uint32_t k = 0, nLeaves = 0;
    std::vector<uint32_t> var, lo, hi, rlo, rhi, roots;
    CmuxGraph(uint32_t k_, uint32_t leaves) : k(k_), nLeaves(leaves) {}
    uint32_t node(uint32_t v, uint32_t l, uint32_t h, uint32_t rl = 0, uint32_t rh = 0) {
        var.push_back(v), lo.push_back(l), hi.push_back(h), rlo.push_back(rl), rhi.push_back(rh);
        return nLeaves + (uint32_t)var.size() - 1;
    }
    // node(), or lo itself when both sides are the same value
    uint32_t mux(uint32_t v, uint32_t l, uint32_t h) { return l == h ? l : node(v, l, h); }
    static CmuxGraph lessThan(uint32_t nbits) {
        CmuxGraph g(2 * nbits, 2);
        uint32_t rest = 0;  // equal on the bits below: not less
        for (uint32_t i = nbits; i-- > 0;) {
            const uint32_t a0 = g.mux(2 * i + 1, rest, 1), a1 = g.mux(2 * i + 1, 0, rest);
            rest = g.mux(2 * i, a0, a1);
        }
        g.roots.push_back(rest);
        return g;
    }
    // tfhe_cmux_graph_plan: levels, slots, depth and the per-query scratch slots
    struct Plan {
        std::vector<uint32_t> level, slot;
        uint32_t depth = 0, nSlots = 0;
    };
    Plan plan(uint32_t N = 1024) const {
        Plan p;
        p.level.resize(var.size()), p.slot.resize(var.size());
        check(tfhe_cmux_graph_plan(nLeaves, (uint32_t)var.size(), k, var.data(), lo.data(), hi.data(), rlo.data(), rhi.data(),
                                   (uint32_t)roots.size(), roots.data(), N, p.level.data(), p.slot.data(), &p.depth,
                                   &p.nSlots),
              "cmux_graph_plan");
        return p;
    }
    // trivial TRLWEs with -1/8 (leaf 0, false) and +1/8 (leaf 1, true) in every coefficient
    static std::vector<Torus> boolLeaves(const tfhe_params &p) {
        std::vector<Torus> lv(2 * 2 * (size_t)p.N, 0u);
        std::fill(lv.begin() + p.N, lv.begin() + 2 * (size_t)p.N, 0xE0000000u);
        std::fill(lv.begin() + 3 * (size_t)p.N, lv.end(), 0x20000000u);
        return lv;
    }
};

// tfhe_gpu_cmux_graph_batch with extract = 2: the graph's roots for each query (addr[q * g.k + j] the selector of
// variable j), extracted at coefficient 0 and key-switched, Q * R TLWELv0, query-major: ordinary gate inputs.
inline std::vector<TLWELv0> cmuxGraph(const CloudKey &ck, const TrgswSet &set, const std::vector<uint32_t> &addr,
                                      const CmuxGraph &g, const std::vector<Torus> &leaves) {
    const size_t Q = g.k ? addr.size() / g.k : 0, R = g.roots.size(), w = ck.params().n + 1;
    if (leaves.size() != (size_t)g.nLeaves * 2 * ck.params().N) throw Error(TFHE_ERR_INVALID, "cmuxGraph: nLeaves * 2N words");
    std::vector<Torus> out(Q * R * w);
    check(tfhe_gpu_cmux_graph_batch(ck.ctx(), set.get(), addr.data(), g.k, leaves.data(), g.nLeaves, (uint32_t)g.var.size(),
                                    g.var.data(), g.lo.data(), g.hi.data(), g.rlo.data(), g.rhi.data(), (uint32_t)R,
                                    g.roots.data(), 2, out.data(), Q),
          "cmux_graph", ck.ctx());
    std::vector<TLWELv0> r(Q * R, TLWELv0(ck.params().n));
    for (size_t i = 0; i < Q * R; i++) std::copy(out.begin() + i * w, out.begin() + (i + 1) * w, r[i].p.begin());
    return r;
}

class PackingKey;  // below
inline std::vector<TRLWELv1> packTlwe(const CloudKey &ck, const PackingKey &key, const std::vector<TLWELv0> &in,
                               const std::vector<uint32_t> &coef);

// A table of 2^k entries of `width` bits packed side by side into 2^v TRLWELv1 (tfhe_packed_lookup_plan) and addressed
// by k TRGSW-encrypted bits per query: the CMUX tree under the high v bits, then the rotation under the low h
// (tfhe_gpu_packed_lookup_batch), (2^v - 1) + h CMUXes.  TableLookup::extractBits at 0 .. width-1 makes gate inputs.
struct PackedTableLookup {
    std::vector<Torus> table;  // plan.trlwes x 2N
    uint32_t k = 0, width = 0;
    tfhe_packed_plan plan{};
    static PackedTableLookup fromBits(const tfhe_params &p, const std::vector<uint64_t> &values, uint32_t width) {
        PackedTableLookup t;
        while (((size_t)1 << t.k) < values.size()) t.k++;
        if (values.size() != (size_t)1 << t.k || t.k < 1) throw Error(TFHE_ERR_INVALID, "PackedTableLookup: 2^k entries, k >= 1");
        t.width = width;
        check(tfhe_packed_lookup_plan(&p, t.k, width, &t.plan), "packed_lookup_plan");
        t.table.assign((size_t)t.plan.trlwes * 2 * p.N, 0u);
        check(tfhe_lookup_table_pack_slots(&p, values.data(), t.k, width, t.table.data()), "pack_slots");
        return t;
    }
    // the same table from 2^k * width ciphertexts computed on the server (entry-major, then bit), by one
    // packTlwe call: B = plan.trlwes, coef[s * width + c] = s * stride + c
    static PackedTableLookup fromCiphertexts(const CloudKey &ck, const PackingKey &key, const std::vector<TLWELv0> &cts,
                                             uint32_t k, uint32_t width) {
        PackedTableLookup t;
        t.k = k;
        t.width = width;
        check(tfhe_packed_lookup_plan(&ck.params(), k, width, &t.plan), "packed_lookup_plan");
        if (cts.size() != (size_t)width << k) throw Error(TFHE_ERR_INVALID, "PackedTableLookup: 2^k * width ciphertexts");
        std::vector<uint32_t> coef;
        for (uint32_t s = 0; s < 1u << t.plan.h; s++)
            for (uint32_t c = 0; c < width; c++) coef.push_back(s * t.plan.stride + c);
        for (const TRLWELv1 &x : packTlwe(ck, key, cts, coef)) t.table.insert(t.table.end(), x.p.begin(), x.p.end());
        return t;
    }
    // addr[q * k + j]: the selector of `set` that encrypts bit j (least significant first) of query q's address
    std::vector<TRLWELv1> lookup(const CloudKey &ck, const TrgswSet &set, const std::vector<uint32_t> &addr) const {
        const size_t Q = addr.size() / k, w = 2 * (size_t)ck.params().N;
        std::vector<Torus> out(Q * w);
        check(tfhe_gpu_packed_lookup_batch(ck.ctx(), set.get(), addr.data(), k, width, table.data(), out.data(), Q),
              "packed_lookup", ck.ctx());
        std::vector<TRLWELv1> r(Q);
        for (size_t q = 0; q < Q; q++) std::copy(out.begin() + q * w, out.begin() + (q + 1) * w, r[q].p.begin());
        return r;
    }
};

// The packing key (tfhe_gpu_packing_key) of the TLWELv0 -> TRLWELv1 key switch, resident on `ck`'s context:
// generated from the secret key (tfhe_gpu_packing_key_gen, row idx from DefaultPrng(seed0 + idx)) or loaded
// from host rows.  Shapes: basebit 2 with t 7..9, basebit 5 with t 2..3.
class PackingKey {
  public:
    PackingKey(const CloudKey &ck, const std::vector<Torus> &rows, uint32_t basebit, uint32_t t) : basebit_(basebit), t_(t) {
        tfhe_gpu_packing_key *h = nullptr;
        check(tfhe_gpu_packing_key_load(ck.ctx(), rows.data(), rows.size(), basebit, t, &h), "packing_key_load", ck.ctx());
        key_.reset(h, tfhe_gpu_packing_key_destroy);
    }
    static PackingKey generate(const CloudKey &ck, const SecretKey &sk, uint64_t seed0, double alpha, uint32_t basebit,
                               uint32_t t) {
        const tfhe_params &p = ck.params();
        std::vector<Torus> rows(((size_t)p.n * t << basebit) * 2 * p.N);
        check(tfhe_gpu_packing_key_gen(ck.ctx(), sk.key_lv0.data(), sk.key_lv1.data(), alpha, basebit, t, seed0, rows.data()),
              "packing_key_gen", ck.ctx());
        return PackingKey(ck, rows, basebit, t);
    }
    const tfhe_gpu_packing_key *get() const { return key_.get(); }
    uint32_t basebit() const { return basebit_; }
    uint32_t t() const { return t_; }

  private:
    std::shared_ptr<tfhe_gpu_packing_key> key_;
    uint32_t basebit_ = 0, t_ = 0;
};

// tfhe_gpu_pack_tlwe_batch: in[b * C + c] goes to coefficient coef[c] (distinct, each < N) of output b;
// in.size() = B * coef.size().  A gate output (+-1/8) becomes a table bit of TableLookup / PackedTableLookup.
inline std::vector<TRLWELv1> packTlwe(const CloudKey &ck, const PackingKey &key, const std::vector<TLWELv0> &in,
                                      const std::vector<uint32_t> &coef) {
    const size_t C = coef.size(), w = ck.params().n + 1, W = 2 * (size_t)ck.params().N;
    if (C == 0 || in.size() % C) throw Error(TFHE_ERR_INVALID, "packTlwe: B * C inputs for C coefficients");
    const size_t B = in.size() / C;
    std::vector<Torus> x(in.size() * w), out(B * W);
    for (size_t k = 0; k < in.size(); k++) std::copy(in[k].p.begin(), in[k].p.end(), x.begin() + k * w);
    check(tfhe_gpu_pack_tlwe_batch(ck.ctx(), key.get(), x.data(), coef.data(), C, out.data(), B), "pack_tlwe", ck.ctx());
    std::vector<TRLWELv1> r(B);
    for (size_t b = 0; b < B; b++) std::copy(out.begin() + b * W, out.begin() + (b + 1) * W, r[b].p.begin());
    return r;
}

// tfhe_gpu_packed_scatter_add_batch, the write beside PackedTableLookup::lookup: delta[q] is rotated to the slot of
// entry address_q (addr as in lookup), routed by the demultiplexer tree to that entry's TRLWE and added to t.table
// there (wrapping u32): the entry's coefficients 0 .. width-1 grow by delta[q]'s; queries with one address all add.
inline void packedScatterAdd(const CloudKey &ck, const TrgswSet &set, const std::vector<uint32_t> &addr,
                             const std::vector<TRLWELv1> &delta, PackedTableLookup &t) {
    const size_t Q = delta.size(), w = 2 * (size_t)ck.params().N;
    if (t.k == 0 || addr.size() != Q * t.k) throw Error(TFHE_ERR_INVALID, "packedScatterAdd: k selectors per delta");
    if (t.table.size() != (size_t)t.plan.trlwes * w) throw Error(TFHE_ERR_INVALID, "packedScatterAdd: a table of plan.trlwes TRLWEs");
    std::vector<Torus> d(Q * w);
    for (size_t q = 0; q < Q; q++) std::copy(delta[q].p.begin(), delta[q].p.end(), d.begin() + q * w);
    check(tfhe_gpu_packed_scatter_add_batch(ck.ctx(), set.get(), addr.data(), t.k, t.width, d.data(), t.table.data(), Q),
          "packed_scatter_add", ck.ctx());
}

// Sets entry address_q of t to in[q * width + c] (bit c; fresh +-1/8 TLWELv0), from existing calls around
// packedScatterAdd: lookup, extractBits with the key switch, the plain bootstrap of the old bits (fresh +-1/8),
// delta = new - old' on all n + 1 words, packTlwe into coefficients 0 .. width-1, packedScatterAdd.  The addresses of
// one call must be distinct for set semantics (the library cannot see them).  Every write adds noise to every entry, so
// a table is refreshed after a number of writes by extraction, bootstrap and fromCiphertexts.
inline void packedWrite(const CloudKey &ck, const TrgswSet &set, const PackingKey &key, const std::vector<uint32_t> &addr,
                        const std::vector<TLWELv0> &in, PackedTableLookup &t) {
    const size_t W = t.width, n1 = ck.params().n + 1;
    if (W == 0 || in.size() % W || t.k == 0 || addr.size() != in.size() / W * t.k)
        throw Error(TFHE_ERR_INVALID, "packedWrite: width ciphertexts and k selectors per write");
    const size_t Q = in.size() / W;
    std::vector<uint32_t> coef(W);
    for (uint32_t c = 0; c < W; c++) coef[c] = c;
    const std::vector<TRLWELv1> read = t.lookup(ck, set, addr);
    std::vector<Torus> old(Q * W * n1), fresh(Q * W * n1);
    for (size_t q = 0; q < Q; q++) {
        const std::vector<TLWELv0> bits = TableLookup::extractBits(ck, read[q], coef);
        for (size_t c = 0; c < W; c++) std::copy(bits[c].p.begin(), bits[c].p.end(), old.begin() + (q * W + c) * n1);
    }
    check(tfhe_gpu_bootstrap_batch(ck.ctx(), old.data(), fresh.data(), Q * W), "bootstrap", ck.ctx());
    std::vector<TLWELv0> delta(Q * W, TLWELv0(ck.params().n));
    for (size_t i = 0; i < Q * W; i++)
        for (size_t x = 0; x < n1; x++) delta[i].p[x] = in[i].p[x] - fresh[i * n1 + x];
    packedScatterAdd(ck, set, addr, packTlwe(ck, key, delta, coef), t);
}

// reencryptTLWELv0 (proxy_reenc.zig:267-306) on the GPU: the key is uploaded once to HBM; a
// context of its own (no cloud key needed).
class HipReencryptor {
  public:
    HipReencryptor(const tfhe_params &p, const ProxyReencryptionKey &k, int device = 0) : p_(p) {
        tfhe_gpu_ctx *c = nullptr;
        check(tfhe_gpu_create_on_device(&p, device, &c), "tfhe_gpu_create_on_device");
        ctx_.reset(c);
        tfhe_gpu_reenc_key *h = nullptr;
        check(tfhe_gpu_reenc_key_load(c, k.key_encryptions.data(), k.key_encryptions.size(), k.basebit, k.t, &h),
              "reenc_key_load", c);
        key_.reset(h);
    }
    std::vector<TLWELv0> reencryptBatch(const std::vector<TLWELv0> &in) const {
        const size_t w = p_.n + 1;
        std::vector<Torus> x(in.size() * w), y(in.size() * w);
        for (size_t k = 0; k < in.size(); k++) std::copy(in[k].p.begin(), in[k].p.end(), x.begin() + k * w);
        check(tfhe_gpu_reencrypt_batch(ctx_.get(), key_.get(), x.data(), y.data(), in.size()), "reencrypt",
              ctx_.get());
        std::vector<TLWELv0> r(in.size(), TLWELv0(p_.n));
        for (size_t k = 0; k < in.size(); k++) std::copy(y.begin() + k * w, y.begin() + (k + 1) * w, r[k].p.begin());
        return r;
    }
    TLWELv0 reencryptTLWELv0(const TLWELv0 &ct) const { return reencryptBatch({ct})[0]; }

  private:
    struct DelCtx {
        void operator()(tfhe_gpu_ctx *c) const { tfhe_gpu_destroy(c); }
    };
    struct DelKey {
        void operator()(tfhe_gpu_reenc_key *k) const { tfhe_gpu_reenc_key_destroy(k); }
    };
    tfhe_params p_{};
    std::unique_ptr<tfhe_gpu_ctx, DelCtx> ctx_;
    std::unique_ptr<tfhe_gpu_reenc_key, DelKey> key_;  // declared after ctx_: destroyed first
};

// bootstrap.zig:30-47 strategy, vanilla.zig:38-75 semantics
class HipBootstrap {
  public:
    TLWELv0 bootstrap(const TLWELv0 &ctxt, const CloudKey &ck) const {
        TLWELv0 out(ctxt.n());
        check(tfhe_gpu_bootstrap_batch(ck.ctx(), ctxt.p.data(), out.p.data(), 1), "bootstrap", ck.ctx());
        return out;
    }
    TLWELv0 bootstrapWithoutKeySwitch(const TLWELv0 &ctxt, const CloudKey &ck) const {
        TLWELv0 out(ctxt.n());
        check(tfhe_gpu_bootstrap_without_key_switch_batch(ck.ctx(), ctxt.p.data(), out.p.data(), 1),
              "bootstrapWithoutKeySwitch", ck.ctx());
        return out;
    }
    const char *name() const { return "mi355x"; }
};

// gates.zig:25-299
class Gates {
  public:
    Gates() = default;
    explicit Gates(HipBootstrap b) : bootstrap_(b) {}  // Gates.withBootstrap
    const char *bootstrapStrategy() const { return bootstrap_.name(); }

    TLWELv0 nandGate(const TLWELv0 &a, const TLWELv0 &b, const CloudKey &ck) const { return one(TFHE_GATE_NAND, a, b, ck); }
    TLWELv0 orGate(const TLWELv0 &a, const TLWELv0 &b, const CloudKey &ck) const { return one(TFHE_GATE_OR, a, b, ck); }
    TLWELv0 andGate(const TLWELv0 &a, const TLWELv0 &b, const CloudKey &ck) const { return one(TFHE_GATE_AND, a, b, ck); }
    TLWELv0 xorGate(const TLWELv0 &a, const TLWELv0 &b, const CloudKey &ck) const { return one(TFHE_GATE_XOR, a, b, ck); }
    TLWELv0 xnorGate(const TLWELv0 &a, const TLWELv0 &b, const CloudKey &ck) const { return one(TFHE_GATE_XNOR, a, b, ck); }
    TLWELv0 norGate(const TLWELv0 &a, const TLWELv0 &b, const CloudKey &ck) const { return one(TFHE_GATE_NOR, a, b, ck); }
    TLWELv0 andNyGate(const TLWELv0 &a, const TLWELv0 &b, const CloudKey &ck) const { return one(TFHE_GATE_ANDNY, a, b, ck); }
    TLWELv0 andYnGate(const TLWELv0 &a, const TLWELv0 &b, const CloudKey &ck) const { return one(TFHE_GATE_ANDYN, a, b, ck); }
    TLWELv0 orNyGate(const TLWELv0 &a, const TLWELv0 &b, const CloudKey &ck) const { return one(TFHE_GATE_ORNY, a, b, ck); }
    TLWELv0 orYnGate(const TLWELv0 &a, const TLWELv0 &b, const CloudKey &ck) const { return one(TFHE_GATE_ORYN, a, b, ck); }

    // muxNaive (gates.zig:124-129): AND(a, b) and AND(NOT a, c) in one batch, then OR
    TLWELv0 muxNaive(const TLWELv0 &a, const TLWELv0 &b, const TLWELv0 &c, const CloudKey &ck) const {
        const std::vector<std::pair<TLWELv0, TLWELv0>> lvl1{{a, b}, {notGate(a), c}};
        const auto r = batch(TFHE_GATE_AND, lvl1, ck);
        return orGate(r[0], r[1], ck);
    }
    TLWELv0 notGate(const TLWELv0 &a) const { return a.neg(); }  // gates.zig:132-135
    TLWELv0 copy(const TLWELv0 &a) const { return a; }           // gates.zig:138-141
    TLWELv0 constant(bool value, size_t n) const {               // gates.zig:144-151
        TLWELv0 r(n);
        const Torus mu = 1u << 29;  // f64ToTorus(0.125)
        r.bMut() = value ? mu : 1u - mu;  // the reference's 1 -% mu
        return r;
    }

    // gates.zig:244-299 declares these (returning error.NotImplemented): one
    // batched GPU launch here
    using Pairs = std::vector<std::pair<TLWELv0, TLWELv0>>;
    std::vector<TLWELv0> batchNand(const Pairs &in, const CloudKey &ck) const { return batch(TFHE_GATE_NAND, in, ck); }
    std::vector<TLWELv0> batchAnd(const Pairs &in, const CloudKey &ck) const { return batch(TFHE_GATE_AND, in, ck); }
    std::vector<TLWELv0> batchOr(const Pairs &in, const CloudKey &ck) const { return batch(TFHE_GATE_OR, in, ck); }
    std::vector<TLWELv0> batchXor(const Pairs &in, const CloudKey &ck) const { return batch(TFHE_GATE_XOR, in, ck); }
    std::vector<TLWELv0> batchNor(const Pairs &in, const CloudKey &ck) const { return batch(TFHE_GATE_NOR, in, ck); }
    std::vector<TLWELv0> batchXnor(const Pairs &in, const CloudKey &ck) const { return batch(TFHE_GATE_XNOR, in, ck); }

    // mixed-op batch: ops[k] applied to (a[k], b[k])
    std::vector<TLWELv0> gateBatch(const std::vector<uint8_t> &ops, const std::vector<TLWELv0> &a,
                                   const std::vector<TLWELv0> &b, const CloudKey &ck) const {
        if (ops.size() != a.size() || a.size() != b.size()) throw Error(TFHE_ERR_INVALID, "gateBatch: size mismatch");
        const size_t w = ck.params().n + 1, B = ops.size();
        std::vector<Torus> fa(B * w), fb(B * w), fo(B * w);
        for (size_t k = 0; k < B; k++) {
            std::copy(a[k].p.begin(), a[k].p.end(), fa.begin() + k * w);
            std::copy(b[k].p.begin(), b[k].p.end(), fb.begin() + k * w);
        }
        check(tfhe_gpu_gate_batch(ck.ctx(), ops.data(), fa.data(), fb.data(), fo.data(), B), "gateBatch", ck.ctx());
        std::vector<TLWELv0> out(B, TLWELv0(ck.params().n));
        for (size_t k = 0; k < B; k++) std::copy(fo.begin() + k * w, fo.begin() + (k + 1) * w, out[k].p.begin());
        return out;
    }

  private:
    TLWELv0 one(uint8_t op, const TLWELv0 &a, const TLWELv0 &b, const CloudKey &ck) const {
        return gateBatch({op}, {a}, {b}, ck)[0];
    }
    std::vector<TLWELv0> batch(uint8_t op, const Pairs &in, const CloudKey &ck) const {
        std::vector<uint8_t> ops(in.size(), op);
        std::vector<TLWELv0> a, b;
        for (const auto &pr : in) {
            a.push_back(pr.first);
            b.push_back(pr.second);
        }
        return gateBatch(ops, a, b, ck);
    }
    HipBootstrap bootstrap_;
};

// Level-scheduled gate circuit (tfhe_gpu_circuit_eval)
class Circuit {
  public:
    using Wire = uint32_t;
    Wire input() {
        if (!ops_.empty()) throw Error(TFHE_ERR_INVALID, "Circuit: declare inputs before gates");
        return n_inputs_++;
    }
    Wire gate(uint8_t op, Wire a, Wire b) {
        const Wire w = (Wire)(n_inputs_ + ops_.size());
        if (a >= w || b >= w) throw Error(TFHE_ERR_INVALID, "Circuit: gate inputs must be existing wires");
        ops_.push_back(op);
        ia_.push_back(a);
        ib_.push_back(b);
        return w;
    }
    Wire andGate(Wire a, Wire b) { return gate(TFHE_GATE_AND, a, b); }
    Wire orGate(Wire a, Wire b) { return gate(TFHE_GATE_OR, a, b); }
    Wire xorGate(Wire a, Wire b) { return gate(TFHE_GATE_XOR, a, b); }
    Wire notGate(Wire a) { return gate(TFHE_GATE_NOT, a, a); }
    Wire muxNaive(Wire a, Wire b, Wire c) { return orGate(andGate(a, b), andGate(notGate(a), c)); }
    // examples/add_two_numbers.zig:24-47
    std::pair<Wire, Wire> fullAdder(Wire a, Wire b, Wire cin) {
        const Wire x = xorGate(a, b), ab = andGate(a, b), xc = andGate(x, cin);
        return {xorGate(x, cin), orGate(ab, xc)};
    }
    void output(Wire w) { outs_.push_back(w); }

    std::vector<TLWELv0> run(const CloudKey &ck, const std::vector<TLWELv0> &inputs, uint32_t *levels = nullptr) const {
        if (inputs.size() != n_inputs_) throw Error(TFHE_ERR_INVALID, "Circuit: wrong number of inputs");
        const size_t w = ck.params().n + 1;
        std::vector<Torus> in(inputs.size() * w), out(outs_.size() * w);
        for (size_t k = 0; k < inputs.size(); k++) std::copy(inputs[k].p.begin(), inputs[k].p.end(), in.begin() + k * w);
        check(tfhe_gpu_circuit_eval(ck.ctx(), n_inputs_, in.data(), ops_.size(), ops_.data(), ia_.data(), ib_.data(),
                                    outs_.size(), outs_.data(), out.data(), levels),
              "Circuit.run", ck.ctx());
        std::vector<TLWELv0> r(outs_.size(), TLWELv0(ck.params().n));
        for (size_t k = 0; k < outs_.size(); k++) std::copy(out.begin() + k * w, out.begin() + (k + 1) * w, r[k].p.begin());
        return r;
    }
    // Inputs (numInputs() TLWELv0 words, row-major) and outputs (numOutputs()) in HBM;
    // async on the context stream (tfhe_gpu_circuit_eval_dev). Returns the bootstrap depth.
    uint32_t runDevice(const CloudKey &ck, const Torus *inputs_dev, Torus *outputs_dev) const {
        uint32_t levels = 0;
        check(tfhe_gpu_circuit_eval_dev(ck.ctx(), n_inputs_, inputs_dev, ops_.size(), ops_.data(), ia_.data(),
                                        ib_.data(), outs_.size(), outs_.data(), outputs_dev, &levels),
              "Circuit.runDevice", ck.ctx());
        return levels;
    }
    size_t numInputs() const { return n_inputs_; }
    size_t numOutputs() const { return outs_.size(); }

  private:
    uint32_t n_inputs_ = 0;
    std::vector<uint8_t> ops_;
    std::vector<uint32_t> ia_, ib_, outs_;
};

// Generator.generateLookupTable (lut/generator.zig:65-135) for f given as a table over m messages: 2N words.
inline std::vector<Torus> lutGenerate(const tfhe_params &p, const std::vector<uint32_t> &f_table) {
    std::vector<Torus> tv(2 * (size_t)p.N);
    check(tfhe_lut_generate(&p, (uint32_t)f_table.size(), f_table.data(), tv.data()), "lutGenerate");
    return tv;
}

// tfhe_lut_interleave: 1, 2, 4 or 8 test vectors -> the one a multi-output node reads (coefficient j = table j).
inline std::vector<Torus> lutInterleave(const tfhe_params &p, const std::vector<std::vector<Torus>> &tables) {
    uint32_t theta = 0;
    while (((size_t)1 << theta) < tables.size()) theta++;
    std::vector<Torus> all, tv(2 * (size_t)p.N);
    for (const std::vector<Torus> &t : tables) all.insert(all.end(), t.begin(), t.end());
    if (((size_t)1 << theta) != tables.size() || all.size() != tables.size() * tv.size())
        throw Error(TFHE_ERR_INVALID, "lutInterleave: 1, 2, 4 or 8 test vectors of 2N words");
    check(tfhe_lut_interleave(&p, all.data(), theta, tv.data()), "lutInterleave");
    return tv;
}

// tfhe_lut_round_tlwe: round_theta of the multi-output bootstrap on every word of a TLWELv0.
inline TLWELv0 lutRoundTlwe(const tfhe_params &p, uint32_t theta, const TLWELv0 &in) {
    TLWELv0 out(p.n);
    check(tfhe_lut_round_tlwe(&p, theta, in.p.data(), out.p.data(), 1), "lutRoundTlwe");
    return out;
}

// Test vectors resident in HBM (tfhe_gpu_lut_set): T TRLWELv1 of 2N words each, the tables of a LutCircuit.
class LutSet {
  public:
    LutSet(const CloudKey &ck, const std::vector<std::vector<Torus>> &tables) : size_(tables.size()) {
        const size_t per = 2 * (size_t)ck.params().N;
        std::vector<Torus> all;
        for (const std::vector<Torus> &t : tables) {
            if (t.size() != per) throw Error(TFHE_ERR_INVALID, "LutSet: a test vector has 2N words");
            all.insert(all.end(), t.begin(), t.end());
        }
        tfhe_gpu_lut_set *h = nullptr;
        check(tfhe_gpu_lut_set_load(ck.ctx(), all.data(), size_, &h), "lut_set_load", ck.ctx());
        set_.reset(h, tfhe_gpu_lut_set_destroy);
    }
    const tfhe_gpu_lut_set *get() const { return set_.get(); }
    size_t size() const { return size_; }

  private:
    std::shared_ptr<tfhe_gpu_lut_set> set_;
    size_t size_ = 0;
};

// ---- Bivariate LUT bootstrap (include/tfhe_gpu.h): f(x, y) of two m-ary digits at the set's full m ----
// The m level-1 tables of f given as f_table[x * m + y]: table i = lutGenerate of y -> f(i, y).  The tables of
// F functions, one after the other, make the LutSet of lutApply2.
inline std::vector<std::vector<Torus>> lutGenerate2(const tfhe_params &p, uint32_t m, const std::vector<uint32_t> &f_table) {
    if (m == 0 || f_table.size() != (size_t)m * m) throw Error(TFHE_ERR_INVALID, "lutGenerate2: m * m values");
    std::vector<std::vector<Torus>> tables;
    for (uint32_t i = 0; i < m; i++)
        tables.push_back(lutGenerate(p, std::vector<uint32_t>(f_table.begin() + (size_t)i * m, f_table.begin() + (size_t)(i + 1) * m)));
    return tables;
}

// tfhe_gpu_lut_spread_batch: the window sum of width w on each half, times X^rot; w = N/m, rot = 2N - N/(2m)
// turns values at the slots x * w into the generator's test vector.
inline std::vector<TRLWELv1> lutSpread(const CloudKey &ck, const std::vector<TRLWELv1> &in, uint32_t w, uint32_t rot) {
    const size_t B = in.size(), W = 2 * (size_t)ck.params().N;
    std::vector<Torus> x(B * W), out(B * W);
    for (size_t b = 0; b < B; b++) std::copy(in[b].p.begin(), in[b].p.end(), x.begin() + b * W);
    check(tfhe_gpu_lut_spread_batch(ck.ctx(), x.data(), w, rot, out.data(), B), "lut_spread", ck.ctx());
    std::vector<TRLWELv1> r(B);
    for (size_t b = 0; b < B; b++) std::copy(out.begin() + b * W, out.begin() + (b + 1) * W, r[b].p.begin());
    return r;
}

// tfhe_gpu_bootstrap_lut_each_batch: item i is bootstrapped with its own test vector testvecs[i] (any a).
inline std::vector<TLWELv0> bootstrapLutEach(const CloudKey &ck, const std::vector<TLWELv0> &in,
                                             const std::vector<TRLWELv1> &testvecs) {
    const size_t B = in.size(), w = ck.params().n + 1, W = 2 * (size_t)ck.params().N;
    if (testvecs.size() != B) throw Error(TFHE_ERR_INVALID, "bootstrapLutEach: one test vector per input");
    std::vector<Torus> x(B * w), tv(B * W), out(B * w);
    for (size_t b = 0; b < B; b++) {
        std::copy(in[b].p.begin(), in[b].p.end(), x.begin() + b * w);
        std::copy(testvecs[b].p.begin(), testvecs[b].p.end(), tv.begin() + b * W);
    }
    check(tfhe_gpu_bootstrap_lut_each_batch(ck.ctx(), x.data(), tv.data(), out.data(), B), "bootstrap_lut_each", ck.ctx());
    std::vector<TLWELv0> r(B, TLWELv0(ck.params().n));
    for (size_t b = 0; b < B; b++) std::copy(out.begin() + b * w, out.begin() + (b + 1) * w, r[b].p.begin());
    return r;
}

// tfhe_gpu_lut_apply2_batch: node b computes f_fn(pool[x_src], pool[y_src]) with the tables set[fn * m + i]
// (lutGenerate2): m level-1 bootstraps of y, the pack, the spread, one bootstrap of x.
struct Lut2Node {
    uint32_t fn, x_src, y_src;
};
inline std::vector<TLWELv0> lutApply2(const CloudKey &ck, const LutSet &set, const PackingKey &key, uint32_t m,
                                      const std::vector<TLWELv0> &pool, const std::vector<Lut2Node> &nodes) {
    const size_t B = nodes.size(), w = ck.params().n + 1;
    std::vector<Torus> x(pool.size() * w), out(B * w);
    std::vector<uint32_t> fn, xs, ys;
    for (size_t k = 0; k < pool.size(); k++) std::copy(pool[k].p.begin(), pool[k].p.end(), x.begin() + k * w);
    for (const Lut2Node &nd : nodes) fn.push_back(nd.fn), xs.push_back(nd.x_src), ys.push_back(nd.y_src);
    check(tfhe_gpu_lut_apply2_batch(ck.ctx(), set.get(), key.get(), m, x.data(), pool.size(), fn.data(), xs.data(), ys.data(),
                                    out.data(), B),
          "lut_apply2", ck.ctx());
    std::vector<TLWELv0> r(B, TLWELv0(ck.params().n));
    for (size_t b = 0; b < B; b++) std::copy(out.begin() + b * w, out.begin() + (b + 1) * w, r[b].p.begin());
    return r;
}

// ---- Extended LUT bootstrap (include/tfhe_gpu.h): 5- and 6-bit digits, E = 2^eta accumulator components ----
// tfhe_lut_generate_ext: the E components (2N words each) of the extended test vector of f_table (m = its size).
// The components of several functions, one function after the other, make the LutSet of lutApplyExt.
inline std::vector<std::vector<Torus>> lutGenerateExt(const tfhe_params &p, uint32_t eta,
                                                      const std::vector<uint32_t> &f_table) {
    if (eta > TFHE_LUT_EXT_MAX_LOG) throw Error(TFHE_ERR_INVALID, "lutGenerateExt: eta > TFHE_LUT_EXT_MAX_LOG");
    const size_t E = (size_t)1 << eta, W = 2 * (size_t)p.N;
    std::vector<Torus> all(E * W);
    check(tfhe_lut_generate_ext(&p, eta, (uint32_t)f_table.size(), f_table.data(), all.data()), "lutGenerateExt");
    std::vector<std::vector<Torus>> comps;
    for (size_t j = 0; j < E; j++) comps.emplace_back(all.begin() + j * W, all.begin() + (j + 1) * W);
    return comps;
}

// tfhe_gpu_blind_rotate_ext_batch (stage entry): all E accumulators of every input, item-major.
inline std::vector<TRLWELv1> blindRotateExt(const CloudKey &ck, uint32_t eta, const std::vector<TLWELv0> &in,
                                            const std::vector<std::vector<Torus>> &testvec) {
    if (eta > TFHE_LUT_EXT_MAX_LOG) throw Error(TFHE_ERR_INVALID, "blindRotateExt: eta > TFHE_LUT_EXT_MAX_LOG");
    const size_t B = in.size(), w = ck.params().n + 1, W = 2 * (size_t)ck.params().N, E = (size_t)1 << eta;
    if (testvec.size() != E) throw Error(TFHE_ERR_INVALID, "blindRotateExt: 2^eta components");
    std::vector<Torus> x(B * w), tv, out(B * E * W);
    for (size_t b = 0; b < B; b++) std::copy(in[b].p.begin(), in[b].p.end(), x.begin() + b * w);
    for (const std::vector<Torus> &c : testvec) {
        if (c.size() != W) throw Error(TFHE_ERR_INVALID, "blindRotateExt: a component has 2N words");
        tv.insert(tv.end(), c.begin(), c.end());
    }
    check(tfhe_gpu_blind_rotate_ext_batch(ck.ctx(), eta, x.data(), tv.data(), out.data(), B), "blind_rotate_ext", ck.ctx());
    std::vector<TRLWELv1> r(B * E);
    for (size_t k = 0; k < B * E; k++) std::copy(out.begin() + k * W, out.begin() + (k + 1) * W, r[k].p.begin());
    return r;
}

// tfhe_gpu_lut_apply_ext_batch: node i = sum coef * pool[src] + konst on the b word, then the extended bootstrap
// with the extended table lut (the set's entries lut * E .. lut * E + E - 1).
struct LutExtNode {
    uint32_t lut;
    std::vector<std::pair<uint32_t, int32_t>> terms;  // (pool index, coefficient)
    Torus konst = 0;
};
inline std::vector<TLWELv0> lutApplyExt(const CloudKey &ck, const LutSet &set, uint32_t eta,
                                        const std::vector<TLWELv0> &pool, const std::vector<LutExtNode> &nodes) {
    const size_t B = nodes.size(), w = ck.params().n + 1;
    std::vector<Torus> x(pool.size() * w), out(B * w);
    for (size_t k = 0; k < pool.size(); k++) std::copy(pool[k].p.begin(), pool[k].p.end(), x.begin() + k * w);
    std::vector<uint32_t> off(1, 0u), src, konst, lut;
    std::vector<int32_t> coef;
    for (const LutExtNode &nd : nodes) {
        for (const auto &t : nd.terms) src.push_back(t.first), coef.push_back(t.second);
        off.push_back((uint32_t)src.size());
        konst.push_back(nd.konst);
        lut.push_back(nd.lut);
    }
    check(tfhe_gpu_lut_apply_ext_batch(ck.ctx(), set.get(), eta, x.data(), pool.size(), off.data(), src.data(), coef.data(),
                                       konst.data(), lut.data(), out.data(), B),
          "lut_apply_ext", ck.ctx());
    std::vector<TLWELv0> r(B, TLWELv0(ck.params().n));
    for (size_t b = 0; b < B; b++) std::copy(out.begin() + b * w, out.begin() + (b + 1) * w, r[b].p.begin());
    return r;
}

// Level-scheduled LUT circuit (tfhe_gpu_lut_circuit_eval): a node is an integer combination of earlier
// wires (TLWELv0.add / addMul / subMul, tlwe.zig:120-240), then a programmable bootstrap with its own table.
class LutCircuit {
  public:
    using Wire = uint32_t;
    using Term = std::pair<Wire, int32_t>;  // (wire, coefficient)
    Wire input() {
        if (!lut_.empty()) throw Error(TFHE_ERR_INVALID, "LutCircuit: declare inputs before nodes");
        n_wires_++;
        return n_inputs_++;
    }
    // theta > 0: a multi-output node (lut names a lutInterleave table); it drives the 2^theta wires from the
    // returned one on, one per interleaved table.  eta > 0 (include/tfhe_gpu.h "Extended nodes"): the extended
    // bootstrap, lut naming the extended table, lutGenerateExt's 2^eta entries from lut * 2^eta on; theta is then 0.
    Wire node(uint32_t lut, const std::vector<Term> &terms, Torus konst = 0, uint32_t theta = 0, uint32_t eta = 0) {
        if (theta > TFHE_LUT_MULTI_MAX_LOG) throw Error(TFHE_ERR_INVALID, "LutCircuit: a node has 1, 2, 4 or 8 outputs");
        if (eta > TFHE_LUT_EXT_MAX_LOG || (eta && theta))
            throw Error(TFHE_ERR_INVALID, "LutCircuit: a node's eta is 0, 1 or 2, and an extended node has one output");
        const Wire w = n_wires_;
        for (const Term &t : terms) {
            if (t.first >= w) throw Error(TFHE_ERR_INVALID, "LutCircuit: node terms must read existing wires");
            wire_.push_back(t.first);
            coef_.push_back(t.second);
        }
        off_.push_back((uint32_t)wire_.size());
        konst_.push_back(konst);
        lut_.push_back(lut);
        theta_.push_back(theta);
        eta_.push_back(eta);
        multi_ = multi_ || theta != 0;
        ext_ = ext_ || eta != 0;
        n_wires_ += 1u << theta;
        return w;
    }
    // A select node (include/tfhe_gpu.h "Select nodes"): the digit x = sum of terms + konst picks one of the
    // m = entries.size() entries, each an earlier wire or a constant Torus word; its table is packed from the
    // entries on the device.  One m per circuit; run / runDevice then take the packing key.  eta > 0: x is read by
    // the extended bootstrap, which keeps the margin of m = 16 at m = 32 (eta = 1) or 64 (eta = 2) on the UINT4 key.
    struct Entry {
        Wire wire = TFHE_LUT_ENTRY_CONST;
        Torus konst = 0;
        Entry(Wire w) : wire(w) {}  // a wire
        static Entry constant(Torus c) {
            Entry e(TFHE_LUT_ENTRY_CONST);
            e.konst = c;
            return e;
        }
    };
    Wire select(const std::vector<Term> &terms, const std::vector<Entry> &entries, Torus konst = 0, uint32_t eta = 0) {
        const uint32_t m = (uint32_t)entries.size();
        if (m < 2 || (m & (m - 1)) || (m_ && m != m_))
            throw Error(TFHE_ERR_INVALID, "LutCircuit: a select node has m entries, m a power of two >= 2, one m per circuit");
        for (const Entry &e : entries)
            if (e.wire != TFHE_LUT_ENTRY_CONST && e.wire >= n_wires_)
                throw Error(TFHE_ERR_INVALID, "LutCircuit: select entries must read existing wires");
        const Wire w = node(0, terms, konst, 0, eta);
        m_ = m;
        for (const Entry &e : entries) sel_wire_.push_back(e.wire), sel_konst_.push_back(e.konst);
        const uint32_t last = sel_off_.back();
        sel_off_.resize(lut_.size(), last);  // the ordinary nodes since the last select node: no entries
        sel_off_.push_back((uint32_t)sel_wire_.size());
        return w;
    }
    // f(x, y) of two m-ary digits: m ordinary nodes with the tables lut_base + i (lutGenerate2's rows) over y_terms
    // and one select node over x_terms; returns the select node's wire.  eta is the select node's.
    Wire node2(uint32_t lut_base, const std::vector<Term> &x_terms, const std::vector<Term> &y_terms, uint32_t m,
               uint32_t eta = 0) {
        if (m_ && m != m_) throw Error(TFHE_ERR_INVALID, "LutCircuit: one m per circuit");
        std::vector<Entry> entries;
        for (uint32_t i = 0; i < m; i++) entries.push_back(Entry(node(lut_base + i, y_terms)));
        return select(x_terms, entries, 0, eta);
    }
    void output(Wire w) { outs_.push_back(w); }
    // Least significant digit first: per digit s = a_i + b_i + carry, message = LUT_msg(s), carry = LUT_carry(s);
    // returns the message wires, then the final carry as an extra digit.
    std::vector<Wire> radixAdd(const std::vector<Wire> &a, const std::vector<Wire> &b, uint32_t msg_lut,
                               uint32_t carry_lut) {
        std::vector<Wire> out;
        bool have_carry = false;
        Wire carry = 0;
        for (size_t i = 0; i < a.size() && i < b.size(); i++) {
            std::vector<Term> terms{{a[i], 1}, {b[i], 1}};
            if (have_carry) terms.push_back({carry, 1});
            out.push_back(node(msg_lut, terms));
            carry = node(carry_lut, terms);
            have_carry = true;
        }
        if (have_carry) out.push_back(carry);
        return out;
    }
    // radixAdd with one two-output node per digit: lut is lutInterleave of the (message, carry) tables, at half
    // the message modulus radixAdd's tables may use.
    std::vector<Wire> radixAddFused(const std::vector<Wire> &a, const std::vector<Wire> &b, uint32_t lut) {
        std::vector<Wire> out;
        bool have_carry = false;
        Wire carry = 0;
        for (size_t i = 0; i < a.size() && i < b.size(); i++) {
            std::vector<Term> terms{{a[i], 1}, {b[i], 1}};
            if (have_carry) terms.push_back({carry, 1});
            const Wire msg = node(lut, terms, 0, 1);
            out.push_back(msg);
            carry = msg + 1;
            have_carry = true;
        }
        if (have_carry) out.push_back(carry);
        return out;
    }
    // tfhe_lut_circuit_schedule(_multi): the level of every node; *depth (may be NULL) the largest
    std::vector<uint32_t> schedule(uint32_t *depth = nullptr) const {
        std::vector<uint32_t> levels(lut_.size());
        check(tfhe_lut_circuit_schedule_select(n_inputs_, lut_.size(), off_.data(), wire_.data(), theta(), m_, selOff(),
                                               sel_wire_.data(), levels.data(), depth),
              "LutCircuit.schedule");
        return levels;
    }
    // tfhe_lut_circuit_schedule_ext: the levels, and per level the node counts of its eta = 0, 1 and 2 groups
    // (groups[3 (lv - 1) + eta]), the items of that level's launches
    std::vector<uint32_t> scheduleExt(std::vector<uint32_t> &groups, uint32_t *depth = nullptr) const {
        std::vector<uint32_t> levels(lut_.size());
        uint32_t d = 0;
        groups.assign(3 * lut_.size(), 0);
        check(tfhe_lut_circuit_schedule_ext(n_inputs_, lut_.size(), off_.data(), wire_.data(), theta(), m_, selOff(),
                                            sel_wire_.data(), eta(), levels.data(), &d, groups.data()),
              "LutCircuit.scheduleExt");
        groups.resize(3 * (size_t)d);
        if (depth) *depth = d;
        return levels;
    }
    // key: the packing key of a circuit with select nodes (NULL without one)
    std::vector<TLWELv0> run(const CloudKey &ck, const LutSet &set, const std::vector<TLWELv0> &inputs,
                             uint32_t *levels = nullptr, const PackingKey *key = nullptr) const {
        if (inputs.size() != n_inputs_) throw Error(TFHE_ERR_INVALID, "LutCircuit: wrong number of inputs");
        if (m_ && !key) throw Error(TFHE_ERR_INVALID, "LutCircuit: select nodes need a packing key");
        const size_t w = ck.params().n + 1;
        std::vector<Torus> in(inputs.size() * w), out(outs_.size() * w);
        for (size_t k = 0; k < inputs.size(); k++) std::copy(inputs[k].p.begin(), inputs[k].p.end(), in.begin() + k * w);
        if (ext_)  // some eta > 0: the entry with eta; otherwise exactly the call without it
            check(tfhe_gpu_lut_circuit_eval_ext(ck.ctx(), set.get(), key ? key->get() : nullptr, m_, n_inputs_, in.data(),
                                                lut_.size(), off_.data(), wire_.data(), coef_.data(), konst_.data(),
                                                lut_.data(), theta(), selOff(), sel_wire_.data(), sel_konst_.data(),
                                                eta(), outs_.size(), outs_.data(), out.data(), levels),
                  "LutCircuit.run", ck.ctx());
        else
            check(tfhe_gpu_lut_circuit_eval_select(ck.ctx(), set.get(), key ? key->get() : nullptr, m_, n_inputs_,
                                                   in.data(), lut_.size(), off_.data(), wire_.data(), coef_.data(),
                                                   konst_.data(), lut_.data(), theta(), selOff(), sel_wire_.data(),
                                                   sel_konst_.data(), outs_.size(), outs_.data(), out.data(), levels),
                  "LutCircuit.run", ck.ctx());
        std::vector<TLWELv0> r(outs_.size(), TLWELv0(ck.params().n));
        for (size_t k = 0; k < outs_.size(); k++) std::copy(out.begin() + k * w, out.begin() + (k + 1) * w, r[k].p.begin());
        return r;
    }
    // Inputs and outputs in HBM; async on the context stream (tfhe_gpu_lut_circuit_eval_dev).  Returns the depth.
    uint32_t runDevice(const CloudKey &ck, const LutSet &set, const Torus *inputs_dev, Torus *outputs_dev,
                       const PackingKey *key = nullptr) const {
        uint32_t levels = 0;
        if (m_ && !key) throw Error(TFHE_ERR_INVALID, "LutCircuit: select nodes need a packing key");
        if (ext_)
            check(tfhe_gpu_lut_circuit_eval_ext_dev(ck.ctx(), set.get(), key ? key->get() : nullptr, m_, n_inputs_,
                                                    inputs_dev, lut_.size(), off_.data(), wire_.data(), coef_.data(),
                                                    konst_.data(), lut_.data(), theta(), selOff(), sel_wire_.data(),
                                                    sel_konst_.data(), eta(), outs_.size(), outs_.data(), outputs_dev,
                                                    &levels),
                  "LutCircuit.runDevice", ck.ctx());
        else
            check(tfhe_gpu_lut_circuit_eval_select_dev(ck.ctx(), set.get(), key ? key->get() : nullptr, m_, n_inputs_,
                                                       inputs_dev, lut_.size(), off_.data(), wire_.data(), coef_.data(),
                                                       konst_.data(), lut_.data(), theta(), selOff(), sel_wire_.data(),
                                                       sel_konst_.data(), outs_.size(), outs_.data(), outputs_dev,
                                                       &levels),
                  "LutCircuit.runDevice", ck.ctx());
        return levels;
    }
    size_t numInputs() const { return n_inputs_; }
    size_t numNodes() const { return lut_.size(); }
    size_t numOutputs() const { return outs_.size(); }

  private:
    // NULL without a multi-output node: the _multi entries are then the single-output ones
    const uint32_t *theta() const { return multi_ ? theta_.data() : nullptr; }
    // NULL without an extended node
    const uint32_t *eta() const { return ext_ ? eta_.data() : nullptr; }
    // NULL without a select node (the _select entries are then the _multi ones); else one offset per node and one
    // more, the nodes behind the last select node without entries
    const uint32_t *selOff() const {
        if (!m_) return nullptr;
        const uint32_t last = sel_off_.back();
        sel_off_.resize(lut_.size() + 1, last);
        return sel_off_.data();
    }
    uint32_t n_inputs_ = 0, n_wires_ = 0, m_ = 0;
    bool multi_ = false, ext_ = false;
    std::vector<uint32_t> off_{0}, wire_, konst_, lut_, theta_, eta_, outs_, sel_wire_, sel_konst_;
    mutable std::vector<uint32_t> sel_off_{0};
    std::vector<int32_t> coef_;
};

// tfhe_gpu_lut_select_batch: the flat form of the select node over a pool.  Node b bootstraps the combination of its
// terms (pool indices) and konst with the test vector packed from its m entries, pool indices or constants.
struct LutSelectNode {
    std::vector<LutCircuit::Term> terms;
    std::vector<LutCircuit::Entry> entries;
    Torus konst = 0;
};
// eta > 0: tfhe_gpu_lut_select_ext_batch (lutSelectExt below).
inline std::vector<TLWELv0> lutSelect(const CloudKey &ck, const PackingKey &key, uint32_t m, const std::vector<TLWELv0> &pool,
                                      const std::vector<LutSelectNode> &nodes, uint32_t eta = 0) {
    const size_t B = nodes.size(), w = ck.params().n + 1;
    std::vector<Torus> x(pool.size() * w), out(B * w);
    std::vector<uint32_t> off{0}, src, konst, sel_src, sel_konst;
    std::vector<int32_t> coef;
    for (size_t k = 0; k < pool.size(); k++) std::copy(pool[k].p.begin(), pool[k].p.end(), x.begin() + k * w);
    for (const LutSelectNode &nd : nodes) {
        if (nd.entries.size() != m) throw Error(TFHE_ERR_INVALID, "lutSelect: a node has m entries");
        for (const LutCircuit::Term &t : nd.terms) src.push_back(t.first), coef.push_back(t.second);
        off.push_back((uint32_t)src.size());
        konst.push_back(nd.konst);
        for (const LutCircuit::Entry &e : nd.entries) sel_src.push_back(e.wire), sel_konst.push_back(e.konst);
    }
    if (eta)
        check(tfhe_gpu_lut_select_ext_batch(ck.ctx(), key.get(), m, eta, x.data(), pool.size(), off.data(), src.data(),
                                            coef.data(), konst.data(), sel_src.data(), sel_konst.data(), out.data(), B),
              "lut_select_ext", ck.ctx());
    else
        check(tfhe_gpu_lut_select_batch(ck.ctx(), key.get(), m, x.data(), pool.size(), off.data(), src.data(), coef.data(),
                                        konst.data(), sel_src.data(), sel_konst.data(), out.data(), B),
              "lut_select", ck.ctx());
    std::vector<TLWELv0> r(B, TLWELv0(ck.params().n));
    for (size_t b = 0; b < B; b++) std::copy(out.begin() + b * w, out.begin() + (b + 1) * w, r[b].p.begin());
    return r;
}

// tfhe_gpu_lut_select_ext_batch: lutSelect with the extended bootstrap, so that m may be 32 (eta = 1) or 64 (eta = 2).
inline std::vector<TLWELv0> lutSelectExt(const CloudKey &ck, const PackingKey &key, uint32_t m, uint32_t eta,
                                         const std::vector<TLWELv0> &pool, const std::vector<LutSelectNode> &nodes) {
    if (eta > TFHE_LUT_EXT_MAX_LOG) throw Error(TFHE_ERR_INVALID, "lutSelectExt: eta > TFHE_LUT_EXT_MAX_LOG");
    return lutSelect(ck, key, m, pool, nodes, eta);
}

// tfhe_gpu_bootstrap_lut_each_ext_batch: the extended bootstrap of item i with its one test vector testvecs[i] (any
// a) in all 2^eta components.
inline std::vector<TLWELv0> bootstrapLutEachExt(const CloudKey &ck, uint32_t eta, const std::vector<TLWELv0> &in,
                                                const std::vector<TRLWELv1> &testvecs) {
    const size_t B = in.size(), w = ck.params().n + 1, W = 2 * (size_t)ck.params().N;
    if (testvecs.size() != B) throw Error(TFHE_ERR_INVALID, "bootstrapLutEachExt: one test vector per input");
    std::vector<Torus> x(B * w), tv(B * W), out(B * w);
    for (size_t b = 0; b < B; b++) {
        std::copy(in[b].p.begin(), in[b].p.end(), x.begin() + b * w);
        std::copy(testvecs[b].p.begin(), testvecs[b].p.end(), tv.begin() + b * W);
    }
    check(tfhe_gpu_bootstrap_lut_each_ext_batch(ck.ctx(), eta, x.data(), tv.data(), out.data(), B), "bootstrap_lut_each_ext",
          ck.ctx());
    std::vector<TLWELv0> r(B, TLWELv0(ck.params().n));
    for (size_t b = 0; b < B; b++) std::copy(out.begin() + b * w, out.begin() + (b + 1) * w, r[b].p.begin());
    return r;
}

}  // namespace tfhe
