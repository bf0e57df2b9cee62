// Stand-alone tests of the GPU-free half of the C ABI (csrc/tfhe_cpu.cpp): the
// circuit planner, the partitioner, cloud-key files, LUT generation and seeded
// encryption.  Links tfhe_cpu.o only — no HIP, no libtfhe_gpu.so — so the same
// two sources also build and run under the host sanitizers (make cpu-check).
// Exit status 0 = all passed.
#include "tfhe_cpu.hpp"

#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {
int failures = 0;
void expect(bool ok, const char *test, const char *what) {
    if (!ok) {
        std::printf("FAIL %s: %s\n", test, what);
        failures++;
    }
}

struct Lcg {  // the test's own generator (Knuth's MMIX constants)
    uint64_t s;
    uint32_t next(uint32_t mod) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33) % mod;
    }
};

// the test's own cost model: whole rounds of 4 x #CUs items
double whole_rounds(size_t items, size_t cus) { return (double)((items + 4 * cus - 1) / (4 * cus)); }

struct Dag {
    size_t n_in = 0;
    std::vector<uint8_t> ops;
    std::vector<uint32_t> a, b, outs;
    size_t gates() const { return ops.size(); }
};

Dag random_dag(uint64_t seed) {
    static const uint8_t OPS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, TFHE_GATE_NOT, TFHE_GATE_COPY};
    Lcg r{seed};
    Dag d;
    d.n_in = 1 + r.next(8);
    const size_t G = r.next(301);
    for (size_t g = 0; g < G; g++) {
        d.ops.push_back(OPS[r.next(12)]);
        d.a.push_back(r.next((uint32_t)(d.n_in + g)));
        d.b.push_back(r.next((uint32_t)(d.n_in + g)));
    }
    for (uint32_t o = 0, n = r.next(5); o < n; o++) d.outs.push_back(r.next((uint32_t)(d.n_in + G)));
    return d;
}

using Levels = std::vector<std::vector<uint32_t>>;

void test_scheduler() {
    bool seen[256] = {};
    for (uint64_t seed = 0; seed < 200; seed++) {
        const Dag d = random_dag(seed);
        const size_t G = d.gates();
        for (uint8_t op : d.ops) seen[op] = true;
        for (size_t cus : {(size_t)4, (size_t)256}) {
            uint32_t depth[2] = {0, 0};
            for (int pack = 0; pack < 2; pack++) {
                std::vector<uint32_t> level;
                Levels bs, nots;
                const char *why = tfhe::schedule_levels(d.n_in, G, d.ops.data(), d.a.data(), d.b.data(), pack != 0, cus,
                                                        whole_rounds, level, depth[pack], bs, nots);
                expect(!why, "scheduler", "a valid graph is refused");
                std::vector<int> times(G, 0);
                for (uint32_t lv = 0; lv < bs.size(); lv++) {
                    for (uint32_t g : bs[lv]) times[g] += d.ops[g] != TFHE_GATE_NOT && level[d.n_in + g] == lv ? 1 : 2;
                    for (uint32_t g : nots[lv]) times[g] += d.ops[g] == TFHE_GATE_NOT && level[d.n_in + g] == lv ? 1 : 2;
                }
                for (size_t g = 0; g < G; g++) {
                    expect(times[g] == 1, "scheduler", "a gate is not in exactly one group of its level");
                    const uint32_t lv = level[d.n_in + g], la = level[d.a[g]], lb = level[d.b[g]];
                    if (d.ops[g] == TFHE_GATE_NOT)
                        expect(lv == la, "scheduler", "a NOT is not at its input's level");
                    else
                        expect(lv > la && (d.ops[g] > TFHE_GATE_ORYN || lv > lb), "scheduler",
                               "a bootstrapped gate is not above its inputs");
                }
                tfhe::CircuitPlan pl;
                why = tfhe::plan_circuit(d.n_in, G, d.ops.data(), d.a.data(), d.b.data(), d.outs.size(), d.outs.data(),
                                         pack != 0, cus, whole_rounds, pl);
                expect(!why && pl.max_level == depth[pack], "plan", "refused, or another depth than the schedule's");
                size_t nb = 0, nn = 0, ip = 0, sp = d.n_in;
                bool earlier = true;
                for (uint32_t lv = 0; lv <= pl.max_level; lv++) {
                    for (size_t k = 0; k < 2 * pl.bs[lv].size(); k++) earlier = earlier && pl.idx[ip++] < sp;
                    sp += pl.bs[lv].size();
                    for (size_t k = 0; k < pl.nots[lv].size(); k++) earlier = earlier && pl.idx[ip++] < sp;
                    sp += pl.nots[lv].size();
                    nb += pl.bs[lv].size();
                    nn += pl.nots[lv].size();
                }
                expect(pl.idx.size() == 2 * nb + nn + d.outs.size(), "plan", "idx size");
                expect(pl.cops.size() == nb, "plan", "cops size");
                expect(earlier, "plan", "a group gathers from its own or a later slot");
            }
            expect(depth[0] == depth[1], "scheduler", "packing changed the depth");
        }
    }
    for (int op : {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 254, 255}) expect(seen[op], "scheduler", "an op never appeared");
    std::printf("ok   scheduler and plan (200 random DAGs, pack on/off, 4 and 256 CUs)\n");
}

void test_packing() {  // the example above pack_levels (tfhe_cpu.cpp)
    const size_t n = 10256;
    std::vector<uint8_t> ops(n + 2, TFHE_GATE_NAND);
    std::vector<uint32_t> a(n + 2, 0), b(n + 2, 1);
    a[n] = 2, b[n] = 3;                     // on gates 0 and 1
    a[n + 1] = (uint32_t)(2 + n), b[n + 1] = 4;  // on that and gate 2
    for (int pack = 0; pack < 2; pack++) {
        std::vector<uint32_t> level;
        Levels bs, nots;
        uint32_t depth = 0;
        const char *why =
            tfhe::schedule_levels(2, n + 2, ops.data(), a.data(), b.data(), pack != 0, 256, whole_rounds, level, depth, bs, nots);
        expect(!why && depth == 3, "packing", "depth 3");
        if (why || depth != 3) continue;
        const size_t want[2][3] = {{10256, 1, 1}, {10240, 17, 1}};
        for (int lv = 1; lv <= 3; lv++) expect(bs[lv].size() == want[pack][lv - 1], "packing", "level sizes");
    }
    std::printf("ok   packing (10,256 / 1 / 1 -> 10,240 / 17 / 1)\n");
}

void test_rejections() {
    struct Case {
        uint8_t op;
        uint32_t a, b, out;
        const char *why;
    };
    const Case cases[] = {{10, 0, 0, 0, "unknown gate op"},
                          {TFHE_GATE_AND, 2, 0, 0, "gate input a is not an earlier wire"},
                          {TFHE_GATE_AND, 0, 2, 0, "gate input b is not an earlier wire"},
                          {TFHE_GATE_AND, 0, 1, 3, "output wire out of range"}};
    for (const Case &c : cases) {  // two inputs, one gate, one output
        tfhe::CircuitPlan pl;
        const char *p = tfhe::plan_circuit(2, 1, &c.op, &c.a, &c.b, 1, &c.out, true, 256, whole_rounds, pl);
        const char *v = tfhe::check_circuit(2, 1, &c.op, &c.a, &c.b, 1, &c.out);
        expect(p && !std::strcmp(p, c.why), "rejections", c.why);
        expect(v && !std::strcmp(v, c.why), "rejections (check_circuit)", c.why);
    }
    tfhe::CircuitPlan pl;
    expect(!tfhe::plan_circuit(3, 0, nullptr, nullptr, nullptr, 0, nullptr, true, 256, whole_rounds, pl) &&
               pl.max_level == 0 && pl.idx.empty(),
           "rejections", "no gates is a valid circuit");
    expect(!tfhe::check_circuit(3, 0, nullptr, nullptr, nullptr, 0, nullptr), "rejections", "no gates is valid");
    std::printf("ok   rejections (four reasons; no gates accepted)\n");
}

void test_partition() {
    for (uint64_t seed = 0; seed < 200; seed++) {
        const Dag d = random_dag(seed);
        for (int D : {1, 2, 3, 8}) {
            std::vector<uint32_t> dev(d.gates(), 99);
            const int rc = tfhe_circuit_partition(d.n_in, d.gates(), d.ops.data(), d.a.data(), d.b.data(), D, dev.data());
            expect(rc == TFHE_OK, "partition", "status");
            for (size_t g = 0; g < d.gates(); g++) {
                expect(dev[g] < (uint32_t)D && (D > 1 || dev[g] == 0), "partition", "device out of range");
                if (d.a[g] >= d.n_in) expect(dev[d.a[g] - d.n_in] == dev[g], "partition", "wire a crosses devices");
                if (d.ops[g] <= TFHE_GATE_ORYN && d.b[g] >= d.n_in)
                    expect(dev[d.b[g] - d.n_in] == dev[g], "partition", "wire b crosses devices");
            }
        }
    }
    expect(tfhe_circuit_partition(4, 0, nullptr, nullptr, nullptr, 3, nullptr) == TFHE_OK, "partition", "no gates");
    std::printf("ok   partition (no wire crosses devices; D = 1, 2, 3, 8)\n");
}

// a circuit on plain booleans: every wire's value
std::vector<bool> eval_bools(size_t n_in, const std::vector<uint8_t> &ops, const std::vector<uint32_t> &a,
                             const std::vector<uint32_t> &b, const std::vector<bool> &in) {
    std::vector<bool> w(in.begin(), in.begin() + n_in);
    for (size_t g = 0; g < ops.size(); g++) {
        const bool x = w[a[g]], y = ops[g] <= TFHE_GATE_ORYN ? (bool)w[b[g]] : false;
        switch (ops[g]) {
        case TFHE_GATE_NAND: w.push_back(!(x && y)); break;
        case TFHE_GATE_OR: w.push_back(x || y); break;
        case TFHE_GATE_AND: w.push_back(x && y); break;
        case TFHE_GATE_XOR: w.push_back(x != y); break;
        case TFHE_GATE_XNOR: w.push_back(x == y); break;
        case TFHE_GATE_NOR: w.push_back(!(x || y)); break;
        case TFHE_GATE_ANDNY: w.push_back(!x && y); break;
        case TFHE_GATE_ANDYN: w.push_back(x && !y); break;
        case TFHE_GATE_ORNY: w.push_back(!x || y); break;
        case TFHE_GATE_ORYN: w.push_back(x || !y); break;
        case TFHE_GATE_NOT: w.push_back(!x); break;
        default: w.push_back(x); break;  // TFHE_GATE_COPY
        }
    }
    return w;
}

// split_circuit of `d` under the placement `dev`: every sub-circuit is a valid circuit, every
// output of the whole circuit comes from exactly one of them, and on plain booleans (all
// assignments of up to 10 inputs, else 64 of them) the re-assembled outputs equal the whole's.
void check_split(const char *what, const Dag &d, const std::vector<uint32_t> &dev, size_t D) {
    const auto sub = tfhe::split_circuit(d.n_in, d.gates(), d.ops.data(), d.a.data(), d.b.data(), d.outs.size(),
                                         d.outs.data(), dev, D);
    expect(sub.size() == D, what, "one sub-circuit per device");
    std::vector<int> covered(d.outs.size(), 0);
    size_t gates = 0;
    for (size_t k = 0; k < sub.size(); k++) {
        const tfhe::SubCircuit &s = sub[k];
        gates += s.ops.size();
        expect(s.in_a.size() == s.ops.size() && s.in_b.size() == s.ops.size() && s.out_index.size() == s.out_wires.size(),
               what, "sub-circuit array lengths");
        expect(!tfhe::check_circuit(s.inputs.size(), s.ops.size(), s.ops.data(), s.in_a.data(), s.in_b.data(),
                                    s.out_wires.size(), s.out_wires.data()),
               what, "sub-circuit passes check_circuit");
        for (uint32_t w : s.inputs) expect(w < d.n_in, what, "sub-circuit input is a primary input");
        for (uint32_t o : s.out_index)
            if (o < covered.size()) covered[o]++;
            else expect(false, what, "out_index out of range");
    }
    expect(gates == d.gates(), what, "every gate on one device");
    for (int c : covered) expect(c == 1, what, "every output from exactly one device");
    const size_t cases = d.n_in <= 10 ? (size_t)1 << d.n_in : 64;
    Lcg r{d.n_in * 977 + d.gates()};
    for (size_t t = 0; t < cases; t++) {
        std::vector<bool> in(d.n_in);
        for (size_t i = 0; i < d.n_in; i++) in[i] = d.n_in <= 10 ? (t >> i) & 1 : r.next(2) != 0;
        const std::vector<bool> whole = eval_bools(d.n_in, d.ops, d.a, d.b, in);
        std::vector<int> got(d.outs.size(), -1);
        for (const tfhe::SubCircuit &s : sub) {
            std::vector<bool> sin(s.inputs.size());
            for (size_t i = 0; i < s.inputs.size(); i++) sin[i] = in[s.inputs[i]];
            const std::vector<bool> w = eval_bools(s.inputs.size(), s.ops, s.in_a, s.in_b, sin);
            for (size_t k = 0; k < s.out_wires.size(); k++) got[s.out_index[k]] = w[s.out_wires[k]];
        }
        bool same = true;
        for (size_t o = 0; o < d.outs.size(); o++) same = same && got[o] == (int)whole[d.outs[o]];
        expect(same, what, "re-assembled outputs equal the whole circuit's");
    }
}

void test_split_circuit() {
    // inputs a0 a1 b0 b1 cin (0-4) and x0..x7 (5-12): a 2-bit ripple adder, then four independent gates
    Dag d;
    d.n_in = 13;
    auto gate = [&](uint8_t op, uint32_t a, uint32_t b) {
        d.ops.push_back(op);
        d.a.push_back(a);
        d.b.push_back(b);
        return (uint32_t)(d.n_in + d.gates() - 1);
    };
    uint32_t carry = 4;
    for (uint32_t i = 0; i < 2; i++) {  // full adder: s = a ^ b ^ c, c' = (a & b) | (c & (a ^ b))
        const uint32_t x = gate(TFHE_GATE_XOR, i, 2 + i), s = gate(TFHE_GATE_XOR, x, carry);
        const uint32_t g1 = gate(TFHE_GATE_AND, i, 2 + i), g2 = gate(TFHE_GATE_AND, carry, x);
        carry = gate(TFHE_GATE_OR, g1, g2);
        d.outs.push_back(s);
    }
    d.outs.push_back(carry);
    d.outs.push_back(gate(TFHE_GATE_NAND, 5, 6));
    d.outs.push_back(gate(TFHE_GATE_ORNY, 7, 8));
    d.outs.push_back(gate(TFHE_GATE_ANDYN, 9, 10));
    d.outs.push_back(gate(TFHE_GATE_COPY, 11, 12));
    for (size_t D : {1, 2, 3}) {
        std::vector<uint32_t> dev;
        tfhe::partition_gates(d.n_in, d.gates(), d.ops.data(), d.a.data(), d.b.data(), D, dev);
        check_split("split: adder + 4 gates", d, dev, D);
        if (D == 3) {  // the adder (10 gates) whole on one device, the four gates on the other two
            std::vector<size_t> n(D, 0);
            for (uint32_t x : dev) n[x]++;
            expect(n[dev[0]] == 10, "split: adder + 4 gates", "the adder stays whole");
        }
    }
    // an output that is a primary input comes from device 0, which here has no gate; device 2 has none either
    Dag e;
    e.n_in = 3;
    e.ops = {TFHE_GATE_AND, TFHE_GATE_XOR};
    e.a = {0, 3};
    e.b = {1, 1};
    e.outs = {2, 4, 2, 0};
    check_split("split: input as output", e, {1, 1}, 3);
    const auto se = tfhe::split_circuit(e.n_in, 2, e.ops.data(), e.a.data(), e.b.data(), 4, e.outs.data(), {1, 1}, 3);
    expect(se[0].ops.empty() && se[0].out_index == std::vector<uint32_t>({0, 2, 3}) &&
               se[0].inputs == std::vector<uint32_t>({2, 0}) && se[0].out_wires == std::vector<uint32_t>({0, 0, 1}),
           "split: input as output", "device 0 copies the primary inputs out");
    expect(se[1].out_index == std::vector<uint32_t>({1}) && se[1].inputs == std::vector<uint32_t>({0, 1}),
           "split: input as output", "device 1 has the gates and their inputs only");
    expect(se[2].ops.empty() && se[2].inputs.empty() && se[2].out_wires.empty(), "split: input as output",
           "a device without gates or outputs is empty");
    // a NOT's in_b is ignored: here it names a gate of the other device and an input nobody reads
    Dag f;
    f.n_in = 3;
    f.ops = {TFHE_GATE_AND, TFHE_GATE_NOT, TFHE_GATE_NOT, TFHE_GATE_OR};
    f.a = {0, 1, 4, 5};
    f.b = {1, 3, 2, 1};
    f.outs = {3, 6};
    check_split("split: NOT ignores in_b", f, {0, 1, 1, 1}, 2);
    const auto sf = tfhe::split_circuit(f.n_in, 4, f.ops.data(), f.a.data(), f.b.data(), 2, f.outs.data(), {0, 1, 1, 1}, 2);
    expect(sf[1].inputs == std::vector<uint32_t>({1}) && sf[1].in_b[0] == 0 && sf[1].in_b[1] == 0,
           "split: NOT ignores in_b", "in_b of a NOT brings in no input and no wire");
    std::printf("ok   split_circuit (adder + 4 gates over D = 1, 2, 3; input as output; empty device; NOT's in_b)\n");
}

void test_slice_of() {
    for (size_t D : {1, 2, 8})
        for (size_t B : {(size_t)0, (size_t)1, D - 1, D, D + 1, (size_t)1100}) {
            const size_t per = (B + D - 1) / D;
            size_t next = 0;
            for (size_t d = 0; d < D; d++) {
                const tfhe::Slice s = tfhe::slice_of(B, D, d);
                expect(s.lo == next, "slice_of", "slices are contiguous and in device order");
                expect(s.lo == std::min(B, d * per) && s.n == std::min(B, s.lo + per) - s.lo, "slice_of",
                       "ceil(B/D) items per device");
                next = s.lo + s.n;
            }
            expect(next == B, "slice_of", "the slices cover [0, B) exactly once");
        }
    std::printf("ok   slice_of (B in {0, 1, D-1, D, D+1, 1100}, D in {1, 2, 8})\n");
}

void test_key_file() {  // the smallest parameters params_ok takes
    tfhe_params p{1, 1024, 10, 1, 8, 3, 2, 0, 2.0e-5, 2.0e-8, 2.0e-5, 2.0e-8};
    const size_t bl = 4096, kl = 32768, bytes = 64 + 2 * 4096 + bl * 8 + kl * 4;
    std::vector<uint32_t> ta(1024), tb(1024), ksk(kl), ta2(1024), tb2(1024), ksk2(kl);
    std::vector<double> bsk(2 * bl), bsk2(2 * bl);  // twice: the L = 2 read below asks for 8,192
    Lcg r{7};
    for (auto &x : ta) x = r.next(0xFFFFFFFFu);
    for (auto &x : tb) x = r.next(0xFFFFFFFFu);
    for (auto &x : ksk) x = r.next(0xFFFFFFFFu);
    for (auto &x : bsk) x = (double)r.next(1u << 30) - 536870912.0;
    char path[] = "/tmp/tfhe_test_cpu_XXXXXX";
    const int fd = mkstemp(path);
    expect(fd >= 0, "key file", "mkstemp");
    if (fd < 0) return;
    close(fd);
    auto read = [&](const tfhe_params &q, size_t bsk_len, uint32_t *off) {
        return tfhe_cloud_key_read(path, &q, off, ta2.data(), tb2.data(), bsk2.data(), bsk_len, ksk2.data(), kl);
    };
    auto rewrite = [&](const std::vector<char> &f, size_t n) {
        FILE *fp = std::fopen(path, "wb");
        const bool ok = fp && std::fwrite(f.data(), 1, n, fp) == n;
        if (fp) std::fclose(fp);
        expect(ok, "key file", "rewrite");
    };
    uint32_t off = 0;
    expect(tfhe_cloud_key_write(path, &p, 0x80808080u, ta.data(), tb.data(), bsk.data(), bl, ksk.data(), kl) == TFHE_OK,
           "key file", "write");
    expect(read(p, bl, &off) == TFHE_OK && off == 0x80808080u && ta2 == ta && tb2 == tb && ksk2 == ksk &&
               !std::memcmp(bsk2.data(), bsk.data(), bl * 8),
           "key file", "round trip");
    tfhe_params p2 = p;
    p2.L = 2;
    expect(read(p2, 2 * bl, &off) == TFHE_ERR_INVALID, "key file", "another L");
    std::vector<char> f(bytes);
    FILE *fp = std::fopen(path, "rb");
    expect(fp && std::fread(f.data(), 1, bytes, fp) == bytes && std::fgetc(fp) == EOF, "key file", "size");
    if (fp) std::fclose(fp);
    for (size_t cut : {(size_t)10, (size_t)64, bytes - 1}) {
        rewrite(f, cut);
        expect(read(p, bl, &off) == TFHE_ERR_IO, "key file", "truncated");
    }
    f[bytes / 2] ^= 1;
    rewrite(f, bytes);
    expect(read(p, bl, &off) == TFHE_ERR_INVALID, "key file", "flipped payload byte");
    f[bytes / 2] ^= 1;
    f[0] ^= 1;
    rewrite(f, bytes);
    expect(read(p, bl, &off) == TFHE_ERR_INVALID, "key file", "wrong magic");
    std::remove(path);
    std::printf("ok   key file (round trip, truncations, flipped byte, magic, other L)\n");
}

void test_lut() {
    const tfhe_params p{636, 1024, 10, 3, 6, 2, 9, 0, 2.0e-5, 2.0e-8, 2.0e-5, 2.0e-8};
    for (uint32_t m : {1u, 2u, 1024u, 1025u, 4096u}) {
        std::vector<uint32_t> f(m), tv(2048, 0xDEADBEEFu);
        for (uint32_t x = 0; x < m; x++) f[x] = (x * 7 + 3) % m;
        expect(tfhe_lut_generate(&p, m, f.data(), tv.data()) == TFHE_OK, "lut", "status");
        bool a0 = true, filled = true;
        for (size_t i = 0; i < 1024; i++) a0 = a0 && tv[i] == 0;
        for (size_t i = 1024; i < 2048; i++) filled = filled && tv[i] != 0xDEADBEEFu;
        expect(a0 && filled, "lut", "2N words, a = 0");
        std::vector<uint32_t> tv2(2048, 1u);
        expect(tfhe_lut_generate_full(&p, m, f.data(), tv2.data()) == TFHE_OK && tv2[0] == 0, "lut", "full");
    }
    uint32_t one = 0, tv[2048];
    expect(tfhe_lut_generate(&p, 0, &one, tv) == TFHE_ERR_INVALID, "lut", "m = 0");
    expect(tfhe_lut_generate(&p, TFHE_LUT_MAX_M + 1, &one, tv) == TFHE_ERR_INVALID, "lut", "m > TFHE_LUT_MAX_M");
    std::printf("ok   lut (m = 1, 2, 1024, 1025, 4096; bad m refused)\n");
}

void test_encrypt() {  // n = 636 with the 128-bit noise
    const tfhe_params p{636, 1024, 10, 3, 6, 2, 9, 0, 2.0e-5, 2.0e-8, 2.0e-5, 2.0e-8};
    const size_t B = 64, w = p.n + 1;
    std::vector<uint32_t> k0(p.n), k1(p.N), ct(B * w), msgs(B), got(B);
    std::vector<uint8_t> bits(B), gotb(B);
    expect(tfhe_secret_key_new(&p, 42, k0.data(), k1.data()) == TFHE_OK, "encrypt", "secret key");
    for (size_t i = 0; i < B; i++) bits[i] = (i * 5 + i / 3) & 1, msgs[i] = (uint32_t)(i * 11 % 16);
    expect(tfhe_encrypt_bool_batch(&p, k0.data(), bits.data(), 1000, ct.data(), B) == TFHE_OK &&
               tfhe_decrypt_bool_batch(&p, k0.data(), ct.data(), gotb.data(), B) == TFHE_OK && gotb == bits,
           "encrypt", "64 booleans decrypt to themselves");
    expect(tfhe_encrypt_lwe_message_batch(&p, k0.data(), msgs.data(), 16, 2000, ct.data(), B) == TFHE_OK &&
               tfhe_decrypt_lwe_message_batch(&p, k0.data(), ct.data(), 16, got.data(), B) == TFHE_OK && got == msgs,
           "encrypt", "64 messages mod 16 decrypt to themselves");
    std::printf("ok   encrypt / decrypt (64 booleans, 64 messages mod 16)\n");
}
}  // namespace

int main() {
    test_scheduler();
    test_packing();
    test_rejections();
    test_partition();
    test_split_circuit();
    test_slice_of();
    test_key_file();
    test_lut();
    test_encrypt();
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "PASSED", failures);
    return failures ? 1 : 0;
}
