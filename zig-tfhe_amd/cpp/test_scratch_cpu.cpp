// Stand-alone test of the scratch arena (csrc/tfhe_scratch.hpp) over an allocator that hands out
// aligned malloc blocks and records every call: alignment and disjoint slices, nested release,
// growth by new blocks that moves nothing, the coalesce of the next outermost frame, the steady
// state, an allocator failure, and the key-switch input's slack.  Includes that header only — no
// HIP, no library — and builds and runs under the host sanitizers too (make cpu-check).
// Exit status 0 = all passed.
#include "tfhe_scratch.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

namespace {
using tfhe::Scratch;
int failures = 0;
void expect(bool ok, const char *test, const char *what) {
    if (!ok) {
        std::printf("FAIL %s: %s\n", test, what);
        failures++;
    }
}

struct Recorder {
    std::map<char *, size_t> live;  // block -> bytes
    int allocs = 0, frees = 0, bad_frees = 0;
    size_t fail_at_or_above = ~(size_t)0;  // requests this large fail
    size_t last_bytes = 0;
};
void *rec_alloc(void *user, size_t bytes) {
    Recorder &r = *static_cast<Recorder *>(user);
    r.allocs++;
    r.last_bytes = bytes;
    if (bytes >= r.fail_at_or_above) return nullptr;
    char *p = static_cast<char *>(std::aligned_alloc(Scratch::ALIGN, (bytes + Scratch::ALIGN - 1) / Scratch::ALIGN * Scratch::ALIGN));
    r.live[p] = bytes;
    return p;
}
void rec_free(void *user, void *p) {
    Recorder &r = *static_cast<Recorder *>(user);
    r.frees++;
    if (!r.live.erase(static_cast<char *>(p))) r.bad_frees++;  // unknown, or freed twice
    else std::free(p);
}
// [p, p + n) lies inside one live block
bool inside(const Recorder &r, const void *p, size_t n) {
    for (const auto &b : r.live)
        if ((const char *)p >= b.first && (const char *)p + n <= b.first + b.second) return true;
    return false;
}
bool aligned(const void *p) { return p && (uintptr_t)p % Scratch::ALIGN == 0; }
bool disjoint(const void *a, size_t na, const void *b, size_t nb) {
    return (const char *)a + na <= (const char *)b || (const char *)b + nb <= (const char *)a;
}
constexpr size_t KB = 1024, MB = 1024 * 1024;

// The calls of one "entry point": an outer frame with two slices, then three sibling frames of `inner` bytes.
void sequence(Scratch &s, size_t inner) {
    Scratch::Frame f(s);
    f.bytes(100 * KB);
    f.bytes(3);
    for (int i = 0; i < 3; i++) {
        Scratch::Frame g(s);
        g.bytes(inner);
        g.take<uint32_t>(1000);
    }
}
}  // namespace

int main() {
    {
        const char *T = "slices";
        Recorder r;
        Scratch s({rec_alloc, rec_free, &r});
        {
            Scratch::Frame f(s);
            const size_t n[5] = {1, 255, 256, 257, 5000};
            void *p[5];
            for (int i = 0; i < 5; i++) {
                p[i] = f.bytes(n[i]);
                expect(aligned(p[i]), T, "a slice is not 256-byte aligned");
                expect(inside(r, p[i], n[i]), T, "a slice is not inside a block");
                std::memset(p[i], i + 1, n[i]);
            }
            for (int i = 0; i < 5; i++)
                for (int j = i + 1; j < 5; j++) expect(disjoint(p[i], n[i], p[j], n[j]), T, "two slices overlap");
            uint64_t *q = f.take<uint64_t>(10);
            expect(aligned(q) && inside(r, q, 80), T, "take<T>(count) is count * sizeof(T) bytes");
            expect(aligned(f.bytes(0)), T, "an empty slice is still a pointer");
            expect(f.rc() == TFHE_OK, T, "rc");
        }
        expect(r.allocs == 1, T, "small slices share one block");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "nested release";
        Recorder r;
        Scratch s({rec_alloc, rec_free, &r});
        Scratch::Frame f(s);
        char *a = static_cast<char *>(f.bytes(1000));
        std::memset(a, 0x5a, 1000);
        void *first = nullptr;
        for (int i = 0; i < 33; i++) {  // 33 levels need the space once
            Scratch::Frame g(s);
            void *b = g.bytes(20 * KB);
            std::memset(b, i, 20 * KB);
            if (i == 0) first = b;
            expect(b == first, T, "a sibling frame does not reuse its predecessor's space");
            expect(disjoint(a, 1000, b, 20 * KB), T, "a nested slice overlaps the parent's");
        }
        char *c = static_cast<char *>(f.bytes(8));
        expect(c == first, T, "the parent does not get the released space back");
        bool kept = true;
        for (int i = 0; i < 1000; i++) kept &= a[i] == 0x5a;
        expect(kept, T, "the parent's slice lost its contents");
        expect(r.allocs == 1 && r.frees == 0, T, "allocator calls");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "growth and coalesce";
        Recorder r;
        Scratch s({rec_alloc, rec_free, &r});
        size_t high = 0;
        {
            Scratch::Frame f(s);
            char *a = static_cast<char *>(f.bytes(10 * KB));
            std::memset(a, 7, 10 * KB);
            char *b = static_cast<char *>(f.bytes(1 * MB));  // does not fit the first block
            expect(r.allocs == 2 && r.last_bytes >= 1 * MB && r.frees == 0, T, "a take that does not fit opens a block of at least its size");
            expect(inside(r, a, 10 * KB) && a[0] == 7 && a[10 * KB - 1] == 7, T, "the earlier slice moved");
            expect(aligned(b) && inside(r, b, 1 * MB), T, "the large slice");
            {
                Scratch::Frame g(s);
                g.bytes(3 * MB);
            }
            char *c = static_cast<char *>(f.bytes(2 * MB));  // the nested frame's block serves again
            expect(r.allocs == 3 && inside(r, c, 2 * MB), T, "a released block is reused");
            expect(s.blocks() == 3, T, "blocks");
            high = s.high_water();
            expect(high >= 10 * KB + 1 * MB + 3 * MB, T, "high water");
        }
        expect(r.frees == 0 && r.live.size() == 3, T, "no block is freed when the frame closes");
        {
            Scratch::Frame f(s);  // the next call
            expect(r.frees == 3 && r.bad_frees == 0 && r.allocs == 4, T, "every old block is freed once, one is allocated");
            expect(s.blocks() == 1 && r.live.size() == 1 && r.last_bytes >= high, T, "one block of at least the high-water size");
            f.bytes(10 * KB);
            f.bytes(1 * MB);
            Scratch::Frame g(s);
            g.bytes(3 * MB);
            expect(r.allocs == 4 && s.blocks() == 1, T, "the same needs fit the one block");
        }
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "steady state";
        Recorder r;
        Scratch s({rec_alloc, rec_free, &r});
        sequence(s, 700 * KB);
        sequence(s, 700 * KB);  // coalesces
        const int allocs = r.allocs, frees = r.frees;
        sequence(s, 700 * KB);
        sequence(s, 700 * KB);
        expect(r.allocs == allocs && r.frees == frees, T, "a repeated sequence calls the allocator");
        sequence(s, 5 * KB);  // a smaller call: nothing shrinks
        expect(r.allocs == allocs && r.frees == frees && s.blocks() == 1, T, "a smaller call calls the allocator");
        sequence(s, 2 * MB);  // a larger one grows, the next coalesces, then steady again
        sequence(s, 2 * MB);
        const int allocs2 = r.allocs;
        sequence(s, 2 * MB);
        sequence(s, 700 * KB);
        expect(r.allocs == allocs2 && s.blocks() == 1 && r.bad_frees == 0, T, "steady after growth");
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "allocator failure";
        Recorder r;
        Scratch s({rec_alloc, rec_free, &r});
        r.fail_at_or_above = 1 * MB;
        {
            Scratch::Frame f(s);
            char *a = static_cast<char *>(f.bytes(1000));
            std::memset(a, 1, 1000);
            expect(f.bytes(4 * MB) == nullptr && f.rc() == TFHE_ERR_OOM, T, "a failed take is NULL with TFHE_ERR_OOM");
            expect(f.bytes(8) == nullptr, T, "a failed call takes nothing more");
            Scratch::Frame g(s);
            expect(g.rc() == TFHE_ERR_OOM, T, "the failure is the whole call's");
            expect(a[999] == 1 && inside(r, a, 1000), T, "the earlier slice is gone");
        }
        {
            Scratch::Frame f(s);  // the next call works
            expect(f.rc() == TFHE_OK && aligned(f.bytes(500 * KB)) && f.rc() == TFHE_OK, T, "the arena is not usable after a failure");
        }
        {  // the coalesce's own allocation fails: the call goes on block by block
            Scratch::Frame f(s);
            f.bytes(500 * KB);
            f.bytes(900 * KB);  // a second block, and a high-water mark of 1.4 MB
            expect(f.rc() == TFHE_OK && s.blocks() >= 2, T, "two blocks");
        }
        {
            Scratch::Frame f(s);  // would coalesce to 1.4 MB: refused
            expect(s.blocks() <= 1 && r.bad_frees == 0, T, "coalesce");
            expect(aligned(f.bytes(900 * KB)) && f.rc() == TFHE_OK, T, "a call after a failed coalesce");
        }
        std::printf("ok   %s\n", T);
    }
    {
        const char *T = "key-switch input";
        Recorder r;
        Scratch s({rec_alloc, rec_free, &r});
        Scratch::Frame f(s);
        // sized so that count * 4 fills whole alignment units: the slack must still be inside the block
        const size_t count = Scratch::MIN_BLOCK / 4;
        uint32_t *x = f.ks_input<uint32_t>(count);
        expect(aligned(x) && inside(r, x, count * 4 + Scratch::KS_INPUT_SLACK), T, "the slack is outside the allocation");
        uint32_t *y = f.ks_input<uint32_t>(count, /*pack*/ true);
        expect(aligned(y) && inside(r, y, count * 4 + 2 * Scratch::KS_INPUT_SLACK), T, "the pack's doubled slack is outside the allocation");
        std::memset(x, 0, count * 4 + Scratch::KS_INPUT_SLACK);
        std::memset(y, 0, count * 4 + 2 * Scratch::KS_INPUT_SLACK);
        void *z = f.bytes(64);
        expect(disjoint(x, count * 4 + Scratch::KS_INPUT_SLACK, y, count * 4 + 2 * Scratch::KS_INPUT_SLACK) &&
                   disjoint(y, count * 4 + 2 * Scratch::KS_INPUT_SLACK, z, 64),
               T, "the slack overlaps the next slice");
        expect(Scratch::KS_INPUT_SLACK == 16, T, "the slack is the GEMM's 16 bytes");
        std::printf("ok   %s\n", T);
    }
    std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
    return failures ? 1 : 0;
}
