// tfhe_scratch.hpp — the device scratch of one GPU as a stack.  A call opens
// a Frame, takes slices from it, and every slice stays valid and the taker's until the frame
// closes; a nested frame's slices go back when it closes, so siblings (a circuit's levels, a
// pack's chunks) share their space.  Memory comes in blocks from an injected allocator and is
// the high-water mark of one call: blocks are neither moved nor freed while a frame is open,
// and the next outermost frame trades several blocks for one of the high-water size.  No HIP
// here: tfhe_gpu.cpp injects hipMalloc / hipFree, cpp/test_scratch_cpu.cpp malloc.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "tfhe_gpu.h"  // TFHE_OK, TFHE_ERR_OOM

namespace tfhe {

class Scratch {
  public:
    static constexpr size_t ALIGN = 256;          // of every slice; the allocator's blocks are at least as aligned
    static constexpr size_t MIN_BLOCK = 64 << 10;
    // bytes past its last row that the one-hot GEMM key switch may read of its input: KS_GEMM_INPUT_SLACK
    // (tfhe_internal.hpp, which needs HIP; tfhe_ctx.hpp asserts the two agree)
    static constexpr size_t KS_INPUT_SLACK = 16;

    // alloc returns NULL on failure (and reports why in its own way: the device's error string).
    struct Allocator {
        void *(*alloc)(void *user, size_t bytes) = nullptr;
        void (*free)(void *user, void *p) = nullptr;
        void *user = nullptr;
    };

    Scratch() = default;
    explicit Scratch(Allocator a) : a_(a) {}
    Scratch(Scratch &&o) noexcept
        : a_(o.a_), blocks_(std::move(o.blocks_)), cur_(o.cur_), off_(o.off_), used_(o.used_), high_(o.high_), depth_(o.depth_), rc_(o.rc_) {
        o.blocks_.clear();
    }
    Scratch &operator=(Scratch &&) = delete;
    ~Scratch() { free_blocks(); }
    void set_allocator(Allocator a) { a_ = a; }

    size_t blocks() const { return blocks_.size(); }
    size_t high_water() const { return high_; }  // most bytes (slices, aligned) any call has held at once

    // A mark with RAII release.  The outermost frame of a call also clears the last call's failure
    // and coalesces; a failure (rc) is the arena's and fails the whole call: takes after it return NULL.
    class Frame {
      public:
        explicit Frame(Scratch &s) : s_(s) {
            if (s_.depth_++ == 0) s_.begin_call();
            cur_ = s_.cur_, off_ = s_.off_, used_ = s_.used_;
        }
        ~Frame() {
            s_.cur_ = cur_, s_.off_ = off_, s_.used_ = used_;
            s_.depth_--;
        }
        Frame(const Frame &) = delete;
        Frame &operator=(const Frame &) = delete;

        void *bytes(size_t n) { return s_.take(n); }  // ALIGN-aligned, or NULL: rc()
        template <class T>
        T *take(size_t count) {
            return static_cast<T *>(bytes(count * sizeof(T)));
        }
        // An input of the GEMM key switch with its read-ahead slack; the pack's GEMM (64 tiles wide) reads
        // whole blocks of 8 coefficients, up to 6 words past the last row's n + 1: twice the slack.
        template <class T>
        T *ks_input(size_t count, bool pack = false) {
            return static_cast<T *>(bytes(count * sizeof(T) + (pack ? 2 : 1) * KS_INPUT_SLACK));
        }
        int rc() const { return s_.rc_; }
        void fail(int code) {
            if (!s_.rc_) s_.rc_ = code;
        }

      private:
        Scratch &s_;
        size_t cur_, off_, used_;
    };

  private:
    struct Block {
        char *p;
        size_t bytes;
    };

    void free_blocks() {
        for (Block &b : blocks_) a_.free(a_.user, b.p);
        blocks_.clear();
    }
    // Several blocks -> one of the high-water size, so the steady state is one block and no allocation.
    // With the real allocator the frees synchronise the device (hipFree does), as growing a buffer always
    // has: a _dev call's kernels may still be running in the old blocks when the next call gets here.
    // If the one block cannot be had the arena is empty, and the call's takes allocate as they go.
    void begin_call() {
        rc_ = TFHE_OK;
        cur_ = off_ = used_ = 0;
        if (blocks_.size() < 2) return;
        free_blocks();
        if (void *p = a_.alloc(a_.user, high_)) blocks_.push_back(Block{static_cast<char *>(p), high_});
    }
    void *take(size_t n) {
        if (rc_) return nullptr;
        const size_t need = (std::max<size_t>(n, 1) + ALIGN - 1) & ~(ALIGN - 1);
        size_t cur = cur_, off = off_;
        while (cur < blocks_.size() && off + need > blocks_[cur].bytes) cur++, off = 0;  // a later block may fit
        if (cur == blocks_.size()) {
            const size_t size = std::max(need, MIN_BLOCK);
            void *p = a_.alloc(a_.user, size);
            if (!p) {
                rc_ = TFHE_ERR_OOM;
                return nullptr;
            }
            blocks_.push_back(Block{static_cast<char *>(p), size});
        }
        cur_ = cur;
        off_ = off + need;
        used_ += need;
        high_ = std::max(high_, used_);
        return blocks_[cur].p + off;
    }

    Allocator a_;
    std::vector<Block> blocks_;
    size_t cur_ = 0, off_ = 0;  // the bump pointer: block and offset
    size_t used_ = 0;           // bytes in open slices, as one block would hold them
    size_t high_ = 0;
    int depth_ = 0;  // open frames
    int rc_ = TFHE_OK;
};

}  // namespace tfhe
