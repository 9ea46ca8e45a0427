// Region bookkeeping of HostStage (common.h): pure arithmetic, no HIP header, so a host program can check it (tests/host_stage_main.cpp).
// add() hands out offsets in order.  Every region starts on a multiple of kAlign and owns at least kAlign bytes, so a region of zero bytes
// still has an address of its own; bytes() is what to allocate and is never zero.  A byte count that does not fit size_t, a negative
// dimension or a region beyond kMaxRegions only sets `overflow`: the caller refuses the whole layout before anything is allocated.
// The regions sit in the object itself (no heap): the single-shot decode call that declares six of them is latency bound.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

namespace qldpc {

struct StageLayout {
    static constexpr size_t kAlign = 256;
    static constexpr int kMaxRegions = 24;          // qldpc_osdw_batch declares 19
    struct Region { size_t off, bytes; };
    Region regions[kMaxRegions];
    int count = 0;
    size_t total = 0;
    bool overflow = false;

    // a region of `n` elements of `elem` bytes -> its index (-1 beyond kMaxRegions)
    int add(size_t n, size_t elem) {
        if (count == kMaxRegions) { overflow = true; return -1; }
        size_t bytes = 0, padded = 0, end = 0;
        if (__builtin_mul_overflow(n, elem, &bytes) || __builtin_add_overflow(bytes, kAlign - 1, &padded) ||
            __builtin_add_overflow(total, padded < kAlign ? kAlign : padded / kAlign * kAlign, &end)) {
            overflow = true;
            bytes = 0; end = total;
        }
        regions[count] = {total, bytes};
        total = end;
        return count++;
    }
    // the same for an element count given as a product of dimensions (B, n, ...)
    int add(std::initializer_list<int64_t> dims, size_t elem) {
        size_t n = 1;
        for (const int64_t d : dims)
            if (d < 0 || __builtin_mul_overflow(n, (size_t)d, &n)) { overflow = true; n = 0; }
        return add(n, elem);
    }
    size_t bytes() const { return total ? total : kAlign; }
};

}  // namespace qldpc
