// tdt_grow.h — the one way a buffer of the host API grows, and the capacity rules in use.  Plain
// C++17 without a HIP include: tests/cpp/test_grow.cpp drives it with a fake allocator.
#pragma once

#include <algorithm>
#include <cstddef>

namespace psy {

// Capacity rules: the capacity a buffer of recorded size `have` takes when a call needs `need`.
// exact: buffers sized by the batch alone (cp_idx, cp_buf, hbases, slot_sums)
inline size_t cap_exact(size_t need, size_t /*have*/) { return need; }
// max(need, 2·have): workspaces that follow growing batches (ws, the plan buffer, mx_tab, h_dev)
inline size_t cap_double(size_t need, size_t have) { return std::max(need, 2 * have); }
// 1.5x, rounded up to a whole MiB: the host-pipeline slots' device and pinned buffers, sized by
// the chunks of varying calls (they settle after a few; the retired ones sum to less than twice
// the last)
inline size_t cap_slot(size_t need, size_t have) {
    constexpr size_t MiB = size_t(1) << 20;
    return (std::max(need, have + have / 2) + MiB - 1) & ~(MiB - 1);
}

// Grow the buffer (p, have) to capacity `cap` when it holds less than `need`; nothing otherwise.
// `need`, `have` and `cap` count whatever the site counts (bytes, words, chunks): alloc takes the
// capacity in that unit.  drop(old) frees or retires the old buffer; alloc(&fresh, cap) allocates;
// both return 0 or an error status, which is passed on.  Order: drop, (p, have) = (nullptr, 0),
// allocate, and the size is recorded only with the new buffer — so after any failure the pair is
// a consistent empty buffer, and the next call grows again instead of trusting a stale size.
template <class T, class S, class Drop, class Alloc>
int grow(T *&p, S &have, size_t need, size_t cap, Drop &&drop, Alloc &&alloc) {
    if (need <= have) return 0;
    int st = p ? drop(p) : 0;
    p = nullptr;
    have = 0;
    if (st) return st;
    T *fresh = nullptr;
    if ((st = alloc(&fresh, cap))) return st;
    p = fresh;
    have = static_cast<S>(cap);
    return 0;
}

}  // namespace psy
