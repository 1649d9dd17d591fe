// The slot arithmetic of the sizes-first packed encode (psyne_amd/csrc/tdt_pack.h: pack_exact_slot),
// driven over length tables exactly as the kernel drives it: one slot per blob from the scanned
// lengths and the output's capacity.  Checked: the accepted slots tile [0, fit) in blob order
// without gap or overlap, fit being where the last blob that ends inside out_cap ends (so
// fit <= min(total, out_cap), with equality when out_cap lies on a blob boundary or past the
// total); and every slot from the first blob that ends past out_cap on has capacity 0.  Host code
// only; built with -fsanitize=address,undefined and run directly (tests/test_sizes_first_slots.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../psyne_amd/csrc/tdt_pack.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

std::vector<uint64_t> offsets(const std::vector<uint64_t> &len) {
    std::vector<uint64_t> off(len.size() + 1, 0);
    for (size_t i = 0; i < len.size(); ++i) off[i + 1] = off[i] + len[i];
    return off;
}

void check_table(const std::vector<uint64_t> &len, uint64_t cap) {
    const uint32_t n = (uint32_t)len.size();
    const std::vector<uint64_t> off = offsets(len);
    const uint64_t total = off[n];
    // the cut: the first blob that ends past cap (n: none).  The offsets ascend, so every blob
    // before it ends inside cap and every blob from it on ends past cap.
    uint32_t cut = n;
    for (uint32_t i = 0; i < n; ++i)
        if (off[i + 1] > cap) {
            cut = i;
            break;
        }
    uint64_t cursor = 0;  // the next byte an accepted slot must begin at
    for (uint32_t i = 0; i < n; ++i) {
        const psy::PackSlot s = psy::pack_exact_slot(off[i], off[i + 1], cap);
        CHECK(s.off == off[i]);
        if (i < cut) {
            CHECK(s.cap == len[i]);           // the blob's exact size
            CHECK(s.off == cursor);           // in order, no gap, no overlap
            CHECK(s.off + s.cap <= cap);      // inside the output
            cursor = s.off + s.cap;
        } else {
            CHECK(s.cap == 0);                // past the cut: nothing may be written
        }
    }
    const uint64_t fit = cut < n ? off[cut] : total;
    CHECK(cursor == fit);
    CHECK(fit <= std::min(total, cap));
    if (cap >= total) CHECK(cut == n && fit == total);
    // out_cap on a blob boundary (or past the total): the accepted slots cover all of min(total, out_cap)
    if (std::find(off.begin(), off.end(), cap) != off.end()) CHECK(fit == std::min(total, cap));
}

// out_cap of 0, at every blob boundary and one byte either side of it, and at / past the total
void check_every_cut(const std::vector<uint64_t> &len) {
    const std::vector<uint64_t> off = offsets(len);
    check_table(len, 0);
    for (uint64_t b : off) {
        if (b > 0) check_table(len, b - 1);
        check_table(len, b);
        check_table(len, b + 1);
    }
    check_table(len, off.back() + 12345);
    check_table(len, ~0ull);
}

}  // namespace

int main() {
    check_every_cut({});
    check_every_cut({0});
    check_every_cut({1});
    check_every_cut({0, 0, 0});
    check_every_cut({4, 0, 68, 0, 0, 1028, 17, 0});
    check_every_cut({0, 0, 5, 0, 0});
    // one huge entry (beyond 2^32 and near 2^62) among small ones and zeros
    check_every_cut({44, 0, (1ull << 33) + 7, 12, 0, 3});
    check_every_cut({(1ull << 62), 1, 0, 2});
    check_every_cut({3, (1ull << 62) - 5, 0, 9});
    // random tables with runs of zeros
    std::mt19937_64 rng(20263);
    for (int t = 0; t < 200; ++t) {
        std::vector<uint64_t> len(1 + rng() % 40);
        for (auto &l : len) {
            const uint64_t k = rng() % 8;
            l = k < 3 ? 0 : k < 6 ? rng() % 300 : k == 6 ? rng() % (1u << 20) : (rng() % (1ull << 40));
        }
        check_every_cut(len);
    }
    std::printf("sizes-first slots: %d failures\n", failures);
    return failures ? 1 : 0;
}
