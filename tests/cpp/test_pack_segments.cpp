// The piece-to-segments arithmetic of the pack kernel (psyne_amd/csrc/tdt_pack.h): the 64-ary
// search for a piece's first blob and the walk over its (blob ∩ piece) segments, driven over
// length tables exactly as the kernel drives them.  Checked: the segments of all pieces tile
// [0, what fits) once and in order, and map every output byte to the right source byte.  Host
// code only; built with -fsanitize=address,undefined and run directly (tests/test_pack_segments.py).
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

constexpr uint64_t P = psy::kPackPiece;
constexpr uint64_t kNoCap = ~0ull;

std::vector<uint64_t> offsets(const std::vector<uint64_t> &len) {
    std::vector<uint64_t> off(len.size() + 1, 0);
    for (size_t i = 0; i < len.size(); ++i) off[i + 1] = off[i] + len[i];
    return off;
}

// byte k of blob i
uint8_t source_byte(uint32_t i, uint64_t k) { return (uint8_t)(i * 131u + k * 7u + (k >> 8) + 1u); }

// Walks every piece as the kernel does.  bytes: also move the bytes and compare them.
void check_table(const std::vector<uint64_t> &len, uint64_t cap, bool bytes) {
    const uint32_t n = (uint32_t)len.size();
    const std::vector<uint64_t> off = offsets(len);
    const uint64_t total = off[n];
    // what must be covered: the blobs that end at or before cap (a prefix: the offsets ascend)
    uint64_t fit = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (off[i + 1] <= cap) fit = off[i + 1];
    std::vector<uint8_t> out, hits;
    if (bytes) out.assign(fit, 0), hits.assign(fit, 0);
    uint64_t cursor = 0;      // the next output byte a segment must begin at
    uint32_t last_blob = 0;   // segments come in blob order
    const uint64_t pieces = std::min(total, cap) / P + 2;  // (and pieces past the end: they are empty)
    for (uint64_t piece = 0; piece < pieces; ++piece) {
        const psy::PackPiece pc = psy::pack_piece(piece, total, cap);
        if (pc.p0 >= pc.p1) {
            CHECK(piece * P >= std::min(total, cap));
            continue;
        }
        CHECK(pc.p0 == piece * P && pc.p1 - pc.p0 <= P && pc.p1 <= std::min(total, cap));
        const uint32_t first = psy::pack_first_blob(off.data(), n, pc.p0);
        // the largest i with off[i] <= p0: not empty, and the blob that holds byte p0
        CHECK(first < n && off[first] <= pc.p0 && pc.p0 < off[first + 1]);
        for (uint32_t b = first; b < n; ++b) {
            const psy::PackWalk wk = psy::pack_walk(off[b], off[b + 1], pc, cap);
            if (wk == psy::PACK_END) break;
            if (wk == psy::PACK_SKIP) {
                CHECK(len[b] == 0);
                continue;
            }
            const psy::PackSeg s = psy::pack_segment(off[b], off[b + 1], pc);
            CHECK(s.len > 0 && s.dst_off == cursor && b >= last_blob);
            CHECK(s.dst_off >= pc.p0 && s.dst_off + s.len <= pc.p1);
            CHECK(s.src_off + s.len <= len[b] && s.dst_off - s.src_off == off[b]);
            CHECK(off[b + 1] <= cap);
            if (bytes && s.dst_off + s.len <= fit)
                for (uint64_t k = 0; k < s.len; ++k) {
                    out[s.dst_off + k] = source_byte(b, s.src_off + k);
                    ++hits[s.dst_off + k];
                }
            cursor = s.dst_off + s.len;
            last_blob = b;
        }
        // a piece ends where the next begins, unless the capacity cut a blob off inside it
        CHECK(cursor == pc.p1 || cursor == fit);
    }
    CHECK(cursor == fit);
    if (bytes) {
        uint64_t x = 0;
        bool ok = true;
        for (uint32_t i = 0; i < n && off[i + 1] <= cap; ++i)
            for (uint64_t k = 0; k < len[i]; ++k, ++x) ok = ok && hits[x] == 1 && out[x] == source_byte(i, k);
        CHECK(ok && x == fit);
    }
}

void check_all_caps(const std::vector<uint64_t> &len, bool bytes) {
    const std::vector<uint64_t> off = offsets(len);
    check_table(len, kNoCap, bytes);
    check_table(len, 0, bytes);
    check_table(len, off.back(), bytes);
    if (off.back()) check_table(len, off.back() - 1, bytes);
    for (size_t i = 0; i < off.size() && i < 40; ++i) {  // at a blob's end, and inside a blob
        check_table(len, off[i], bytes);
        if (i + 1 < off.size() && off[i + 1] - off[i] > 1) check_table(len, off[i] + (off[i + 1] - off[i]) / 2, bytes);
    }
}

// the search alone, against a linear scan, on tables long enough for three steps
void check_search(std::mt19937_64 &rng) {
    for (uint32_t n : {1u, 2u, 63u, 64u, 65u, 4095u, 4096u, 4097u, 262144u, 300001u}) {
        std::vector<uint64_t> len(n);
        for (auto &l : len) l = rng() % 4 == 0 ? 0 : rng() % 3000;
        len[rng() % n] += 1;  // (not all empty)
        const std::vector<uint64_t> off = offsets(len);
        uint32_t want = 0;
        for (uint64_t p0 = 0; p0 < off[n]; p0 += std::max<uint64_t>(1, off[n] / 257)) {
            while (off[want + 1] <= p0) ++want;
            CHECK(psy::pack_first_blob(off.data(), n, p0) == want);
        }
        CHECK(psy::pack_first_blob(off.data(), n, off[n] - 1) == (uint32_t)(std::upper_bound(off.begin(), off.end(), off[n] - 1) - off.begin() - 1));
    }
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261);
    // all zeros
    for (uint32_t n : {1u, 5u, 64u, 65u, 1000u}) check_all_caps(std::vector<uint64_t>(n, 0), true);
    // a single blob of many pieces
    check_all_caps({5 * P + 123}, true);
    check_all_caps({0, 0, 7 * P, 0}, true);
    // lengths around the piece size
    for (uint64_t l : {P - 1, P, P + 1}) {
        check_all_caps({l}, true);
        check_all_caps({l, l, l}, true);
        check_all_caps({1, l, 0, l, 17}, true);
    }
    check_all_caps({P - 1, P, P + 1, P + 1, P, P - 1}, true);
    // runs of zero-length blobs at piece boundaries: before, at and after them, and longer than a batch of 64
    for (uint32_t run : {1u, 5u, 63u, 64u, 65u, 200u}) {
        std::vector<uint64_t> len{P};
        len.insert(len.end(), run, 0);
        len.push_back(P - 3);
        len.insert(len.end(), run, 0);
        len.push_back(3);
        len.insert(len.end(), run, 0);
        len.push_back(2 * P + 1);
        len.insert(len.end(), run, 0);
        check_all_caps(len, true);
    }
    // random tables
    for (int t = 0; t < 10000; ++t) {
        const uint32_t n = 1 + (uint32_t)(rng() % (t % 50 == 0 ? 400 : 60));
        std::vector<uint64_t> len(n);
        for (auto &l : len) {
            const uint64_t k = rng() % 100;
            if (k < 30) l = 0;
            else if (k < 60) l = rng() % 40;
            else if (k < 85) l = rng() % 3000;
            else if (k < 97) l = (1 + rng() % 2) * P - 2 + rng() % 5;
            else l = rng() % (3 * P);
        }
        const std::vector<uint64_t> off = offsets(len);
        const bool bytes = t < 300;
        check_table(len, kNoCap, bytes);
        check_table(len, off[n] ? rng() % (off[n] + 1) : 0, bytes);
        check_table(len, off[rng() % (n + 1)], bytes);
    }
    check_search(rng);
    std::printf("pack segments: %d failures\n", failures);
    return failures ? 1 : 0;
}
