// The arithmetic of the raw fallback's copy (psyne_amd/csrc/tdt_rawfb.h): the flagged blobs laid end
// to end in a virtual buffer, split into pieces as the pack kernel splits its output, every piece
// of a blob going to that blob's own slot — marker bytes for blob bytes 0..3, message byte k - 4 for
// blob byte k.  Driven over offset tables exactly as the kernel drives it.  Checked: every byte of
// every flagged blob is written exactly once with the right value, nothing of an unflagged message's
// slot is touched, and the bound and the decision are what the contract states.  Host code only;
// built with -fsanitize=address,undefined and run directly (tests/test_raw_fallback_segments.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../psyne_amd/csrc/tdt_rawfb.h"

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
const uint8_t kMarker[4] = {0x50, 0x43, 0x4E, 0x55};  // 0x554E4350, little-endian

uint8_t message_byte(uint32_t i, uint64_t k) { return (uint8_t)(i * 131u + k * 7u + (k >> 8) + 1u); }

// size[i]: the message's bytes; flagged[i]: the rule stores it raw.  Walks every piece as the kernel does.
void check_table(const std::vector<uint64_t> &size, const std::vector<bool> &flagged) {
    const uint32_t n = (uint32_t)size.size();
    std::vector<uint64_t> off(n + 1, 0);  // the scan of raw_len
    for (uint32_t i = 0; i < n; ++i) off[i + 1] = off[i] + (flagged[i] ? psy::raw_blob_bytes(size[i]) : 0);
    const uint64_t total = off[n];
    // every message's own slot, exactly n + 4 bytes, with a count of the writes to each byte
    std::vector<std::vector<uint8_t>> slot(n), hits(n);
    for (uint32_t i = 0; i < n; ++i) slot[i].assign(size[i] + 4, 0xEE), hits[i].assign(size[i] + 4, 0);
    uint64_t cursor = 0;  // the next byte of the virtual buffer a segment must begin at
    for (uint64_t piece = 0; piece < total / P + 2; ++piece) {
        const psy::PackPiece pc = psy::pack_piece(piece, total, ~0ull);
        if (pc.p0 >= pc.p1) {  // (nothing flagged: the first piece is empty and the launch leaves at once)
            CHECK(piece * P >= total);
            continue;
        }
        const uint32_t first = psy::pack_first_blob(off.data(), n, pc.p0);
        CHECK(first < n && flagged[first] && off[first] <= pc.p0 && pc.p0 < off[first + 1]);
        for (uint32_t b = first; b < n; ++b) {
            const psy::PackWalk wk = psy::pack_walk(off[b], off[b + 1], pc, ~0ull);
            if (wk == psy::PACK_END) break;
            if (wk == psy::PACK_SKIP) {
                CHECK(!flagged[b]);  // (a flagged blob holds at least its marker)
                continue;
            }
            CHECK(flagged[b]);
            const psy::RawSeg s = psy::raw_segment(off[b], off[b + 1], pc);
            const uint64_t begin = s.marker_n ? s.marker_at : s.dst_off, len = s.marker_n + s.len;
            CHECK(len > 0 && off[b] + begin == cursor);
            CHECK(s.marker_at + s.marker_n <= 4);
            if (s.marker_n && s.len) CHECK(s.marker_at + s.marker_n == 4 && s.dst_off == 4);
            if (s.len) CHECK(s.dst_off >= 4 && s.dst_off == s.src_off + 4 && s.src_off + s.len <= size[b]);
            CHECK(off[b] + begin >= pc.p0 && off[b] + begin + len <= pc.p1);
            for (uint32_t t = 0; t < s.marker_n; ++t) {
                slot[b][s.marker_at + t] = psy::raw_marker_byte(s.marker_at + t);
                ++hits[b][s.marker_at + t];
            }
            for (uint64_t k = 0; k < s.len; ++k) {
                slot[b][s.dst_off + k] = message_byte(b, s.src_off + k);
                ++hits[b][s.dst_off + k];
            }
            cursor = off[b] + begin + len;
        }
        CHECK(cursor == pc.p1);
    }
    CHECK(cursor == total);
    for (uint32_t i = 0; i < n; ++i) {
        bool ok = true;
        for (uint64_t k = 0; k < size[i] + 4; ++k) {
            if (!flagged[i]) ok = ok && hits[i][k] == 0 && slot[i][k] == 0xEE;
            else ok = ok && hits[i][k] == 1 && slot[i][k] == (k < 4 ? kMarker[k] : message_byte(i, k - 4));
        }
        CHECK(ok);
    }
}

void check_rule() {
    // the bound: n + 4 under the option, max(n + 4, 28 + 4 ws + 2n) without
    for (uint64_t n : {0ull, 1ull, 63ull, 1024ull, 65536ull, 1ull << 40})
        for (uint32_t ws : {1u, 4u, 12u, 64u}) {
            CHECK(psy::encode_bound_of(n, ws, true) == n + 4);
            CHECK(psy::encode_bound_of(n, ws, false) == std::max<uint64_t>(n + 4, 28 + 4ull * ws + 2 * n));
        }
    // the decision: TDT_E_CAPACITY (5) under a slot clamped to n + 4 means E > n + 4
    const uint64_t n = 1024;
    CHECK(psy::raw_flagged(5, 0, n, n + 4) && psy::raw_flagged(5, 0, n, 2 * n + 44));
    CHECK(!psy::raw_flagged(5, 0, n, n + 3));              // no room for the raw blob either
    CHECK(!psy::raw_flagged(0, n + 4, n, n + 4));          // the tie stays TDT; a routed UNCP blob too
    CHECK(!psy::raw_flagged(0, n + 2, n, 2 * n + 44));
    CHECK(psy::raw_flagged(0, n + 6, n, 2 * n + 44));      // a slot that could not be clamped
    CHECK(!psy::raw_flagged(4, 0, n, 2 * n + 44) && !psy::raw_flagged(8, 0, n, 2 * n + 44));  // other statuses stay
    CHECK(!psy::raw_flagged(5, 0, 0, 3) && !psy::raw_flagged(0, 4, 0, 4));  // size 0
    CHECK(psy::raw_min_size(n + 6, n) == n + 4 && psy::raw_min_size(n + 4, n) == n + 4 && psy::raw_min_size(n + 2, n) == n + 2);
    CHECK(psy::raw_min_size(0, n) == 0);
}

}  // namespace

int main() {
    std::mt19937_64 rng(20271);
    check_rule();
    // nothing flagged
    for (uint32_t n : {1u, 5u, 64u, 65u, 1000u}) check_table(std::vector<uint64_t>(n, 4096), std::vector<bool>(n, false));
    // one blob over many pieces, alone and between zero-length neighbours
    check_table({5 * P + 123}, {true});
    check_table({64, 64, 7 * P, 64, 64}, {false, false, true, false, false});
    // marker bytes split across a piece edge: the blob before ends 0..4 bytes before the edge
    for (uint64_t cut = 0; cut <= 5; ++cut) {
        check_table({P - 4 - cut, 3 * P, 100}, {true, true, true});
        check_table({P - 4 - cut, 0, 0, 1}, {true, false, true, true});
        check_table({2 * P - 4 - cut, 64, 1000}, {true, false, true});
    }
    // size-0 messages that are flagged hold the marker alone (the rule never flags one; the copy would still be right)
    check_table({0, 0, 0}, {true, true, true});
    // runs of unflagged messages at piece edges, longer than a batch of 64
    for (uint32_t run : {1u, 5u, 63u, 64u, 65u, 200u}) {
        std::vector<uint64_t> size{P - 4};
        std::vector<bool> fl{true};
        auto gap = [&] { size.insert(size.end(), run, 4096), fl.insert(fl.end(), run, false); };
        gap(), size.push_back(P - 7), fl.push_back(true);
        gap(), size.push_back(3), fl.push_back(true);
        gap(), size.push_back(2 * P + 1), fl.push_back(true);
        gap();
        check_table(size, fl);
    }
    // random tables
    for (int t = 0; t < 3000; ++t) {
        const uint32_t n = 1 + (uint32_t)(rng() % (t % 50 == 0 ? 400 : 60));
        std::vector<uint64_t> size(n);
        std::vector<bool> fl(n);
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t k = rng() % 100;
            size[i] = k < 40 ? rng() % 3000 : k < 80 ? 1024 * (1 + rng() % 8) : k < 95 ? (1 + rng() % 2) * P - 8 + rng() % 12
                                                                                       : rng() % (3 * P);
            fl[i] = rng() % 3 != 0;
        }
        check_table(size, fl);
    }
    std::printf("raw fallback segments: %d failures\n", failures);
    return failures ? 1 : 0;
}
