// The part arithmetic of the host pipeline's raw gather (TDT_OPT_HOST_RAW_FALLBACK; raw_span of
// psyne_amd/csrc/tdt_rawfb.h): wave part p of P of a flagged blob of l = n + 4 bytes is blob bytes
// [l * p / P, l * (p + 1) / P) — marker bytes for blob bytes 0..3, message byte k - 4 for blob byte k.
// Driven exactly as host_raw_gather_kernel drives it, into an arena between canaries.  Checked: every
// blob byte is written exactly once, the result is marker + message, no canary is touched, and a span
// reads only message bytes.  Host code only; built with -fsanitize=address,undefined and run directly
// (tests/test_host_raw_parts.py).
#include <cstdint>
#include <cstdio>
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

constexpr uint64_t kGuard = 64;
constexpr uint8_t kCanary = 0xA5;
const uint8_t kMarker[4] = {0x50, 0x43, 0x4E, 0x55};  // 0x554E4350, little-endian

uint8_t message_byte(uint64_t k) { return (uint8_t)(k * 7u + (k >> 8) + 1u); }

void check_blob(uint64_t n, uint32_t P) {
    const uint64_t l = psy::raw_blob_bytes(n);
    CHECK(l == n + 4);
    std::vector<uint8_t> msg(n);
    for (uint64_t k = 0; k < n; ++k) msg[k] = message_byte(k);
    std::vector<uint8_t> arena(kGuard + l + kGuard, kCanary), hits(l, 0);
    uint8_t *o = arena.data() + kGuard;
    uint64_t cursor = 0;  // the parts tile the blob in order
    for (uint32_t p = 0; p < P; ++p) {
        const uint64_t a = l * p / P, e = l * (p + 1) / P;
        CHECK(a == cursor && e >= a && e <= l);
        cursor = e;
        if (e <= a) continue;  // (the kernel skips an empty part)
        const psy::RawSeg s = psy::raw_span(a, e);
        CHECK(s.marker_n + s.len == e - a);
        CHECK(s.marker_at + s.marker_n <= 4);
        if (s.marker_n) CHECK(s.marker_at == a);
        if (s.marker_n && s.len) CHECK(s.marker_at + s.marker_n == 4 && s.dst_off == 4);
        if (s.len) CHECK(s.dst_off >= 4 && s.dst_off == s.src_off + 4 && s.src_off + s.len <= n);
        if (s.len && !s.marker_n) CHECK(s.dst_off == a);
        for (uint32_t t = 0; t < s.marker_n; ++t) {  // (lane t of the wave)
            o[s.marker_at + t] = psy::raw_marker_byte(s.marker_at + t);
            ++hits[s.marker_at + t];
        }
        for (uint64_t k = 0; k < s.len; ++k) {  // (the shared copy, msg + src_off -> o + dst_off)
            o[s.dst_off + k] = msg[s.src_off + k];
            ++hits[s.dst_off + k];
        }
    }
    CHECK(cursor == l);
    bool once = true, bytes = true, guards = true;
    for (uint64_t k = 0; k < l; ++k) {
        once = once && hits[k] == 1;
        bytes = bytes && o[k] == (k < 4 ? kMarker[k] : message_byte(k - 4));
    }
    for (uint64_t k = 0; k < kGuard; ++k) guards = guards && arena[k] == kCanary && arena[kGuard + l + k] == kCanary;
    CHECK(once);
    CHECK(bytes);
    CHECK(guards);
}

}  // namespace

int main() {
    std::vector<uint64_t> sizes;
    for (uint64_t n = 0; n <= 70; ++n) sizes.push_back(n);
    for (uint64_t n : {1023ull, 4096ull, 65537ull}) sizes.push_back(n);
    for (uint64_t n : sizes)
        for (uint32_t P = 1; P <= 64; ++P) check_blob(n, P);
    // the pack-piece form is the same span of the blob's own coordinates
    const psy::PackPiece pc = psy::pack_piece(0, 3000, ~0ull);
    const psy::RawSeg a = psy::raw_segment(0, 1028, pc), b = psy::raw_span(0, 1028);
    CHECK(a.marker_at == b.marker_at && a.marker_n == b.marker_n && a.src_off == b.src_off && a.dst_off == b.dst_off &&
          a.len == b.len);
    std::printf("host raw parts: %d failures\n", failures);
    return failures ? 1 : 0;
}
