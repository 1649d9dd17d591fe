// tdt_rawfb.h — the raw fallback (TDT_OPT_RAW_FALLBACK): a message whose TDT blob would be longer
// than its UNCP blob (marker + the message, n + 4 bytes) is stored as that UNCP blob instead.
//
// The encode kernels are left as they are.  Under the option every output slot is clamped to n + 4
// bytes before they run, so a message whose blob would be longer comes out of them as
// TDT_E_CAPACITY with nothing final written; a follow-up pass behind them, on the caller's stream,
// stores those messages raw:
//
//   flag    one lane per message: it is flagged when the encode left TDT_E_CAPACITY and the caller's
//           real capacity holds n + 4 bytes (or left TDT_OK with a length above n + 4, where a slot
//           could not be clamped).  The lane writes the final status and length, and raw_len[i] =
//           n + 4 for a flagged message, 0 for every other.  A message that took UNCP by the routing
//           is never flagged: its blob is n + 4 bytes, which fits whenever the capacity is n + 4.
//   scan    raw_len into n + 1 offsets: the flagged blobs laid end to end in a VIRTUAL buffer.
//   copy    split by the bytes of that virtual buffer, as the pack kernel splits its output
//           (tdt_pack.h: the same 64-ary search, pieces and walk; messages that are not flagged are
//           zero-length entries and fall out of the walk).  The piece of a blob goes to the blob's
//           OWN slot: blob bytes 0..3 are the marker, byte k >= 4 is message byte k - 4.
//
// The host calls have an option of their own (TDT_OPT_HOST_RAW_FALLBACK) with the same rule and a
// cheaper mechanism: the host pipeline's gather takes a flagged blob straight from the chunk's input on
// its way to host memory (host_raw_flag_kernel, host_raw_gather_kernel in tdt_api.hip), so nothing of the
// copy pass above runs there.  It shares the bound, raw_flagged and raw_span below.
//
// The bound, the decision and the segment arithmetic are plain host / device C++ here, so that a
// host program can drive them over offset tables (tests/cpp/test_raw_fallback_segments.cpp,
// tests/cpp/test_host_raw_parts.cpp); the kernels are in tdt_rawfb.hip.
#pragma once
#include <stdint.h>

#include "tdt_pack.h"

namespace psy {

constexpr uint32_t kRawMarkerBytes = 4;
constexpr uint32_t kRawMarker = 0x554E4350u;  // "UNCP", little-endian in the blob (kMagicUNCP)

// ---- the bound -----------------------------------------------------------------------------
// Worst-case blob of an n-byte message at word size ws: max(n + 4, 28 + 4·ws + 2n) without the
// fallback (tdt_encode_bound), n + 4 with it.
PSY_PACK_HD uint64_t raw_blob_bytes(uint64_t n) { return n + kRawMarkerBytes; }
PSY_PACK_HD uint64_t encode_bound_of(uint64_t n, uint32_t ws, bool raw_fallback) {
    const uint64_t raw = raw_blob_bytes(n), tdt = 28ull + 4ull * ws + 2ull * n;
    return raw_fallback || raw > tdt ? raw : tdt;
}

// ---- the decision --------------------------------------------------------------------------
// The statuses the rule looks at (TDT_OK, TDT_E_CAPACITY of psyne_tdt.h)
constexpr int32_t kRawStOk = 0, kRawStCapacity = 5;
// status / len: what the encode left for a message of n bytes whose slot was clamped to
// min(cap, n + 4); cap: the caller's real capacity.
PSY_PACK_HD bool raw_flagged(int32_t status, uint64_t len, uint64_t n, uint64_t cap) {
    const uint64_t raw = raw_blob_bytes(n);
    if (cap < raw) return false;
    return status == kRawStCapacity || (status == kRawStOk && len > raw);
}
// The size routes: min(E, n + 4) of an accepted message (a rejected one reports 0, which stays)
PSY_PACK_HD uint64_t raw_min_size(uint64_t enc, uint64_t n) {
    const uint64_t raw = raw_blob_bytes(n);
    return enc > raw ? raw : enc;
}

// ---- segments ------------------------------------------------------------------------------
// Blob [o0, o1) of the virtual buffer in piece pc (pack_walk gave PACK_COPY).  In the blob's own
// coordinates the segment is [b, b + len): its marker part — bytes marker_at .. marker_at +
// marker_n of the four marker bytes, at the same offsets of the slot — and its payload part:
// message bytes [src_off, src_off + len) to slot bytes [dst_off, dst_off + len), dst_off = src_off + 4.
struct RawSeg {
    uint32_t marker_at, marker_n;
    uint64_t src_off, dst_off, len;
};
// Bytes [b, e) of a raw blob, in the blob's own coordinates (b <= e <= n + 4).  The host pipeline's
// gather (TDT_OPT_HOST_RAW_FALLBACK, tdt_api.hip) calls it with a wave's part of the blob: part p of P
// of a blob of l = n + 4 bytes is raw_span(l * p / P, l * (p + 1) / P).
PSY_PACK_HD RawSeg raw_span(uint64_t b, uint64_t e) {
    RawSeg r{0u, 0u, 0u, 0u, 0u};
    if (b < kRawMarkerBytes) {
        r.marker_at = (uint32_t)b;
        r.marker_n = (uint32_t)((e < kRawMarkerBytes ? e : (uint64_t)kRawMarkerBytes) - b);
    }
    const uint64_t pb = b > kRawMarkerBytes ? b : (uint64_t)kRawMarkerBytes;
    if (e > pb) {
        r.src_off = pb - kRawMarkerBytes;
        r.dst_off = pb;
        r.len = e - pb;
    }
    return r;
}
PSY_PACK_HD RawSeg raw_segment(uint64_t o0, uint64_t o1, PackPiece pc) {
    const PackSeg s = pack_segment(o0, o1, pc);
    return raw_span(s.src_off, s.src_off + s.len);
}
PSY_PACK_HD uint8_t raw_marker_byte(uint32_t k) { return (uint8_t)(kRawMarker >> (8u * k)); }

// ---- the counter block (the snapshot scheme of the plan counters, tdt_plan.h) -----------------
enum RawCount : int {
    RC_FLAGGED = 0,  // messages of the call stored raw by the rule
};
constexpr int lo32(RawCount k) { return 2 * (int)k; }

// ---- launchers (tdt_rawfb.hip; `stream` is a hipStream_t; the result a hipError_t as int) ----
// cap_out[i] = min(cap[i], size[i] + 4)
int launch_raw_clamp(const uint64_t *size, const uint64_t *cap, uint64_t *cap_out, uint32_t n, void *stream);
// a contiguous slotted batch as a scattered one: ptr[i] = in + in_off[i], size[i], optr[i] = out +
// slot_off[i], cap[i] = slot_off[i + 1] - slot_off[i]
int launch_raw_contig(const uint8_t *in, const uint64_t *in_off, uint8_t *out, const uint64_t *slot_off, uint64_t *ptr,
                      uint64_t *size, uint64_t *optr, uint64_t *cap, uint32_t n, void *stream);
// the flag pass: status / len in place (the caller's arrays, or the call's workspace where the caller
// gave none), raw_len[i], *count += the flagged messages
int launch_raw_flag(const uint64_t *size, const uint64_t *cap, int32_t *status, uint64_t *len, uint64_t *raw_len,
                    unsigned long long *count, uint32_t n, void *stream);
// the copy: off[0..n] the scanned raw_len; msgs / blobs: the addresses of the messages and slots
int launch_raw_copy(const uint64_t *msgs, const uint64_t *blobs, const uint64_t *off, uint32_t n, uint32_t cut,
                    uint32_t grid, void *stream);
// the size routes: enc[i] = min(enc[i], n_i + 4), n_i = size[i] (in_off null) or in_off[i + 1] - in_off[i]
int launch_raw_min(const uint64_t *size, const uint64_t *in_off, uint64_t *enc, uint32_t n, void *stream);
// off[i] = size[i] + 4, or 0 for a width that has no blob (as launch_pack_bounds) — the scan's input
int launch_raw_bounds(const uint64_t *size, const int32_t *ws, int32_t ws_all, uint64_t mask, uint64_t *off, uint32_t n,
                      void *stream);
// off[0..n] = exclusive prefix of n_i + 4 over the messages of in_off (closed form, no scan)
int launch_raw_slots(const uint64_t *in_off, uint64_t *off, uint32_t n, void *stream);

}  // namespace psy
