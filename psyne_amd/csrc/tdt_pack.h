// tdt_pack.h — slotted or scattered blobs into one packed wire buffer (tdt_pack_v, and the second
// phase of tdt_encode_batch_vp).
//
// Blob i goes to out[off[i] .. off[i+1]), off being the exclusive prefix sum of the lengths
// (n + 1 entries, the total at [n]).  The copy is split by OUTPUT BYTES, not by blob: one 512-lane
// workgroup takes one piece of kPackPiece bytes of the packed output — the shape of the codec's
// HBM copy (hbm_copy_kernel) — so a 256 MiB blob beside 4 KiB ones costs what its bytes cost, not
// one wave's serial walk over it.
//
//   search    the first blob reaching into piece [p0, p1) is the largest i with off[i] <= p0
//             (off[n] = total > p0, so it exists and is not empty; zero-length blobs before it
//             share its offset and lose to it).  A 64-ary search: every step the 64 lanes of a
//             wave probe 64 equally spaced entries with one load, and the count of probes at or
//             below p0 narrows the range 64-fold (pack_stride / pack_probe / pack_narrow).
//   segments  a segment is (blob ∩ piece).  The waves walk the blobs from the first one, 64
//             offsets per load; zero-length blobs fall out of the ballot.  A segment of at most
//             `cut` bytes is copied by one wave (segment s by wave s % 8), a longer one by all
//             eight waves, 16-byte chunk k by lane k % 512.
//   capacity  a blob with off[i+1] > out_cap is not copied (TDT_E_CAPACITY); the offsets ascend,
//             so the walk ends at the first such blob and no byte at or past out_cap is written.
//
// The arithmetic of the search and of the segments is plain host / device C++ here, so that a
// host program can drive it over offset tables (tests/cpp/test_pack_segments.cpp); the kernels
// are in tdt_pack.hip.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PSY_PACK_HD __host__ __device__ inline
#else
#define PSY_PACK_HD inline
#endif

namespace psy {

constexpr uint32_t kPackPiece = 65536;  // bytes of packed output per workgroup and step (512 lanes x 8 x 16)
constexpr uint32_t kPackLanes = 512;
constexpr uint32_t kPackWaves = kPackLanes / 64;
// Segments up to this many bytes go one per wave, longer ones across the workgroup; and the most
// workgroups of a launch (larger outputs are grid-strided).  Defaults of tdt_ctx_create; the
// measurements behind them are in DESIGN.md §5 (profiles/pack/).
constexpr uint32_t kPackCut = 4096;
constexpr uint32_t kPackGridCap = 16384;

// ---- the 64-ary search -------------------------------------------------------------------
// Range invariant: off[lo] <= p0 < off[hi], 0 <= lo < hi <= n.  Done when hi - lo == 1: blob lo.
struct PackRange {
    uint32_t lo, hi;
};
PSY_PACK_HD bool pack_found(PackRange r) { return r.hi - r.lo <= 1u; }
PSY_PACK_HD uint32_t pack_stride(PackRange r) { return (r.hi - r.lo + 63u) / 64u; }
// the entry lane `lane` probes in this step (at or past r.hi: none)
PSY_PACK_HD uint64_t pack_probe(PackRange r, uint32_t stride, uint32_t lane) {
    return (uint64_t)r.lo + (uint64_t)(lane + 1u) * stride;
}
// hits: the number of probes below r.hi with off[probe] <= p0 (a prefix of the lanes: off ascends)
PSY_PACK_HD PackRange pack_narrow(PackRange r, uint32_t stride, uint32_t hits) {
    const uint64_t lo = (uint64_t)r.lo + (uint64_t)hits * stride;
    const uint64_t hi = lo + stride < (uint64_t)r.hi ? lo + stride : (uint64_t)r.hi;
    return PackRange{(uint32_t)lo, (uint32_t)hi};
}
// The search as one thread runs it (the kernel takes `hits` from a ballot instead).  p0 < off[n].
PSY_PACK_HD uint32_t pack_first_blob(const uint64_t *off, uint32_t n, uint64_t p0) {
    PackRange r{0u, n};
    while (!pack_found(r)) {
        const uint32_t stride = pack_stride(r);
        uint32_t hits = 0;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const uint64_t j = pack_probe(r, stride, lane);
            if (j < r.hi && off[j] <= p0) ++hits;
        }
        r = pack_narrow(r, stride, hits);
    }
    return r.lo;
}

// ---- pieces and segments -----------------------------------------------------------------
// Piece `piece` covers [p0, p1) of the packed output; empty (p0 >= p1) at or past the end of what
// is copied at all: the total, or the capacity.
struct PackPiece {
    uint64_t p0, p1;
};
PSY_PACK_HD PackPiece pack_piece(uint64_t piece, uint64_t total, uint64_t out_cap) {
    const uint64_t lim = total < out_cap ? total : out_cap;
    const uint64_t p0 = piece * (uint64_t)kPackPiece;
    if (p0 >= lim) return PackPiece{p0, p0};
    return PackPiece{p0, lim - p0 < (uint64_t)kPackPiece ? lim : p0 + kPackPiece};
}
// What the walk does with blob [o0, o1) in piece pc.
enum PackWalk { PACK_SKIP = 0, PACK_COPY = 1, PACK_END = 2 };
PSY_PACK_HD PackWalk pack_walk(uint64_t o0, uint64_t o1, PackPiece pc, uint64_t out_cap) {
    if (o0 >= pc.p1 || o1 > out_cap) return PACK_END;  // (every later blob too: the offsets ascend)
    return o1 > o0 && o1 > pc.p0 ? PACK_COPY : PACK_SKIP;
}
// The segment of blob [o0, o1) in piece pc (pack_walk gave PACK_COPY): bytes [src_off, src_off +
// len) of the blob go to [dst_off, dst_off + len) of the packed output.
struct PackSeg {
    uint64_t src_off, dst_off, len;
};
PSY_PACK_HD PackSeg pack_segment(uint64_t o0, uint64_t o1, PackPiece pc) {
    const uint64_t b = o0 > pc.p0 ? o0 : pc.p0, e = o1 < pc.p1 ? o1 : pc.p1;
    return PackSeg{b - o0, b, e - b};
}

// ---- sizes-first slots (tdt_encode_batch_vp with TDT_OPT_PACK_SIZES_FIRST) -------------------------
// The blobs' exact sizes are known before a byte is written (the size pass), so blob i is encoded
// straight into the packed output: its slot is [o0, o1) = [off[i], off[i+1]) of it when that ends
// inside out_cap, and a slot of capacity 0 — TDT_E_CAPACITY, no byte written — when it does not.
// The offsets ascend, so the accepted slots tile [0, min(total, out_cap)) up to the first blob
// that ends past out_cap, and every slot from that blob on has capacity 0.
struct PackSlot {
    uint64_t off, cap;  // blob i at out + off, `cap` bytes
};
PSY_PACK_HD PackSlot pack_exact_slot(uint64_t o0, uint64_t o1, uint64_t out_cap) {
    return PackSlot{o0, o1 <= out_cap ? o1 - o0 : 0u};
}

// ---- launchers (tdt_pack.hip; `stream` is a hipStream_t; the result a hipError_t as int) ----
// off[0..n] holds the scanned lengths.  status (may be null): TDT_E_CAPACITY for blob i with
// off[i+1] > out_cap, else TDT_OK — or, with keep_errors, left as it is unless it was TDT_OK.
int launch_pack(const uint64_t *blobs, const uint64_t *off, uint32_t n, uint8_t *out, uint64_t out_cap,
                int32_t *status, bool keep_errors, uint32_t cut, uint32_t grid_cap, void *stream);
// off[i] = the encode bound of size[i] bytes at width ws[i] (ws null: ws_all); 0 for a width outside
// 1..64 or, with ws given, one whose bit (w - 1) of mask is clear: such a message has no blob
int launch_pack_bounds(const uint64_t *size, const int32_t *ws, int32_t ws_all, uint64_t mask, uint64_t *off, uint32_t n,
                       void *stream);
// slot i = buf + off[i], its capacity off[i+1] - off[i], or 0 where the slot would end past buf_bytes
int launch_pack_slots(const uint64_t *off, uint8_t *buf, uint64_t buf_bytes, uint64_t *ptr, uint64_t *cap,
                      uint32_t n, void *stream);

// ptr[i] = out + off[i] and cap[i] as pack_exact_slot gives it for out_cap
int launch_pack_exact_slots(const uint64_t *off, uint8_t *out, uint64_t out_cap, uint64_t *ptr, uint64_t *cap,
                            uint32_t n, void *stream);

}  // namespace psy
