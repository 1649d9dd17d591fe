// tdt_decode.h — batched TDT decode for CDNA4 (gfx950), v2: one wave per blob.
//
// Restates include/psyne/protocol/tdt_compression.hpp (reference):
//   decode                  :271-304  size < 4 → error; UNCP → payload; else TDT
//   TDTEncodedData::deserialize :119-170 (+ the bounds checks the reference lacks)
//   simple_rle_decompress   :596-612  pairs while i+1 < len; count 0 emits nothing
//   recombine_byte_streams  :614-637  zero-initialised output; short streams leave zeros
//
// Work decomposition: one 64-lane wave per blob (no workgroup barrier, many
// blobs in flight per CU).  The output is produced in WINDOWS of WR rounds; a round is 64
// 16-byte groups (lane l ↔ group l).  Per window and referenced stream r (k_r byte positions
// per word, so 64·WR·WPG·k_r stream positions):
//   1. pairs, 8 per lane per pair-round, are prefix-summed (in-lane + DPP wave scan) and each
//      writes a HEAD key (position tag) << 8 | value at its start position into an
//      LDS array (positions past the window land in a pad slot); the pairs that start in the
//      window are consumed (a ballot finds the boundary lane, a scalar walk the exact pair);
//   2. per round, lane l owns 16 consecutive positions of the round's concatenated stream
//      planes: a packed u16 prefix-max (v_pk_max_u16) fills every position with the last
//      head before it — the key's position tag makes "last" the maximum — seeded by a wave
//      max-scan over lanes (and the stream's carry from the previous round);
//   3. lane l gathers its group's bytes of every stream from the planes (4 dword LDS reads
//      when stream segments are dword-sized) and scatters them into word order with
//      v_perm_b32 selectors (recombine_byte_streams), one 16-byte store per lane.
#pragma once
#include "tdt_device.h"
#include "tdt_encode.h"
#include "tdt_plan.h"

namespace psy {

struct DMeta;

struct DecodeArgs {
    const uint8_t *in;
    const uint64_t *in_off;
    uint32_t n_msgs;
    uint8_t *out;
    uint64_t out_cap;
    uint64_t *out_off;
    int32_t *status;
    uint64_t *sizes_out;  // sizes-only mode
    uint64_t *lookback;
    uint32_t *ticket;
    uint32_t *errflags;
    const uint64_t *slot_off;  // slotted outputs (LB = 0)
    uint64_t *out_len;
    const uint64_t *in_len;  // optional blob lengths (blob i = in[in_off[i] .. +in_len[i]))
    // slotted batches: blob ids from the plan's list
    const uint32_t *list;
    const uint32_t *list_count;  // the list's length (device memory: the plan's counter)
    uint32_t list_base;
    // (main list only) blobs decoding to more than big_min bytes, dispatched before `list`: a
    // one-wave blob of up to 1 MiB started late would run alone in the kernel's tail
    const uint32_t *blist;
    const uint32_t *blist_count;
    // the plan's counters (u32 view, lo32(): DC_LARGE, DC_TILES, DC_BLOCKS claimed) and the
    // budgets it ran with
    const uint32_t *pcnt;
    uint32_t lcap, tcap, bcap;
    // large blobs (tiled path)
    DMeta *dmeta;
    const uint32_t *bent;  // block-slot entries (large-blob index)
    uint32_t *bsum;        // per 512-pair block: count sum, then (scan) start position
    const uint32_t *tent;  // tile entries (large-blob index)
    uint32_t *tblk;        // per tile and referenced stream: the block holding its position - 1
    // blobs of a generic word size (tdt_anyws.h): the kernels here place them and append their
    // ids to dlist (length *dcount, one atomic each); a follow-up launch decodes the listed blobs
    uint32_t *dlist;
    uint32_t *dcount;
};

// blob_check's internal status of a valid blob whose word size (<= 64, not 1/2/4/8/16) the
// kernels of this file do not decode: deferred to tdt_anyws.hip.  Never reported to the caller.
constexpr uint32_t ST_DEFER = 0x100;

constexpr int kMaxRef = 16;  // referenced streams <= word_size <= 16
constexpr uint32_t kDecTileGroups = 2048;  // large blobs: 32 KiB of output per tile
#ifndef PSY_DEC_WR
#define PSY_DEC_WR 3
#endif
constexpr int kDecWR = PSY_DEC_WR;  // rounds per window
#ifndef PSY_DEC_REBASE_LOG2
#define PSY_DEC_REBASE_LOG2 28  // decode_fast rebases its held pair starts every 2^this positions
#endif
constexpr int kHdrCache = 256;

template <int WR = kDecWR>
struct DecLayoutT {
    // Fast path (decode_fast): the two referenced streams' heads, WR·64·seg_r + 16 pad u16 each
    // (seg_0 + seg_1 = 16); a round's plane bytes are staged inside the heads of that round
    // (already read by the fill) and zeroed after the gather.
    static constexpr int FHEADS = (WR * 1024 + 32) * 2;
    // (the fast path's heads start 16 bytes in: the u16 before stream 0's heads is the pad slot
    // of pairs that start before the window — stream 1's is the last pad slot of stream 0)
    static constexpr int OFF_FHEADS = 16;
    // Generic path (any shape, up to 16 referenced streams): windows of GWR rounds, its own
    // planes and the lane-0 parser's fields.
    static constexpr int GWR = 1;
    static constexpr int GHEADS = (GWR * 1024 + 16 * kMaxRef) * 2;
    static constexpr int PLANES = 1024 + 64;  // one round of plane bytes (+ slack)
    static constexpr int MISC = 192 * 4;      // D_* fields
    // The header cache is read only while the blob's header is parsed, before any heads write.
    static constexpr int OFF_HDR = 0;
    static constexpr int OFF_HEADS = 0;
    static constexpr int OFF_GPLANES = GHEADS;
    // One-round windows (the small-blob list): the fast path's heads end at 2128 and the generic
    // path writes only MISC before its heads, so [OFF_BLOB, OFF_BLOB + BLOBC) holds the blob's
    // first BLOBC bytes for the whole decode — a blob of up to BLOBC bytes is read from HBM in ONE
    // trip and its header, stream table and pair blocks come from LDS.  2,112 bytes hold a whole
    // 1 KiB message's blob at word size 4 (2,092 B when every run has length 1, uniform bytes);
    // MISC moves past the cache, 5,024 B per wave: still 8 waves per SIMD.
#ifndef PSY_DEC_BLOBC
#define PSY_DEC_BLOBC 2112
#endif
    static constexpr int OFF_BLOB = WR == 1 ? 2144 : OFF_HDR;
    static constexpr int BLOBC = WR == 1 ? PSY_DEC_BLOBC : kHdrCache;
    static constexpr int OFF_MISC = WR == 1 && OFF_BLOB + BLOBC > OFF_GPLANES + PLANES ? OFF_BLOB + BLOBC
                                                                                      : OFF_GPLANES + PLANES;
    static constexpr int GBYTES = OFF_MISC + MISC;
    static constexpr int BYTES = OFF_FHEADS + FHEADS > GBYTES ? OFF_FHEADS + FHEADS : GBYTES;
    static_assert(kHdrCache + 16 <= GHEADS && kHdrCache + 16 <= FHEADS, "header cache inside the heads");
    static_assert(WR != 1 || 32 * ((BYTES + 511) / 512 * 512) <= 160 * 1024, "8 one-wave decodes per SIMD");
    static_assert(WR != 1 || (OFF_BLOB >= OFF_FHEADS + FHEADS && OFF_BLOB % 16 == 0 && BLOBC % 16 == 0 &&
                              OFF_BLOB + BLOBC <= OFF_MISC && OFF_BLOB + BLOBC + 20 <= BYTES),
                  "blob cache beside the fast path's heads, before MISC (+20: a pair block's 5-dword over-read)");
};
using DecLayout = DecLayoutT<>;

// misc (uint32 index)
enum {
    D_MSG = 0, D_STATUS = 1, D_UNCP = 2, D_ORIG = 3, D_WS = 4, D_NREF = 5, D_BASE = 6 /*u64*/, D_FAST = 8,
    D_K = 16, D_SOFF = 32, D_NP = 48, D_OA = 64 /*4*/, D_OB = 68 /*4*/, D_SB = 72 /*16: S byte → (r<<8)|off*/,
    D_PIDX = 96, D_POS = 112, D_CV = 128, D_SLEN = 144, D_HOFF = 160, D_PB = 176
};

// 16 bytes at p (any alignment): aligned dword loads + v_alignbyte when the aligned span
// ends inside [p, lim); byte-exact (zero-filled past `valid`) otherwise.
__device__ __forceinline__ uint4 ld16_span(const uint8_t *p, int valid, const uint8_t *lim) {
    const uintptr_t a = (uintptr_t)p;
    const uintptr_t a0 = a & ~(uintptr_t)3;
    if (valid >= 16 && a0 + 20 <= (uintptr_t)lim) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(a0);
        const uint32_t sh = (uint32_t)(a & 3);
        const uint32_t w0 = gload<uint32_t>(q), w1 = gload<uint32_t>(q + 1), w2 = gload<uint32_t>(q + 2),
                       w3 = gload<uint32_t>(q + 3), w4 = gload<uint32_t>(q + 4);
        if (sh == 0) return make_uint4(w0, w1, w2, w3);
        return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                          __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
    }
    return ld16_any(p, valid);
}

// Header validation of one blob: decode :271-304 (size < 4, magic), deserialize :119-170
// (header, mapping and stream table must lie inside the blob — the reference has no bounds
// checks there) and recombine_byte_streams :614-637's preconditions (word_size > 0, every
// mapping entry < num_streams whenever a word exists).  rd32(off) reads the u32 at blob
// offset off (only called for offsets proven inside the blob).  osize = the decoded size
// (original_size, or len - 4 for UNCP), 0 on error.  A blob that passes every check but has a
// word size the kernels here do not take returns, last, ST_DEFER (word size <= 64: osize =
// original_size, the generic kernel decodes it) or ST_UNSUPPORTED (word size > 64).
// (Written as one status chain without early returns: the hipcc 7.2 structurizer dropped the
// success value of osize when the checks returned from inside the loops.)
template <class RD>
__device__ __forceinline__ uint32_t blob_check(RD &&rd32, uint64_t len, uint32_t &uncp, uint64_t &osize) {
    uint32_t st = ST_OK, orig = 0;
    uncp = 0;
    if (len < 4) {
        st = ST_SHORT;
    } else {
        const uint32_t magic = rd32(0);
        if (magic == kMagicUNCP) {
            uncp = 1;
        } else if (magic != kMagicTDT) {
            st = ST_MAGIC;
        } else if (len < 20) {
            st = ST_TRUNCATED;
        } else {
            orig = rd32(4);
            const uint32_t ns = rd32(8);
            const uint32_t ws = rd32(12);
            const uint32_t msize = rd32(16);
            uint64_t off = 20 + 4ull * msize;
            if (off > len) st = ST_TRUNCATED;
            for (uint32_t s = 0; s < ns && st == ST_OK; ++s) {
                if (off + 4 > len) {
                    st = ST_TRUNCATED;
                } else {
                    const uint32_t sl = rd32(off);
                    off += 4;
                    if (off + sl > len) st = ST_TRUNCATED;
                    off += sl;
                }
            }
            const int32_t wsi = (int32_t)ws;
            if (st == ST_OK && wsi == 0) st = ST_BAD_HEADER;
            const uint64_t wc = wsi > 0 ? orig / (uint64_t)wsi : 0;
            if (st == ST_OK && wc > 0) {
                if (msize < ws) st = ST_BAD_MAPPING;
                for (uint32_t b = 0; b < ws && st == ST_OK; ++b) {
                    const int32_t m = (int32_t)rd32(20 + 4 * b);
                    if (m < 0 || (uint32_t)m >= ns) st = ST_BAD_MAPPING;
                }
                if (st == ST_OK && (ws > 16 || (16 % ws) != 0)) st = ws <= 64 ? ST_DEFER : ST_UNSUPPORTED;
            }
        }
    }
    osize = (st != ST_OK && st != ST_DEFER) ? 0ull : uncp ? len - 4 : (uint64_t)orig;
    return st;
}

#ifndef PSY_DEC_INST_TU  // (the non-template kernels are defined once, in tdt_api.hip)
// Decoded sizes (and statuses) only: one lane per blob, no LDS — the header words sit in the
// first cache lines of each blob.
__global__ __launch_bounds__(256) void tdt_decode_sizes_kernel(DecodeArgs a) {
    const uint32_t msg = blockIdx.x * 256u + threadIdx.x;
    if (msg >= a.n_msgs) return;
    const uint64_t boff = a.in_off[msg];
    const uint64_t len = a.in_len ? a.in_len[msg] : a.in_off[msg + 1] - boff;
    const uint8_t *blob = a.in + boff;
    const bool al4 = ((uintptr_t)blob & 3) == 0;
    // the first 48 bytes (header, a word-size-4 mapping, the first stream's length) in one burst
    // of independent loads: the header check then waits on memory once more at most (the second
    // stream's length), instead of once per field
    uint32_t w[12];
    const bool pre = al4 && len >= 48;
    if (pre) {
        if (((uintptr_t)blob & 15) == 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 v = *reinterpret_cast<const uint4 *>(blob + 16 * q);
                w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) w[k] = *reinterpret_cast<const uint32_t *>(blob + 4 * k);
        }
    }
    auto rd32 = [&](uint64_t off) -> uint32_t {
        if (pre && off < 48 && (off & 3) == 0) {
            uint32_t v = w[0];
#pragma unroll
            for (int k = 1; k < 12; ++k) v = (off >> 2) == (uint64_t)k ? w[k] : v;
            return v;
        }
        return (al4 && (off & 3) == 0) ? *reinterpret_cast<const uint32_t *>(blob + off) : ld_u32_bytes(blob + off);
    };
    uint32_t uncp;
    uint64_t osize;
    const uint32_t st = blob_check(rd32, len, uncp, osize);
    a.sizes_out[msg] = osize;
    if (a.status) a.status[msg] = (int32_t)(st == ST_DEFER ? (uint32_t)ST_OK : st);  // (a generic width decodes)
}
#endif  // PSY_DEC_INST_TU

// ---------------------------------------------------------------------------------------
// Fast path: at most two referenced streams whose per-group segments seg_r = WPG·k_r are
// whole dwords (every blob psyne's encoder writes for word_size 4 has this shape).
//
// Pair BLOCKS: a stream is read in blocks of 512 pairs (8 per lane, one 16-byte load per
// lane); a block is prefix-summed ONCE into absolute start positions st[i] (invalid pairs —
// count 0 or past the stream — get start ~0) and packed head keys, and stays in registers
// across output windows until the window passes its end.  Per window and block, every pair
// writes its key at slot min(st - wstart, wlen): pairs outside the window land in the pad
// slot, so the write is branch-free (3 VALU + 1 ds_write_b16 per pair).
//
// Keys are gen << 13 | (16 + pos mod 16) << 8 | value (a 5-bit tag, 0 = no head) with gen =
// window index mod 8, so the head array is only zeroed every 8 windows: stale keys compare
// below the current window's seed key (gen << 13 | value) and below every current head.
//
// Fill, per round of 64 groups: lane l owns 16 consecutive positions of the round's two
// stream planes (stream 0: lanes [0, 4·seg0), stream 1 after); an in-lane u16 prefix max,
// seeded by a wave max-scan of each lane's last head (restricted to its own stream) or by the
// stream's carry, gives every position its run's value.  Planes → LDS; each lane gathers its
// group's segments (dword reads) and v_perm's them into word order (recombine :614-637).

// Parameters of a fast-path blob (parse_fast): referenced streams r = 0, 1 (stream 1 absent
// when !two) with seg[r] = WPG·k_r bytes per 16-byte group, np[r] pairs at blob offset soff[r].
struct FastHdr {
    uint32_t kind;  // 0: not fast (lane-0 parser + generic path), 1: UNCP, 2: TDT fast path
    uint32_t orig, ws, two;
    uint32_t seg[2], np[2], soff[2];
    uint32_t OA[4], OB[4];
    uint32_t rkind;  // recombine form (RecLayout::rkind); OA / OB then hold its selectors
    uint64_t osize;
};

// Groups [g_lo, g_hi) of the output (the whole blob, or one tile of a large one).  A tile that
// starts inside the blob begins at block b0[r] of stream r — the 512-pair block holding
// position g_lo·seg_r - 1, whose first pair starts at s0[r] (the scan's prefix); kNone: the
// stream ends before the tile (s0 = its length).
// pair-block dword loads (PSY_DEC_LDNT: non-temporal)
__device__ __forceinline__ uint32_t gload_blk(const uint32_t *p) {
#ifdef PSY_DEC_LDNT
    return __builtin_nontemporal_load((const __attribute__((address_space(1))) uint32_t *)(p));
#else
    return gload<uint32_t>(p);
#endif
}

template <int WR_ = kDecWR>
__device__ __forceinline__ void decode_fast(const FastHdr &H, uint8_t *smem, const uint8_t *blob, const uint8_t *blim,
                                            uint8_t *dst, uint32_t ngroups, uint64_t wbytes, uint32_t g_lo = 0,
                                            uint32_t g_hi = 0, const uint32_t *b0 = nullptr, const uint32_t *s0 = nullptr,
                                            const uint8_t *bc = nullptr, uint32_t bcl = 0) {
    using Lay = DecLayoutT<WR_>;
    constexpr uint32_t WR = WR_;
    const uint32_t lane = (uint32_t)lane_id();
    PSY_PROF_BEGIN();
    uint16_t *heads = reinterpret_cast<uint16_t *>(smem + Lay::OFF_FHEADS);
    // (every field is wave-uniform: readfirstlane keeps them in SGPRs)
    auto U = [](uint32_t x) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };
    const bool two = U(H.two) != 0;
    const uint32_t seg[2] = {U(H.seg[0]), two ? U(H.seg[1]) : 0u};
    const uint32_t np[2] = {U(H.np[0]), two ? U(H.np[1]) : 0u};
    const uint32_t soff[2] = {U(H.soff[0]), two ? U(H.soff[1]) : 0u};
    const uint32_t OA[4] = {U(H.OA[0]), U(H.OA[1]), U(H.OA[2]), U(H.OA[3])};
    const uint32_t OB[4] = {U(H.OB[0]), U(H.OB[1]), U(H.OB[2]), U(H.OB[3])};
    const uint32_t rkind = U(H.rkind);
    const uint32_t wlen[2] = {WR * 64u * seg[0], WR * 64u * seg[1]};
    const uint32_t hbase[2] = {(uint32_t)Lay::OFF_FHEADS, (uint32_t)Lay::OFF_FHEADS + 2u * (wlen[0] + 16u)};
    // round rl's plane bytes go to the heads of round rl of the stream with the larger segment
    // (128·seg >= 1 KiB bytes, 16-byte aligned), which the fill has read by then
    const uint32_t rbig = seg[1] > seg[0] ? 1u : 0u;
    const uint32_t pl_base = hbase[rbig], pl_step = 128u * seg[rbig];
    // fill lane
    const bool f1 = lane * 16u >= 64u * seg[0];
    const uint32_t fu = f1 ? lane * 16u - 64u * seg[0] : lane * 16u;
    const uint32_t fseg = f1 ? seg[1] : seg[0];
    // scan tags: (lane + 1) << 8, + 64 << 8 on stream-1 lanes; lthr: the lowest tag of this
    // lane's stream
    const uint32_t ltag = (lane + 1u + (f1 ? 64u : 0u)) << 8;
    const uint32_t lthr = f1 ? (65u << 8) : (1u << 8);
    const uint32_t fh = (f1 ? hbase[1] : hbase[0]) + 2u * fu;
    const uint32_t last_lane0 = 4u * seg[0] - 1u;  // lane holding stream 0's last plane byte
    // recombine: S dword d (S = the group's seg[0] stream-0 bytes, then its seg[1] stream-1
    // bytes) = plane bytes sd_pb[d] + lane·sd_mul[d] (4 bytes of one stream: seg[r] % 4 == 0),
    // held per lane (sd_off: VGPRs, so the round loop needs no SGPRs for them)
    uint32_t sd_pb[4], sd_mul[4], sd_off[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t r = 4u * (uint32_t)d >= seg[0] ? 1u : 0u;
        const uint32_t u = 4u * (uint32_t)d - (r ? seg[0] : 0u);
        sd_pb[d] = (r ? 64u * seg[0] : 0u) + u;
        sd_mul[d] = r ? seg[1] : seg[0];
        sd_off[d] = sd_pb[d] + lane * sd_mul[d];
    }

    // streams held whole in the LDS blob cache (bc: the blob's first bcl bytes, decode_one's
    // small-blob list): their pair blocks are LDS reads, not dependent HBM trips
    const bool cached[2] = {bc != nullptr && soff[0] + 2u * np[0] <= bcl, bc != nullptr && soff[1] + 2u * np[1] <= bcl};

    // per stream block state (uniform) and registers (per lane)
    uint32_t bidx[2] = {0u, 0u};      // pair index of the NEXT block to load
    uint32_t bend[2] = {0u, 0u};      // absolute end position of the loaded block
    uint32_t slen[2] = {~0u, ~0u};    // decoded stream length once its last block is loaded
    bool have[2] = {false, false};
    // pair starts are held as st = 2·(start - P0[r]) (signed; P0 = the stream position of group
    // g_lo, rebased forward every 2^28 positions), with bit 31 set on count-0 pairs; a window's
    // key address is then med3(st - c, lo, hi): 2 VALU per pair, pairs outside the window (or
    // without a count) landing on the pad u16 just before or after the stream's heads
    int32_t P0[2] = {(int32_t)(g_lo * seg[0]), (int32_t)(g_lo * seg[1])};
    int32_t st[2][8];
    uint32_t kp[2][4];  // packed keys without gen: key(2j) | key(2j+1) << 16
    uint32_t cv[2] = {0u, 0u};  // carry: value of the last plane position of the previous round
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int i = 0; i < 8; ++i) st[r][i] = INT32_MIN;
#pragma unroll
        for (int j = 0; j < 4; ++j) kp[r][j] = 0u;
    }

    auto load_block = [&](int r) __attribute__((always_inline)) {
        const uint32_t p0 = bidx[r] + 8u * lane;
        // (uniform) a block before the stream's last: every lane holds 8 pairs, read with plain
        // aligned dword loads (the dword after them, read when the pairs are not dword-aligned,
        // holds a byte of the next pair: no bounds tests) — else the checked, zero-filled load
        const bool full = bidx[r] + 512u < np[r];
        uint4 pv;
        if (cached[r]) {
            // 5 dword LDS reads + alignbyte; past the stream's end the bytes are zeroed (a lane
            // without pairs reads the block's first, in-range, bytes)
            const uint32_t nv = full ? 8u : (p0 < np[r] ? (np[r] - p0 < 8u ? np[r] - p0 : 8u) : 0u);
            const uint32_t sh = soff[r] & 3u;
            const uint32_t *q =
                reinterpret_cast<const uint32_t *>(bc + (soff[r] & ~3u) + 2u * (nv ? p0 : bidx[r]));
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
            if (sh == 0u) {
                pv = make_uint4(w0, w1, w2, w3);
            } else {
                const uint32_t w4 = q[4];
                pv = make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                                __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
            }
            if (!full) {
                const uint32_t vb = 2u * nv;  // valid bytes (even: 0, 2 or 4 per dword)
                uint32_t m[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t kq = vb <= 4u * j ? 0u : (vb - 4u * j >= 4u ? 4u : vb - 4u * j);
                    m[j] = kq >= 4u ? 0xffffffffu : ((1u << (8u * kq)) - 1u);
                }
                pv = make_uint4(pv.x & m[0], pv.y & m[1], pv.z & m[2], pv.w & m[3]);
            }
        } else if (full) {
            const uint8_t *sb = blob + soff[r];
            const uint32_t sh = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uintptr_t)sb & 3u));
            const uint32_t *q = reinterpret_cast<const uint32_t *>(((uintptr_t)sb & ~(uintptr_t)3) + 2ull * p0);
            const uint32_t w0 = gload_blk(q), w1 = gload_blk(q + 1), w2 = gload_blk(q + 2), w3 = gload_blk(q + 3);
            if (sh == 0u) {
                pv = make_uint4(w0, w1, w2, w3);
            } else {
                const uint32_t w4 = gload_blk(q + 4);
                pv = make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                                __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
            }
        } else {
            const uint32_t nv = p0 < np[r] ? (np[r] - p0 < 8u ? np[r] - p0 : 8u) : 0u;
            pv = nv ? ld16_span(blob + soff[r] + 2ull * p0, (int)(2 * nv), blim) : make_uint4(0, 0, 0, 0);
        }
        const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w};
        const uint32_t cw[4] = {pw[0] & 0x00ff00ffu, pw[1] & 0x00ff00ffu, pw[2] & 0x00ff00ffu, pw[3] & 0x00ff00ffu};
        const uint32_t s2 = cw[0] + cw[1] + cw[2] + cw[3];
        const uint32_t tot = (s2 & 0xffffu) + (s2 >> 16);
        const uint32_t linc = wave_incl_scan<OpAdd>(tot);
        // this lane's first start - P0 (P0 % 16 == 0: the low 4 bits are the position mod 16)
        uint32_t run = bend[r] - (uint32_t)P0[r] + linc - tot;
        // (uniform) a full block whose pairs all carry a count (psyne's encoder writes no count-0
        // pairs; past a stream's end the zero-filled loads do): starts held without the flag
        bool counted = false;
#ifndef PSY_X_NOCOUNTED
        if (full) {
            const uint32_t mn = pk_min_u16(pk_min_u16(cw[0], cw[1]), pk_min_u16(cw[2], cw[3]));
            counted = !__any((mn & 0xffffu) == 0u || (mn >> 16) == 0u);
        }
#endif
        if (counted) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t w = pw[j];
                const uint32_t r0 = run, r1 = run + (w & 0xffu);
                run = r1 + ((w >> 16) & 0xffu);
                st[r][2 * j] = (int32_t)add_self(r0);
                st[r][2 * j + 1] = (int32_t)add_self(r1);
                const uint32_t T = (perm(r1, r0, 0x0c0c0400u) & 0x0f0fu) | 0x1010u;
                kp[r][j] = perm(T, w, 0x05030401u);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t w = pw[j];
                const uint32_t c0 = w & 0xffu, c1 = (w >> 16) & 0xffu;
                const uint32_t r0 = run, r1 = run + c0;
                run = r1 + c1;
                // (pairs past the stream's end were loaded as zero bytes: count 0, no extra test)
                st[r][2 * j] = (int32_t)((r0 << 1) | ((c0 + 0xffffffffu) & 0x80000000u));
                st[r][2 * j + 1] = (int32_t)((r1 << 1) | ((c1 + 0xffffffffu) & 0x80000000u));
                // keys (16 + pos mod 16) << 8 | value: tags 16..31 (0 = empty), values = bytes 1
                // and 3 of the dword
                const uint32_t T = (perm(r1, r0, 0x0c0c0400u) & 0x0f0fu) | 0x1010u;
                kp[r][j] = perm(T, w, 0x05030401u);
            }
        }
        bend[r] += rdlane(linc, 63);
        bidx[r] += 512u;
        have[r] = true;
        if (bidx[r] >= np[r]) slen[r] = bend[r];
    };
    auto write_keys = [&](int r, uint32_t wstart, uint32_t genk) __attribute__((always_inline)) {
        const int32_t c = 2 * ((int32_t)wstart - P0[r]) - (int32_t)hbase[r];
        const int32_t lo = (int32_t)hbase[r] - 2, hi = (int32_t)(hbase[r] + 2u * wlen[r]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t k = kp[r][j] | genk;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int32_t v = (int32_t)((uint32_t)st[r][2 * j + h] - (uint32_t)c);
                const int32_t a = med3_i32(v, lo, hi);  // (lo, hi: VGPR copies, per window)
#ifndef PSY_X_NOKEYS
                *reinterpret_cast<uint16_t *>(smem + a) = (uint16_t)(h ? (k >> 16) : k);
#else
                if (a == 0xfffff) *reinterpret_cast<uint16_t *>(smem + hbase[r]) = (uint16_t)k;
#endif
            }
        }
    };

    if (g_hi == 0) g_hi = ngroups;
    if (g_lo > 0) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !two) break;
            const uint32_t P = g_lo * seg[r];
            const uint32_t b = U(b0[r]), sp = U(s0[r]);
            if (b == 0xffffffffu) {  // the stream ended before this tile: zeros
                bidx[r] = np[r];
                bend[r] = sp;
                slen[r] = sp;
                continue;
            }
            bidx[r] = 512u * b;
            bend[r] = sp;
            {
                // the carry: the value at position P - 1, i.e. of the last pair with a count that
                // starts at or before P - 1 (it lies in block b; starts of counted pairs increase)
                const uint32_t p0 = bidx[r] + 8u * lane;
                const uint32_t nv = p0 < np[r] ? (np[r] - p0 < 8u ? np[r] - p0 : 8u) : 0u;
                const uint4 pv =
                    nv ? ld16_span(blob + soff[r] + 2ull * p0, (int)(2 * nv), blim) : make_uint4(0, 0, 0, 0);
                const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w};
                uint32_t tot = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) tot += (pw[j] & 0xffu) + ((pw[j] >> 16) & 0xffu);
                uint32_t run = sp + wave_incl_scan<OpAdd>(tot) - tot;
                bool any = false;
                uint32_t bv = 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t w = pw[i >> 1] >> (16 * (i & 1));
                    const uint32_t cnt = w & 0xffu;
                    if (cnt != 0u && run <= P - 1u) {
                        any = true;
                        bv = (w >> 8) & 0xffu;
                    }
                    run += cnt;
                }
                const uint64_t who = __ballot(any);
                cv[r] = who ? rdlane(bv, 63 - (int)__builtin_clzll(who)) : 0u;
            }
            load_block(r);
        }
    }
    const bool dal16 = ((uintptr_t)dst & 15) == 0;
    // whole 16-byte groups of the output (a 32-bit uniform compare per round: gfx9 has no scalar
    // u64 less-than)
    const uint32_t wg16 = (uint32_t)(wbytes >> 4);
    uint32_t win = 0;
    for (uint32_t gwin = g_lo; gwin < g_hi; gwin += 64u * WR, ++win) {
        const uint32_t gen = win & 7u;
        if (gen == 0) {
            // (re)initialise the head array every 8 windows
            for (uint32_t i = lane; i < (uint32_t)Lay::FHEADS / 16; i += 64)
                reinterpret_cast<uint4 *>(heads)[i] = make_uint4(0, 0, 0, 0);
            team_sync<1>();
        }
        const uint32_t genk = (gen << 13) | (gen << 29);
        // ---- pairs → heads
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !two) break;
            const uint32_t wstart = gwin * seg[r], wend = wstart + wlen[r];
            if (wstart - (uint32_t)P0[r] >= (1u << PSY_DEC_REBASE_LOG2)) {
                // rebase the held starts (kept within +-2^30 of the window: the key address
                // arithmetic is 32-bit; positions per call reach 2^32)
                const uint32_t d = wstart - (uint32_t)P0[r];
                P0[r] = (int32_t)wstart;
#pragma unroll
                for (int i = 0; i < 8; ++i) st[r][i] = (int32_t)((uint32_t)st[r][i] - 2u * d);
            }
            if (have[r]) write_keys(r, wstart, genk);
            // blocks whose first pair starts inside this window
            while (bend[r] < wend && bidx[r] < np[r]) {
                load_block(r);
                write_keys(r, wstart, genk);
            }
        }
        team_sync<1>();
        PSY_PROF_MARK(9);
        // ---- per round: fill, recombine, store
        for (uint32_t rl = 0; rl < WR; ++rl) {
            const uint32_t g0 = gwin + rl * 64u;
            if (g0 >= g_hi) break;
            const uint32_t hoffb = fh + 2u * rl * 64u * fseg;
            uint8_t *const planes = smem + pl_base + rl * pl_step;
            // lanes 8-15 of every 16 read their second half first: with 32-byte lane rows the
            // two ds_read_b128 are then bank-conflict-free (MI355X_MICROARCH.md §LDS groups)
#ifndef PSY_DEC_NOSWAP
            const bool sw = (lane & 8u) != 0u;
            const uint4 ha = *reinterpret_cast<const uint4 *>(smem + hoffb + (sw ? 16u : 0u));
            const uint4 hb = *reinterpret_cast<const uint4 *>(smem + hoffb + (sw ? 0u : 16u));
            const uint4 h0 = sw ? hb : ha, h1 = sw ? ha : hb;
#else
            const uint4 h0 = *reinterpret_cast<const uint4 *>(smem + hoffb);
            const uint4 h1 = *reinterpret_cast<const uint4 *>(smem + hoffb + 16u);
#endif
            uint32_t x[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
            uint32_t m = pk_max_u16(pk_max_u16(pk_max_u16(x[0], x[1]), pk_max_u16(x[2], x[3])),
                                    pk_max_u16(pk_max_u16(x[4], x[5]), pk_max_u16(x[6], x[7])));
            m = pk_max_self_lo(m) >> 16;
            // a current head exists in the lane iff the max key carries this window's gen and a
            // tag (older gens only hold smaller keys); the lane's tag orders the scan, stream-1
            // lanes tagged above every stream-0 lane, so one compare tells a head earlier in the
            // lane's own stream plane from the carry
            const uint32_t lk = m >= ((gen << 13) | 0x1000u) ? perm(ltag, m, 0x07060500u) : 0u;
            const uint32_t ex = wave_shr1(wave_incl_scan<OpMax>(lk), 0u);
            const uint32_t carry = f1 ? cv[1] : cv[0];
            const uint32_t seedv = ex >= lthr ? (ex & 0xffu) : carry;
            const uint32_t seed = (gen << 13) | seedv;
            x[0] = pk_max_u16(x[0], seed);
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = pk_max_self_lo(x[q]);
#pragma unroll
            for (int q = 1; q < 8; ++q) x[q] = pk_max_bcast_hi(x[q], x[q - 1]);
            uint32_t bw[4] = {perm(x[1], x[0], 0x06040200u), perm(x[3], x[2], 0x06040200u),
                              perm(x[5], x[4], 0x06040200u), perm(x[7], x[6], 0x06040200u)};
            // a stream that ran out of pairs leaves zeros (recombine :626-631)
            const uint32_t rend0 = (g0 + 64u) * seg[0], rend1 = (g0 + 64u) * seg[1];
            if (slen[0] < rend0 || (two && slen[1] < rend1)) {
                const uint32_t sl = f1 ? slen[1] : slen[0];
                const uint32_t p0 = g0 * fseg + fu;
                const uint32_t keep = sl <= p0 ? 0u : (sl - p0 >= 16u ? 16u : sl - p0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t kq = keep <= 4u * q ? 0u : (keep - 4u * q >= 4u ? 4u : keep - 4u * q);
                    bw[q] &= kq >= 4u ? 0xffffffffu : ((1u << (8u * kq)) - 1u);
                }
            }
            cv[0] = rdlane(bw[3], (int)last_lane0) >> 24;
            if (two) cv[1] = rdlane(bw[3], 63) >> 24;
            *reinterpret_cast<uint4 *>(planes + 16u * lane) = make_uint4(bw[0], bw[1], bw[2], bw[3]);
            team_sync<1>();
            uint32_t S[4];
            if (seg[0] == 8u && seg[1] == 8u) {  // two streams of 8 bytes: 2 x ds_read_b64
                const uint2 s0 = *reinterpret_cast<const uint2 *>(planes + lane * 8u);
                const uint2 s1 = *reinterpret_cast<const uint2 *>(planes + 512u + lane * 8u);
                S[0] = s0.x, S[1] = s0.y, S[2] = s1.x, S[3] = s1.y;
            } else if (seg[0] == 16u) {  // one stream: ds_read_b128
                const uint4 s0 = *reinterpret_cast<const uint4 *>(planes + lane * 16u);
                S[0] = s0.x, S[1] = s0.y, S[2] = s0.z, S[3] = s0.w;
            } else {
#pragma unroll
                for (int d = 0; d < 4; ++d)
                    S[d] = *reinterpret_cast<const uint32_t *>(planes + sd_off[d]);
            }
            uint4 o;
            if (rkind == 1u) {
                o = make_uint4(perm(S[3], S[0], OA[0]), perm(S[3], perm(S[1], S[0], OB[1]), OA[1]),
                               perm(S[3], perm(S[2], S[1], OB[2]), OA[2]), perm(S[3], S[2], OA[3]));
            } else if (rkind == 3u) {
                o = make_uint4(perm(S[2], S[0], OA[0]), perm(S[2], S[0], OA[1]), perm(S[3], S[1], OA[2]),
                               perm(S[3], S[1], OA[3]));
            } else if (rkind == 2u) {
                o = make_uint4(perm(S[0], S[1], OA[0]), perm(S[0], perm(S[2], S[1], OB[1]), OA[1]),
                               perm(S[0], perm(S[3], S[2], OB[2]), OA[2]), perm(S[0], S[3], OA[3]));
            } else if (rkind == 4u) {
                o = make_uint4(S[0], S[1], S[2], S[3]);
            } else {
                o = make_uint4(perm(S[1], S[0], OA[0]) | perm(S[3], S[2], OB[0]),
                               perm(S[1], S[0], OA[1]) | perm(S[3], S[2], OB[1]),
                               perm(S[1], S[0], OA[2]) | perm(S[3], S[2], OB[2]),
                               perm(S[1], S[0], OA[3]) | perm(S[3], S[2], OB[3]));
            }
            const uint32_t g = g0 + lane;
            if (dal16 && g0 + 64u <= wg16) {
                // a whole aligned round (uniform): one 16-byte store per lane, no per-lane tests
#ifndef PSY_X_NOSTORE
                st16_nt(dst + 16ull * g, o);
#else
                if (o.x == 0x12345678u && o.y == 0x9abcdef0u) *reinterpret_cast<uint4 *>(dst + 16ull * g) = o;
#endif
            } else if (g < ngroups) {
                const uint64_t vb64 = wbytes - 16ull * g;
                st16_any(dst + 16ull * g, o, vb64 >= 16 ? 16 : (int)vb64);
            }
            // the planes' bytes are heads slots again: empty for the windows that follow (the
            // gather's reads precede these writes in the wave's LDS order)
            *reinterpret_cast<uint4 *>(planes + 16u * lane) = make_uint4(0, 0, 0, 0);
        }
        PSY_PROF_MARK(10);
    }
}

// Recombine layout of a blob with at most two streams, word size <= 8, as a function of its
// mapping bits (bit b = mapping[b] in {0, 1}): the referenced stream of first use (r = 0) holds
// mapping[0]'s value; two = both values occur; seg[r] = bytes of stream r per 16-byte group;
// OA / OB = the v_perm selectors that scatter a group's S dwords (its seg[0] bytes of stream
// r = 0, then its seg[1] bytes of stream r = 1) into word order (recombine :614-637): output
// byte i = word i / ws, position b = i % ws → S byte (r_b ? seg0 : 0) + (i / ws)·k_b + rank_b.
// Compiled into constant tables (parse_fast's general derivation handles everything else).
// Word size 4 has four S-dword structures with cheaper forms than 2 v_perm + v_or per output
// dword (rkind; OA / OB then hold their selectors): 1 — segments 12 + 4: words 0 and 3 one v_perm
// of two S dwords, words 1 and 2 two chained v_perm (S0|S1 or S1|S2, then S3); 2 — segments
// 4 + 12: the same with S0 as the shared dword; 3 — segments 8 + 8: one v_perm per word; 4 — one
// stream: the S dwords are the words.  0: the general form.
struct RecLayout {
    uint32_t two, m0, seg0, seg1, OA[4], OB[4], rkind;
};
template <int WS>
struct RecTable {
    RecLayout e[1 << WS];
};
template <int WS>
constexpr RecLayout make_rec_layout(uint32_t mb) {
    RecLayout L{};
    constexpr uint32_t WPG = 16 / WS;
    const uint32_t m0 = mb & 1u;
    uint32_t k[2] = {0, 0};
    for (int b = 0; b < WS; ++b) k[(mb >> b) & 1u]++;
    L.m0 = m0;
    L.two = (k[0] && k[1]) ? 1u : 0u;
    L.seg0 = WPG * k[m0];
    L.seg1 = L.two ? WPG * k[m0 ^ 1u] : 0u;
    uint32_t A[4] = {0x0c0c0c0cu, 0x0c0c0c0cu, 0x0c0c0c0cu, 0x0c0c0c0cu}, B[4] = {0x0c0c0c0cu, 0x0c0c0c0cu, 0x0c0c0c0cu, 0x0c0c0c0cu};
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t b = i % WS, v = (mb >> b) & 1u;
        uint32_t rank = 0;
        for (uint32_t bb = 0; bb < b; ++bb) rank += ((mb >> bb) & 1u) == v ? 1u : 0u;
        const uint32_t sidx = (v == m0 ? 0u : L.seg0) + (i / WS) * k[v] + rank;
        const uint32_t q = i >> 2, sh = 8u * (i & 3u);
        if (sidx < 8) A[q] = (A[q] & ~(0xffu << sh)) | (sidx << sh);
        else B[q] = (B[q] & ~(0xffu << sh)) | ((sidx - 8) << sh);
    }
    for (int q = 0; q < 4; ++q) {
        L.OA[q] = A[q];
        L.OB[q] = B[q];
    }
    L.rkind = 0;
    if (WS == 4) {
        uint32_t sx[16];  // S byte of output byte i
        for (uint32_t i = 0; i < 16; ++i) {
            const uint32_t b = i % WS, v = (mb >> b) & 1u;
            uint32_t rank = 0;
            for (uint32_t bb = 0; bb < b; ++bb) rank += ((mb >> bb) & 1u) == v ? 1u : 0u;
            sx[i] = (v == m0 ? 0u : L.seg0) + (i / WS) * k[v] + rank;
        }
        // selector byte j of word q from the S byte s: `lo` = the low operand's first S byte,
        // `hi` = the high operand's (0x0c: a zero byte)
        bool ok = true;  // every output byte has a source in its form (else the general form)
        auto sel = [&](uint32_t q, uint32_t lo, uint32_t hi, uint32_t lo_n, bool partial = false) -> uint32_t {
            uint32_t r = 0;
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t x = sx[4 * q + j];
                uint32_t t = 0x0c;
                if (x >= lo && x < lo + lo_n) t = x - lo;
                else if (x >= hi && x < hi + 4) t = 4 + (x - hi);
                else if (!partial) ok = false;
                r |= t << (8 * j);
            }
            return r;
        };
        // chained second step: bytes of the first step's result (t: bytes lo..lo+7) pass as j,
        // the rest come from the shared dword at `hi`
        auto sel2 = [&](uint32_t q, uint32_t lo, uint32_t hi) -> uint32_t {
            uint32_t r = 0;
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t x = sx[4 * q + j];
                const bool inl = x >= lo && x < lo + 8;
                if (!inl && !(x >= hi && x < hi + 4)) ok = false;
                r |= (inl ? j : 4 + (x - hi)) << (8 * j);
            }
            return r;
        };
        uint32_t sA[4] = {L.OA[0], L.OA[1], L.OA[2], L.OA[3]}, sB[4] = {L.OB[0], L.OB[1], L.OB[2], L.OB[3]};
        uint32_t rk = 0;
        if (L.seg0 == 12 && L.seg1 == 4) {
            rk = 1;  // o0 = perm(S3, S0), o1 = perm(S3, perm(S1, S0)), o2 = perm(S3, perm(S2, S1)), o3 = perm(S3, S2)
            sA[0] = sel(0, 0, 12, 4);
            sB[1] = sel(1, 0, 99, 8, true);
            sA[1] = sel2(1, 0, 12);
            sB[2] = sel(2, 4, 99, 8, true);
            sA[2] = sel2(2, 4, 12);
            sA[3] = sel(3, 8, 12, 4);
        } else if (L.seg0 == 4 && L.seg1 == 12) {
            rk = 2;  // o0 = perm(S0, S1), o1 = perm(S0, perm(S2, S1)), o2 = perm(S0, perm(S3, S2)), o3 = perm(S0, S3)
            sA[0] = sel(0, 4, 0, 4);
            sB[1] = sel(1, 4, 99, 8, true);
            sA[1] = sel2(1, 4, 0);
            sB[2] = sel(2, 8, 99, 8, true);
            sA[2] = sel2(2, 8, 0);
            sA[3] = sel(3, 12, 0, 4);
        } else if (L.seg0 == 8 && L.seg1 == 8) {
            rk = 3;  // o_q = perm(S[2 + q/2], S[q/2])
            for (uint32_t q = 0; q < 4; ++q) sA[q] = sel(q, 4 * (q >> 1), 8 + 4 * (q >> 1), 4);
        } else if (L.seg0 == 16) {
            rk = 4;  // one stream: o_q = S_q
            for (uint32_t i = 0; i < 16; ++i) ok = ok && sx[i] == i;
        }
        if (rk && ok) {
            L.rkind = rk;
            for (int q = 0; q < 4; ++q) {
                L.OA[q] = sA[q];
                L.OB[q] = sB[q];
            }
        }
    }
    return L;
}
template <int WS>
constexpr RecTable<WS> make_rec_table() {
    RecTable<WS> t{};
    for (uint32_t mb = 0; mb < (1u << WS); ++mb) t.e[mb] = make_rec_layout<WS>(mb);
    return t;
}
static __constant__ RecTable<1> c_rec1 = make_rec_table<1>();
static __constant__ RecTable<2> c_rec2 = make_rec_table<2>();
static __constant__ RecTable<4> c_rec4 = make_rec_table<4>();
static __constant__ RecTable<8> c_rec8 = make_rec_table<8>();

// Wave-parallel header parse (decode :271-304, deserialize :119-170, recombine :614-637) for
// the blobs the fast path takes: UNCP, or a valid TDT blob with word size 1/2/4/8/16, at most
// 16 streams, a mapping inside the header cache, at most two referenced streams whose
// per-group segments are whole dwords, and wc > 0.  Anything else (errors included) returns
// kind 0 and goes through the lane-0 parser (blob_check) and the generic path, which assign
// the reference's status codes.  hdr: the blob's first 256 bytes (zero-padded) in LDS.
__device__ __forceinline__ FastHdr parse_fast(const uint8_t *blob, uint64_t len, const uint8_t *hdr, uint32_t hcl) {
    const uint32_t lane = (uint32_t)lane_id();
    FastHdr h{};
    h.kind = 0;
    auto hw = [&](uint32_t off) -> uint32_t { return *reinterpret_cast<const uint32_t *>(hdr + off); };  // off % 4 == 0
    if (len < 4) return h;
    const uint32_t magic = hw(0);
    if (magic == kMagicUNCP) {
        h.kind = 1;
        h.osize = len - 4;
        return h;
    }
    if (magic != kMagicTDT || len < 20) return h;
    const uint32_t orig = hw(4), ns = hw(8), ws = hw(12), msize = hw(16);
    if (!(ws == 1 || ws == 2 || ws == 4 || ws == 8 || ws == 16) || msize < ws || ns == 0 || ns > 16) return h;
    if (20u + 4u * msize + 4u > hcl || orig / ws == 0) return h;
    if (ns <= 2 && ws <= 8) {
        // one or two streams, word size <= 8 (every blob the encoder writes for ws <= 8): the
        // stream table is two length words, the recombine layout a table entry
        const uint32_t m = lane < ws ? hw(20 + 4 * lane) : 0u;
        if (__any(lane < ws && m >= ns)) return h;  // (also negative values) → BAD_MAPPING via blob_check
        const uint32_t mb = (uint32_t)__ballot(lane < ws && m == 1u);
        uint64_t off = 20ull + 4ull * msize;
        if (off + 4 > len) return h;
        const uint32_t l0 = hw((uint32_t)off);  // (off + 4 <= hcl, off % 4 == 0)
        const uint32_t o0 = (uint32_t)off + 4u;
        if ((uint64_t)o0 + l0 > len) return h;
        uint32_t o1 = 0, l1 = 0;
        if (ns == 2) {
            const uint64_t t1 = (uint64_t)o0 + l0;
            if (t1 + 4 > len) return h;
            l1 = t1 + 4 <= hcl ? ld_u32_bytes(hdr + t1) : ld_u32_bytes(blob + t1);
            o1 = (uint32_t)t1 + 4u;
            if ((uint64_t)o1 + l1 > len) return h;
        }
        const RecLayout &R = ws == 1 ? c_rec1.e[mb] : ws == 2 ? c_rec2.e[mb] : ws == 4 ? c_rec4.e[mb] : c_rec8.e[mb];
        const uint32_t seg0 = R.seg0, seg1 = R.seg1;
        if ((seg0 & 3u) || (seg1 & 3u)) return h;
        const bool first1 = R.m0 != 0;  // stream 1 is used first: it is r = 0
        h.soff[0] = first1 ? o1 : o0;
        h.np[0] = (first1 ? l1 : l0) / 2u;
        h.soff[1] = R.two ? (first1 ? o0 : o1) : 0u;
        h.np[1] = R.two ? (first1 ? l0 : l1) / 2u : 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            h.OA[q] = R.OA[q];
            h.OB[q] = R.OB[q];
        }
        h.rkind = R.rkind;
        h.orig = orig;
        h.ws = ws;
        h.two = R.two;
        h.seg[0] = seg0;
        h.seg[1] = seg1;
        h.osize = orig;
        h.kind = 2;
        return h;
    }
    // stream table: lane s keeps stream s's data offset and length
    uint64_t off = 20ull + 4ull * msize;
    uint32_t my_off = 0, my_len = 0;
    for (uint32_t s = 0; s < ns; ++s) {  // uniform
        if (off + 4 > len) return h;
        const uint32_t l = off + 4 <= hcl ? ld_u32_bytes(hdr + off) : ld_u32_bytes(blob + off);
        off += 4;
        if (off + l > len) return h;
        if (lane == s) {
            my_off = (uint32_t)off;
            my_len = l;
        }
        off += l;
    }
    // mapping: lane b < ws holds mapping[b]; k = how many positions share it, rank = how many
    // before b, first = the lowest such position
    const uint32_t m = lane < ws ? hw(20 + 4 * lane) : 0xffffffffu;
    if (__any(lane < ws && m >= ns)) return h;  // (also negative values) → BAD_MAPPING via blob_check
    uint32_t k = 0, rank = 0, first = lane;
    for (uint32_t bb = 0; bb < ws; ++bb) {  // uniform
        const uint32_t mb = (uint32_t)__builtin_amdgcn_readlane((int)m, (int)bb);
        if (mb == m) {
            ++k;
            if (bb < lane) ++rank;
            first = first < bb ? first : bb;
        }
    }
    const uint64_t fum = __ballot(lane < ws && first == lane);  // first uses, in order
    if (__builtin_popcountll(fum) > 2) return h;
    const uint32_t f0 = (uint32_t)__builtin_ctzll(fum);
    const uint64_t fum1 = fum & (fum - 1);
    const bool two = fum1 != 0;
    const uint32_t f1 = two ? (uint32_t)__builtin_ctzll(fum1) : f0;
    const uint32_t WPG = 16 / ws;
    const uint32_t seg0 = WPG * (uint32_t)__builtin_amdgcn_readlane((int)k, (int)f0);
    const uint32_t seg1 = two ? WPG * (uint32_t)__builtin_amdgcn_readlane((int)k, (int)f1) : 0u;
    if ((seg0 & 3u) || (seg1 & 3u)) return h;
    const uint32_t m0 = (uint32_t)__builtin_amdgcn_readlane((int)m, (int)f0);
    const uint32_t m1 = (uint32_t)__builtin_amdgcn_readlane((int)m, (int)f1);
    h.soff[0] = (uint32_t)__builtin_amdgcn_readlane((int)my_off, (int)m0);
    h.np[0] = (uint32_t)__builtin_amdgcn_readlane((int)my_len, (int)m0) / 2u;
    h.soff[1] = two ? (uint32_t)__builtin_amdgcn_readlane((int)my_off, (int)m1) : 0u;
    h.np[1] = two ? (uint32_t)__builtin_amdgcn_readlane((int)my_len, (int)m1) / 2u : 0u;
    // recombine selectors: output byte i = word i / ws, position b = i % ws of stream
    // r = ref(mapping[b]) → S byte (r ? seg0 : 0) + (i / ws)·k_b + rank_b
    const uint32_t i = lane & 15u, b = i % ws;
    const uint32_t kb = (uint32_t)__shfl((int)k, (int)b), rb = (uint32_t)__shfl((int)rank, (int)b);
    const uint32_t fb = (uint32_t)__shfl((int)first, (int)b);
    const uint32_t sidx = (fb == f0 ? 0u : seg0) + (i / ws) * kb + rb;
    const uint32_t sh = 8u * (i & 3u);
    uint32_t A = (sidx < 8u ? sidx : 0x0cu) << sh, B = (sidx >= 8u ? sidx - 8u : 0x0cu) << sh;
    A |= dpp_mov_self<0xb1>(A);  // quad_perm [1,0,3,2]
    A |= dpp_mov_self<0x4e>(A);  // quad_perm [2,3,0,1]
    B |= dpp_mov_self<0xb1>(B);
    B |= dpp_mov_self<0x4e>(B);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        h.OA[q] = (uint32_t)__builtin_amdgcn_readlane((int)A, 4 * q);
        h.OB[q] = (uint32_t)__builtin_amdgcn_readlane((int)B, 4 * q);
    }
    h.orig = orig;
    h.ws = ws;
    h.two = two ? 1u : 0u;
    h.seg[0] = seg0;
    h.seg[1] = seg1;
    h.osize = orig;
    h.kind = 2;
    return h;
}

// One blob, one wave (LB: compacted output by look-back; else its slot).  PAIR: slot_off is a
// (begin, end) pair table (table_at, tdt_plan.h) — the instances of the scattered batches
// (tdt_decode_batch_v: in and out are null, in_off holds the blobs' addresses beside in_len).
template <int LB, int WR = kDecWR, bool PAIR = false>
__device__ __forceinline__ void decode_one(const DecodeArgs &a, uint8_t *smem, uint32_t msg) {
    using Lay = DecLayoutT<WR>;
    uint32_t *misc = reinterpret_cast<uint32_t *>(smem + Lay::OFF_MISC);
    uint8_t *hdrc = smem + Lay::OFF_BLOB;
    const int lane = lane_id();
    PSY_PROF_BEGIN();
    if (msg >= a.n_msgs) return;
    const uint64_t boff = a.in_off[msg];
    const uint64_t len = a.in_len ? a.in_len[msg] : a.in_off[msg + 1] - boff;
    // the slot is read beside the offsets (it depends on msg only): one dependent trip fewer
    uint64_t slot_b = 0, slot_e = 0;
    if constexpr (!LB) {
        slot_b = a.slot_off[table_at<PAIR>(msg, 0)];
        slot_e = a.slot_off[table_at<PAIR>(msg, 1)];
    }
    const uint8_t *blob = a.in + boff;
    const uint8_t *blim = blob + len;

    // ------------------------------------------------ blob cache: its first BLOBC bytes in LDS
    // (256 with the main list's windows; 2,112 with one-round windows: whole 1 KiB-message blobs)
    constexpr uint32_t BLOBC = (uint32_t)Lay::BLOBC;
    const uint32_t hcl = len < (uint64_t)BLOBC ? (uint32_t)len : BLOBC;
    if constexpr (BLOBC > 1024) {
        // 16 bytes per lane and load (dwordx4 at any dword-aligned start; a lane whose 16 bytes
        // cross the blob's end, or a blob that is not dword-aligned, takes bytes)
        constexpr int NQ = (int)((BLOBC / 16 + 63) / 64);
        uint4 q[NQ];
        const bool al4 = ((uintptr_t)blob & 3) == 0;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {  // (all loads issued before the first LDS write)
            const uint32_t o = ((uint32_t)lane + 64u * (uint32_t)j) * 16u;
            q[j] = make_uint4(0, 0, 0, 0);
            if (al4 && o + 16 <= hcl) {
                typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
                const u32x4_t v = gload<u32x4_t>(blob + o);
                q[j] = make_uint4(v.x, v.y, v.z, v.w);
            } else if (o < hcl) {
                uint32_t w[4] = {0, 0, 0, 0};
                for (uint32_t i = 0; i < 16 && o + i < hcl; ++i) w[i >> 2] |= (uint32_t)blob[o + i] << (8 * (i & 3));
                q[j] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const uint32_t d = (uint32_t)lane + 64u * (uint32_t)j;
            if (d < BLOBC / 16) reinterpret_cast<uint4 *>(hdrc)[d] = q[j];
        }
    } else {
        constexpr int ND = (int)((BLOBC / 4 + 63) / 64);  // dwords per lane
        uint32_t w[ND];
        const bool al4 = ((uintptr_t)blob & 3) == 0;
#pragma unroll
        for (int j = 0; j < ND; ++j) {  // (all loads issued before the first LDS write)
            const uint32_t o = ((uint32_t)lane + 64u * (uint32_t)j) * 4u;
            w[j] = 0;
            if (al4 && o + 4 <= hcl) {
                w[j] = *reinterpret_cast<const uint32_t *>(blob + o);
            } else if (o < hcl) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (o + i < hcl) w[j] |= (uint32_t)blob[o + i] << (8 * i);
            }
        }
#pragma unroll
        for (int j = 0; j < ND; ++j) {
            const uint32_t d = (uint32_t)lane + 64u * (uint32_t)j;
            if (d < BLOBC / 4) reinterpret_cast<uint32_t *>(hdrc)[d] = w[j];
        }
    }
    team_sync<1>();

    // ------------------------------------------------ fast path (wave-parallel header parse)
    const FastHdr H = parse_fast(blob, len, hdrc, hcl);
    if (H.kind != 0) {
        const uint64_t osize = H.osize;
        uint64_t ob;
        bool fits;
        if constexpr (LB) {
            ob = lookback_excl_wave(a.lookback, msg, osize, a.errflags);
            fits = ob + osize <= a.out_cap;
        } else {
            ob = slot_b;
            fits = osize <= slot_e - ob;
        }
        const uint32_t st = fits ? ST_OK : ST_CAPACITY;
        if (lane == 0) {
            if constexpr (LB) {
                a.out_off[msg] = ob;
                if (msg == a.n_msgs - 1) a.out_off[a.n_msgs] = ob + osize;
            } else {
                if (a.out_len) a.out_len[msg] = fits ? osize : 0;
            }
            if (a.status) a.status[msg] = (int32_t)st;
        }
        if (!fits) return;
        uint8_t *dst = a.out + ob;
        if (H.kind == 1) {
            team_copy_g2g<64>(dst, blob + 4, len - 4);
            return;
        }
        const uint64_t wbytes = (uint64_t)(H.orig / H.ws) * H.ws;
        // recombine :617 zero-initialises; bytes past the last whole word stay zero
        if (H.orig > wbytes) team_zero<64>(dst + wbytes, H.orig - wbytes);
        decode_fast<WR>(H, smem, blob, blim, dst, (uint32_t)((wbytes + 15) / 16), wbytes, 0, 0, nullptr, nullptr,
                        WR == 1 ? hdrc : nullptr, WR == 1 ? hcl : 0u);
        return;
    }
    auto rd32 = [&](uint64_t off) -> uint32_t {
        if (off + 4 <= hcl) {
            if ((off & 3) == 0) return *reinterpret_cast<const uint32_t *>(hdrc + off);
            return ld_u32_bytes(hdrc + off);
        }
        return ld_u32_bytes(blob + off);
    };

    // ------------------------------------------------ header parse (lane 0)
    if (lane == 0) {
        uint32_t uncp = 0, orig = 0, ws = 0, nref = 0;
        uint64_t osize = 0;
        const uint32_t st = blob_check(rd32, len, uncp, osize);
        if (st == ST_OK && !uncp) {
            orig = rd32(4);
            const uint32_t ns = rd32(8);
            ws = rd32(12);
            const uint64_t toff = 20 + 4ull * rd32(16);
            if ((int32_t)ws > 0 && orig / ws > 0) {
                // referenced streams in order of first use; stream table → data offsets
                uint32_t refc[kMaxRef];
                for (uint32_t b = 0; b < ws; ++b) {
                    const uint32_t m = rd32(20 + 4 * b);
                    uint32_t r = 0;
                    while (r < nref && refc[r] != m) ++r;
                    if (r == nref) refc[nref++] = m;
                }
                uint64_t off = toff;
                for (uint32_t s = 0; s < ns; ++s) {
                    const uint32_t sl = rd32(off);
                    off += 4;
                    for (uint32_t r = 0; r < nref; ++r)
                        if (refc[r] == s) {
                            misc[D_SOFF + r] = (uint32_t)off;
                            misc[D_NP + r] = sl / 2;
                        }
                    off += sl;
                }
                const uint32_t WPG = 16 / ws;
                uint32_t soffb = 0, hoff = 0, pb = 0;
                uint32_t fast = 1;
                for (uint32_t r = 0; r < nref; ++r) {
                    uint32_t k = 0;
                    for (uint32_t b = 0; b < ws; ++b) k += rd32(20 + 4 * b) == refc[r];
                    misc[D_K + r] = k;
                    misc[D_PIDX + r] = 0;
                    misc[D_POS + r] = 0;
                    misc[D_CV + r] = 0;
                    misc[D_SLEN + r] = 0xffffffffu;
                    misc[D_HOFF + r] = hoff;
                    misc[D_PB + r] = pb;
                    const uint32_t seg = WPG * k;  // S bytes of stream r per group
                    for (uint32_t u = 0; u < seg; ++u) misc[D_SB + soffb + u] = (r << 8) | u;
                    if (seg & 3u) fast = 0;
                    soffb += seg;
                    hoff += Lay::GWR * 64 * seg + 16;
                    pb += 64 * seg;
                }
                misc[D_FAST] = fast;
                // recombine selectors: output byte i = word i/ws, position b = i%ws of
                // stream r = ref(mapping[b]), rank t among the positions mapped to it →
                // S byte Soff_r + (i/ws)·k_r + t
                for (int q = 0; q < 4; ++q) {
                    uint32_t A = 0x0c0c0c0cu, B = 0x0c0c0c0cu;
                    for (int t4 = 0; t4 < 4; ++t4) {
                        const uint32_t i = 4 * q + t4, w = i / ws, b = i % ws;
                        const uint32_t m = rd32(20 + 4 * b);
                        uint32_t r = 0, so = 0;
                        while (refc[r] != m) so += WPG * misc[D_K + r++];
                        uint32_t rank = 0;
                        for (uint32_t bb = 0; bb < b; ++bb) rank += rd32(20 + 4 * bb) == m;
                        const uint32_t sidx = so + w * misc[D_K + r] + rank;
                        if (sidx < 8) A = (A & ~(0xffu << (8 * t4))) | (sidx << (8 * t4));
                        else B = (B & ~(0xffu << (8 * t4))) | ((sidx - 8) << (8 * t4));
                    }
                    misc[D_OA + q] = A;
                    misc[D_OB + q] = B;
                }
            }
        }
        misc[D_STATUS] = st;
        misc[D_UNCP] = uncp;
        misc[D_ORIG] = orig;
        misc[D_WS] = ws;
        misc[D_NREF] = nref;
        *reinterpret_cast<uint64_t *>(misc + D_BASE) = osize;
    }
    team_sync<1>();
    uint32_t st = __builtin_amdgcn_readfirstlane(misc[D_STATUS]);
    const uint64_t osize = *reinterpret_cast<const uint64_t *>(misc + D_BASE);
    // ------------------------------------------------ output placement
    uint64_t ob;
    bool fits;
    if constexpr (LB) {
        ob = lookback_excl_wave(a.lookback, msg, osize, a.errflags);
        fits = ob + osize <= a.out_cap;
    } else {
        ob = slot_b;
        fits = osize <= slot_e - ob;
    }
    if (st == ST_DEFER) {
        // a generic word size: placed here (the look-back has published its size), decoded —
        // status, length and bytes — by the follow-up launch over dlist (tdt_anyws.hip)
        if (lane == 0) {
            if constexpr (LB) {
                a.out_off[msg] = ob;
                if (msg == a.n_msgs - 1) a.out_off[a.n_msgs] = ob + osize;
            }
            if (a.dlist) {
                a.dlist[atomicAdd(a.dcount, 1u)] = msg;
            } else {  // (a launch without the follow-up: the one-message host call, which the host keeps such blobs from)
                if (!LB && a.out_len) a.out_len[msg] = 0;
                if (a.status) a.status[msg] = ST_UNSUPPORTED;
            }
        }
        return;
    }
    if (st == ST_OK && !fits) st = ST_CAPACITY;
    if (lane == 0) {
        if constexpr (LB) {
            a.out_off[msg] = ob;
            if (msg == a.n_msgs - 1) a.out_off[a.n_msgs] = ob + osize;
        } else {
            if (a.out_len) a.out_len[msg] = st == ST_OK ? osize : 0;
        }
        if (a.status) a.status[msg] = (int32_t)st;
    }
    if (st != ST_OK) return;
    PSY_PROF_MARK(8);
    uint8_t *dst = a.out + ob;
    if (misc[D_UNCP]) {
        team_copy_g2g<64>(dst, blob + 4, len - 4);
        return;
    }
    const uint32_t orig = __builtin_amdgcn_readfirstlane(misc[D_ORIG]);
    const uint32_t ws = __builtin_amdgcn_readfirstlane(misc[D_WS]);
    const uint64_t wc = orig / ws;
    const uint64_t wbytes = wc * ws;
    // recombine :617 zero-initialises; bytes past the last whole word stay zero
    if (orig > wbytes) team_zero<64>(dst + wbytes, orig - wbytes);
    if (wc == 0) return;
    const uint32_t WPG = 16 / ws;
    const uint32_t nref = __builtin_amdgcn_readfirstlane(misc[D_NREF]);
    const bool fast = misc[D_FAST] != 0;
    const uint32_t ngroups = (uint32_t)((wbytes + 15) / 16);
    uint32_t OA[4], OB[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        OA[q] = __builtin_amdgcn_readfirstlane(misc[D_OA + q]);
        OB[q] = __builtin_amdgcn_readfirstlane(misc[D_OB + q]);
    }
    constexpr uint32_t GWR = Lay::GWR;
    uint16_t *heads = reinterpret_cast<uint16_t *>(smem + Lay::OFF_HEADS);
    uint8_t *planes = smem + Lay::OFF_GPLANES;

    // (blobs parse_fast accepts never get here; the generic path serves every other shape)

    // ---------------------------------------------------------------- generic path
    // (more than two referenced streams, or stream segments that are not whole dwords)
    // fill lane → (stream, first plane position of the lane within the stream's round plane)
    uint32_t fr = 0, fu = 0, fk = 0;
    for (uint32_t r = 0; r < nref; ++r) {
        const uint32_t pb = misc[D_PB + r], seg = 64 * WPG * misc[D_K + r];
        if ((uint32_t)lane * 16u >= pb && (uint32_t)lane * 16u < pb + seg) {
            fr = r;
            fu = (uint32_t)lane * 16u - pb;
            fk = misc[D_K + r];
        }
    }
    const uint32_t f_hoff = misc[D_HOFF + fr], f_lb = misc[D_PB + fr] / 16u;
    // recombine fast path: S dword d = 4 bytes of one stream r at plane byte pb_r + l·4k_r + x
    uint32_t sd_pb[4] = {0, 0, 0, 0}, sd_mul[4] = {0, 0, 0, 0};
    if (fast) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t e = __builtin_amdgcn_readfirstlane(misc[D_SB + 4 * d]);
            const uint32_t r = e >> 8;
            sd_pb[d] = __builtin_amdgcn_readfirstlane(misc[D_PB + r]) + (e & 0xffu);
            sd_mul[d] = WPG * __builtin_amdgcn_readfirstlane(misc[D_K + r]);
        }
    }

    // One pair-round (8 pairs per lane from pair index pidx) of a stream; byte-exact at the
    // stream's end.
    auto load_pairs = [&](uint32_t pidx_, uint32_t np_, uint32_t soff_) __attribute__((always_inline)) -> uint4 {
        const uint32_t p0 = pidx_ + 8u * (uint32_t)lane;
        const uint32_t nv = p0 < np_ ? (np_ - p0 < 8u ? np_ - p0 : 8u) : 0u;
        return nv ? ld16_span(blob + soff_ + 2ull * p0, (int)(2 * nv), blim) : make_uint4(0, 0, 0, 0);
    };
    // The first pair-round of the next window of referenced streams 0 and 1 is loaded as soon
    // as this window's consumption is known, so its HBM latency overlaps this window's fill,
    // recombine and store (pf_idx = the pair index the registers hold, ~0 = none).
    uint4 pf0 = make_uint4(0, 0, 0, 0), pf1 = make_uint4(0, 0, 0, 0);
    uint32_t pf_idx0 = ~0u, pf_idx1 = ~0u;

    for (uint32_t gwin = 0; gwin < ngroups; gwin += 64 * GWR) {
        // ---- zero the heads of this window (16 B per lane per step)
        for (uint32_t i = (uint32_t)lane; i < (uint32_t)Lay::GHEADS / 16; i += 64)
            reinterpret_cast<uint4 *>(heads)[i] = make_uint4(0, 0, 0, 0);
        team_sync<1>();
        // ---- pairs → heads, per referenced stream
        for (uint32_t r = 0; r < nref; ++r) {
            const uint32_t k = __builtin_amdgcn_readfirstlane(misc[D_K + r]);
            const uint32_t np = __builtin_amdgcn_readfirstlane(misc[D_NP + r]);
            const uint32_t soff = __builtin_amdgcn_readfirstlane(misc[D_SOFF + r]);
            const uint32_t hoff = __builtin_amdgcn_readfirstlane(misc[D_HOFF + r]);
            uint32_t pidx = __builtin_amdgcn_readfirstlane(misc[D_PIDX + r]);
            uint32_t pos = __builtin_amdgcn_readfirstlane(misc[D_POS + r]);
            const uint32_t wstart = gwin * WPG * k;
            const uint32_t wlen = GWR * 64 * WPG * k;
            const uint32_t hb = Lay::OFF_HEADS + 2u * hoff;
            while (pidx < np && pos - wstart < wlen) {
                const uint32_t p0 = pidx + 8u * (uint32_t)lane;
                const uint32_t nv = p0 < np ? (np - p0 < 8u ? np - p0 : 8u) : 0u;
                uint4 pv;
                if (r == 0 && pidx == pf_idx0) pv = pf0;
                else if (r == 1 && pidx == pf_idx1) pv = pf1;
                else pv = load_pairs(pidx, np, soff);
                const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w};
                // lane total of counts (packed u16 sums of the even bytes)
                const uint32_t s2 = (pw[0] & 0x00ff00ffu) + (pw[1] & 0x00ff00ffu) + (pw[2] & 0x00ff00ffu) +
                                    (pw[3] & 0x00ff00ffu);
                const uint32_t tot = (s2 & 0xffffu) + (s2 >> 16);
                const uint32_t linc = wave_incl_scan<OpAdd>(tot);
                const uint32_t relb = pos - wstart + (linc - tot);  // start of this lane's first pair
                // zero counts (never made by the encoder) and the stream's last pair-round take
                // the predicated path
                const bool exact = (pidx + 512u > np) || __any((pw[0] & 0xffu) == 0 || (pw[0] & 0xff0000u) == 0 ||
                                                             (pw[1] & 0xffu) == 0 || (pw[1] & 0xff0000u) == 0 ||
                                                             (pw[2] & 0xffu) == 0 || (pw[2] & 0xff0000u) == 0 ||
                                                             (pw[3] & 0xffu) == 0 || (pw[3] & 0xff0000u) == 0);
                uint32_t run = relb;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t c = (pw[i >> 1] >> (16 * (i & 1))) & 0xffu;
                    const uint32_t v = (pw[i >> 1] >> (16 * (i & 1) + 8)) & 0xffu;
                    const uint32_t key = (((run & 15u) << 8) + 0x100u) | v;
                    const uint32_t slot = run < wlen ? run : wlen;  // wlen = the pad slot
                    if (!exact || (c != 0 && (uint32_t)i < nv))
                        *reinterpret_cast<uint16_t *>(smem + hb + 2u * slot) = (uint16_t)key;
                    run += c;
                }
                // consumed = the pairs starting inside the window: every lane whose first pair
                // starts inside is consumed up to the next lane; the last such lane is walked.
                const uint64_t bl = __ballot(nv > 0 && relb < wlen);
                if (bl == 0) break;  // (cannot happen: pos < window end)
                const int L = 63 - __builtin_clzll(bl);
                const uint32_t rbL = rdlane(relb, L), nvL = rdlane(nv, L);
                uint32_t cw[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) cw[q] = rdlane(pw[q], L);
                uint32_t cons = 0, rr = rbL;
                for (uint32_t i = 0; i < nvL; ++i) {
                    if (rr >= wlen) break;
                    rr += (cw[i >> 1] >> (16 * (i & 1))) & 0xffu;
                    ++cons;
                }
                pidx += 8u * (uint32_t)L + cons;
                pos = wstart + rr;
                if (cons < 8u || L < 63) break;  // the window ends inside this pair-round
            }
            if (pidx < np) {
                if (r == 0) {
                    pf0 = load_pairs(pidx, np, soff);
                    pf_idx0 = pidx;
                } else if (r == 1) {
                    pf1 = load_pairs(pidx, np, soff);
                    pf_idx1 = pidx;
                }
            }
            if (lane == 0) {
                misc[D_PIDX + r] = pidx;
                misc[D_POS + r] = pos;
                if (pidx >= np) misc[D_SLEN + r] = pos;  // stream exhausted: decoded length
            }
        }
        team_sync<1>();
        PSY_PROF_MARK(9);
        // ---- per round: fill the planes, recombine, store
        for (uint32_t rl = 0; rl < GWR; ++rl) {
            const uint32_t g0 = gwin + rl * 64;
            if (g0 >= ngroups) break;
            // lane's 16 plane positions: heads[hoff + rl·64·WPG·k + fu ..)
            const uint32_t hidx = f_hoff + rl * 64u * WPG * fk + fu;
            const uint4 h0 = *reinterpret_cast<const uint4 *>(heads + hidx);
            const uint4 h1 = *reinterpret_cast<const uint4 *>(heads + hidx + 8);
            uint32_t x[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
            // last head key of the lane (tags order the keys by position)
            uint32_t m = pk_max_u16(pk_max_u16(pk_max_u16(x[0], x[1]), pk_max_u16(x[2], x[3])),
                                    pk_max_u16(pk_max_u16(x[4], x[5]), pk_max_u16(x[6], x[7])));
            m = pk_max_self_lo(m) >> 16;
            const uint32_t lk = m ? (((uint32_t)lane + 1u) << 8) | (m & 0xffu) : 0u;
            const uint32_t ex = wave_shr1(wave_incl_scan<OpMax>(lk), 0u);
            uint32_t seed;
            if (ex && (ex >> 8) - 1u >= f_lb) seed = ex & 0xffu;  // a head earlier in this stream's plane
            else seed = misc[D_CV + fr];                        // carried from the previous round
            x[0] = pk_max_u16(x[0], seed);
            // in-lane prefix max: within each dword, then across dwords
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = pk_max_self_lo(x[q]);
#pragma unroll
            for (int q = 1; q < 8; ++q) x[q] = pk_max_bcast_hi(x[q], x[q - 1]);
            uint4 bytes = make_uint4(perm(x[1], x[0], 0x06040200u), perm(x[3], x[2], 0x06040200u),
                                     perm(x[5], x[4], 0x06040200u), perm(x[7], x[6], 0x06040200u));
            // a stream that ran out of pairs leaves zeros (recombine :626-631)
            {
                const uint32_t slen = misc[D_SLEN + fr];
                const uint32_t p0 = g0 * WPG * fk + fu;  // absolute position of the lane's first byte
                if (slen != 0xffffffffu && slen < p0 + 16u) {
                    uint32_t w[4] = {bytes.x, bytes.y, bytes.z, bytes.w};
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        if (p0 + (uint32_t)i >= slen) w[i >> 2] &= ~(0xffu << (8 * (i & 3)));
                    bytes = make_uint4(w[0], w[1], w[2], w[3]);
                }
            }
            *reinterpret_cast<uint4 *>(planes + 16u * (uint32_t)lane) = bytes;
            // carries: each stream's value at the end of its round plane
            team_sync<1>();
            for (uint32_t r = 0; r < nref; ++r) {
                const uint32_t pe = misc[D_PB + r] + 64u * WPG * misc[D_K + r] - 1u;
                if (lane == 0) misc[D_CV + r] = planes[pe];
            }
            // recombine: S = this group's bytes of every stream, then v_perm into word order
            uint32_t S[4];
            if (fast) {
#pragma unroll
                for (int d = 0; d < 4; ++d)
                    S[d] = *reinterpret_cast<const uint32_t *>(planes + sd_pb[d] + (uint32_t)lane * sd_mul[d]);
            } else {
                S[0] = S[1] = S[2] = S[3] = 0;
                for (int i = 0; i < 16; ++i) {
                    const uint32_t e = misc[D_SB + i];
                    const uint32_t r = e >> 8;
                    if (r >= nref) break;
                    const uint32_t seg = WPG * misc[D_K + r];
                    S[i >> 2] |= (uint32_t)planes[misc[D_PB + r] + (uint32_t)lane * seg + (e & 0xffu)] << (8 * (i & 3));
                }
            }
            const uint4 o = make_uint4(perm(S[1], S[0], OA[0]) | perm(S[3], S[2], OB[0]),
                                       perm(S[1], S[0], OA[1]) | perm(S[3], S[2], OB[1]),
                                       perm(S[1], S[0], OA[2]) | perm(S[3], S[2], OB[2]),
                                       perm(S[1], S[0], OA[3]) | perm(S[3], S[2], OB[3]));
            const uint32_t g = g0 + (uint32_t)lane;
            if (g < ngroups) {
                const uint64_t vb64 = wbytes - 16ull * g;
                st16_any(dst + 16ull * g, o, vb64 >= 16 ? 16 : (int)vb64);
            }
            // the planes' bytes are heads slots again: empty for the windows that follow (the
            // gather's reads precede these writes in the wave's LDS order)
            *reinterpret_cast<uint4 *>(planes + 16u * lane) = make_uint4(0, 0, 0, 0);
        }
        PSY_PROF_MARK(10);
    }
}

// ------------------------------------------------------------------ large blobs (slotted)
// A blob whose decoded size exceeds large_min is decoded by many waves: the
// prep pass parses its header (wave-parallel) and places it; the block pass sums the counts of
// every 512-pair block of its referenced streams; the scan turns them into block start
// positions and records, for every 32 KiB output tile, the block holding the tile's first
// position - 1 (the carry); the tile pass decodes each tile with the fast path from there.
// Blobs the fast path does not take are decoded whole, by one wave, in the prep pass.
struct DMeta {
    FastHdr H;
    uint32_t msg, nbs, blk0, ntiles, tile0;
    uint32_t nb[2];    // 512-pair blocks per referenced stream (prep)
    uint32_t slen[2];  // decoded stream lengths (scan)
    uint32_t tiled;    // 1: the tile pass decodes it (kind 1 copy / kind 2 fast path)
    uint64_t ob;       // output offset (its slot)
};

struct DPlanArgs {
    const uint8_t *in;
    const uint64_t *in_off;
    const uint64_t *in_len;
    uint32_t n_msgs;
    // the counter block (DecCount, tdt_plan.h)
    unsigned long long *cnt;
    uint32_t *list;
    uint32_t *slist;          // blobs decoding to <= small_max bytes (one-round windows: less LDS per wave)
    uint64_t small_max;
    uint32_t *blist;          // one-wave blobs decoding to > big_min bytes (dispatched first)
    uint64_t big_min;
    uint32_t *clist;          // UNCP blobs (passthrough copies, several per wave)
    DMeta *dmeta;
    uint32_t *bent, *tent;
    uint32_t lmax, bcap, tcap;  // (0, 0, 0: no tiled path)
    uint64_t large_min;
    uint32_t small_on;  // 0: small blobs join the one-wave list
    uint32_t copy_on;   // 0: UNCP blobs join the one-wave lists
};

#ifndef PSY_DEC_INST_TU
// PAIR: a scattered batch, whose bytes are counter DC_BYTES (the table kernel's sum)
template <bool PAIR = false>
__global__ __launch_bounds__(1024) void tdt_decode_plan_kernel(DPlanArgs p) {
    __shared__ uint64_t lds[6 * (4 * 16 + 1)];
    // one wave per blob keeps the chip busy while a blob is at most ~1/4096 of the batch's
    // bytes; only larger blobs (and only above large_min) are worth the tiled passes
    uint64_t thr = p.large_min;
    if (p.n_msgs) {
        const uint64_t last = p.in_len ? p.in_off[p.n_msgs - 1] + p.in_len[p.n_msgs - 1] : p.in_off[p.n_msgs];
        const uint64_t share = (PAIR ? p.cnt[DC_BYTES] : last - p.in_off[0]) / 4096;
        thr = share > thr ? share : thr;
    }
    // the claims' values (A: large blobs, tiles, block slots; B: the lists) and their starts
    uint64_t A[3][4], SA[3][4], B[6][4], SB[6][4];
    auto &isl = A[0], &nt = A[1], &nb = A[2];
    auto &j = SA[0], &t0 = SA[1], &b0 = SA[2];
    auto &one = B[0], &sm = B[1], &sc = B[2], &bg = B[3], &ucc = B[4], &cpo = B[5];
    auto &pos = SB[0], &spos = SB[1], &bpos = SB[3], &cpp = SB[5];
    uint64_t osz_k[4], unc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = (blockIdx.x * 4 + k) * 1024 + threadIdx.x;
        isl[k] = nt[k] = nb[k] = 0;
        osz_k[k] = 0;
        if (i < p.n_msgs) {
            const uint64_t boff = p.in_off[i];
            const uint64_t len = p.in_len ? p.in_len[i] : p.in_off[i + 1] - boff;
            uint64_t osz = 0, nbs = 0;
            if (len >= 20) {
                const uint8_t *bp = p.in + boff;
                const bool al8 = ((uintptr_t)bp & 7) == 0;
                uint32_t magic, w1;
                if (al8) {  // (one 8-byte load instead of eight byte loads)
                    const uint2 v = *reinterpret_cast<const uint2 *>(bp);
                    magic = v.x;
                    w1 = v.y;
                } else {
                    magic = ld_u32_bytes(bp);
                    w1 = ld_u32_bytes(bp + 4);
                }
                if (magic == kMagicTDT) {
                    osz = w1;
                    nbs = len / 1024 + 3;  // >= the 512-pair blocks of <= 2 referenced streams
                } else if (magic == kMagicUNCP) {
                    osz = len - 4;
                    unc[k] = 1;
                }
            } else if (len >= 4 && ld_u32_bytes(p.in + boff) == kMagicUNCP) {
                osz = len - 4;
                unc[k] = 1;
            }
            osz_k[k] = osz;
            if (osz > thr) {
                isl[k] = 1;
                nt[k] = (osz + 16ull * kDecTileGroups - 1) / (16ull * kDecTileGroups);
                nb[k] = nbs;
            }
        }
    }
    {
        constexpr int ia[3] = {DC_LARGE, DC_TILES, DC_BLOCKS};
        wg_claim_n<3, 4>(A, SA, p.cnt, ia, lds);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = (blockIdx.x * 4 + k) * 1024 + threadIdx.x;
        bool large = false;
        if (isl[k]) {
            large = j[k] < p.lmax && t0[k] + nt[k] <= p.tcap && b0[k] + nb[k] <= p.bcap;
            if (large) {
                DMeta m{};
                m.msg = i;
                m.nbs = (uint32_t)nb[k];
                m.blk0 = (uint32_t)b0[k];
                m.ntiles = (uint32_t)nt[k];
                m.tile0 = (uint32_t)t0[k];
                p.dmeta[j[k]] = m;
            } else {  // over a budget: the one-wave path; the ranges it claimed stay empty
                if (j[k] < p.lmax) p.dmeta[j[k]].msg = kNone;
                for (uint64_t t = t0[k]; t < t0[k] + nt[k] && t < p.tcap; ++t) p.tent[t] = kNone;
                for (uint64_t b = b0[k]; b < b0[k] + nb[k] && b < p.bcap; ++b) p.bent[b] = kNone;
            }
        }
        const bool uncp = i < p.n_msgs && !large && !isl[k] && unc[k];
        const bool copy = uncp && p.copy_on;
        ucc[k] = uncp ? 1u : 0u;
        cpo[k] = copy ? 1u : 0u;
        const bool any = i < p.n_msgs && !large && !copy;
        const bool small = any && !isl[k] && p.small_max && osz_k[k] <= p.small_max;
        sc[k] = small ? 1u : 0u;
        sm[k] = small && p.small_on ? 1u : 0u;
        const bool big = any && !sm[k] && p.blist && osz_k[k] > p.big_min;
        bg[k] = big ? 1u : 0u;
        one[k] = (any && !sm[k] && !big) ? 1u : 0u;
    }
    {
        constexpr int ib[6] = {DC_MAIN, DC_SMALL, DC_SMALL_ALL, DC_BIG, DC_UNCP_ALL, DC_UNCP};
        wg_claim_n<6, 4>(B, SB, p.cnt, ib, lds);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (one[k]) p.list[pos[k]] = (blockIdx.x * 4 + k) * 1024 + threadIdx.x;
        if (sm[k]) p.slist[spos[k]] = (blockIdx.x * 4 + k) * 1024 + threadIdx.x;
        if (bg[k]) p.blist[bpos[k]] = (blockIdx.x * 4 + k) * 1024 + threadIdx.x;
        if (cpo[k]) p.clist[cpp[k]] = (blockIdx.x * 4 + k) * 1024 + threadIdx.x;
    }
}

// Prep: one workgroup per large blob; wave 0 parses and places it, then every thread writes
// its block-slot and tile entries (kNone where no pass has work).
template <bool PAIR = false>
__global__ __launch_bounds__(256) void tdt_decode_lprep_kernel(DecodeArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[DecLayout::BYTES];
    __shared__ uint32_t s_tiled, s_fast;
    const uint32_t nl = __builtin_amdgcn_readfirstlane(umin(a.pcnt[lo32(DC_LARGE)], a.lcap));
    for (uint32_t j = blockIdx.x; j < nl; j += gridDim.x) {  // grid-stride over the large blobs
    if (j != blockIdx.x) __syncthreads();
    DMeta *m = a.dmeta + j;
    const uint32_t msg = m->msg;
    if (msg == kNone) continue;  // over a budget (the plan emptied its ranges)
    if (threadIdx.x < 64) {
        const int lane = lane_id();
        const uint64_t boff = a.in_off[msg];
        const uint64_t len = a.in_len ? a.in_len[msg] : a.in_off[msg + 1] - boff;
        const uint8_t *blob = a.in + boff;
        uint8_t *hdrc = smem + DecLayout::OFF_HDR;
        {
            const uint64_t hc = len < (uint64_t)kHdrCache ? len : (uint64_t)kHdrCache;
            const uint32_t o = (uint32_t)lane * 4u;
            uint32_t w = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (o + q < hc) w |= (uint32_t)blob[o + q] << (8 * q);
            reinterpret_cast<uint32_t *>(hdrc)[lane] = w;
        }
        team_sync<1>();
        const uint32_t hcl = len < (uint64_t)kHdrCache ? (uint32_t)len : (uint32_t)kHdrCache;
        const FastHdr H = parse_fast(blob, len, hdrc, hcl);
        uint32_t tiled = 0, fast = 0;
        if (H.kind != 0) {
            const uint64_t ob = a.slot_off[table_at<PAIR>(msg, 0)];
            const bool fits = H.osize <= a.slot_off[table_at<PAIR>(msg, 1)] - ob;
            if (lane == 0) {
                if (a.out_len) a.out_len[msg] = fits ? H.osize : 0;
                if (a.status) a.status[msg] = fits ? ST_OK : ST_CAPACITY;
            }
            if (fits) {
                tiled = 1;
                fast = H.kind == 2 ? 1u : 0u;
                if (H.kind == 2) {
                    const uint64_t wbytes = (uint64_t)(H.orig / H.ws) * H.ws;
                    if (H.orig > wbytes) team_zero<64>(a.out + ob + wbytes, H.orig - wbytes);
                }
                if (lane == 0) {
                    m->H = H;
                    m->ob = ob;
                    m->nb[0] = (H.np[0] + 511u) / 512u;
                    m->nb[1] = H.two ? (H.np[1] + 511u) / 512u : 0u;
                }
            }
        } else {
            decode_one<0, kDecWR, PAIR>(a, smem, msg);  // any other shape (or an error): one wave, whole
        }
        if (lane == 0) {
            m->tiled = tiled;
            s_tiled = tiled;
            s_fast = fast;
        }
    }
    __syncthreads();
    const uint32_t tv = s_tiled ? j : kNone, bv = s_fast ? j : kNone;
    for (uint32_t i = threadIdx.x; i < m->ntiles; i += 256) const_cast<uint32_t *>(a.tent)[m->tile0 + i] = tv;
    for (uint32_t i = threadIdx.x; i < m->nbs; i += 256) const_cast<uint32_t *>(a.bent)[m->blk0 + i] = bv;
    }
}

// Block pass: one wave per 512-pair block (8 pairs per lane): the block's count sum.
__global__ __launch_bounds__(256) void tdt_decode_lblock_kernel(DecodeArgs a) {
    const uint32_t nslots = __builtin_amdgcn_readfirstlane(umin(a.pcnt[lo32(DC_BLOCKS)], a.bcap));
    for (uint32_t slot = blockIdx.x * 4u + (threadIdx.x >> 6); slot < nslots; slot += gridDim.x * 4u) {
    const uint32_t j = a.bent[slot];
    if (j == kNone) continue;
    const DMeta *m = a.dmeta + j;
    const uint32_t idx = slot - m->blk0, nb0 = m->nb[0];
    const uint32_t r = idx < nb0 ? 0u : 1u;
    const uint32_t b = r ? idx - nb0 : idx;
    if (r == 1 && b >= m->nb[1]) continue;
    const uint32_t msg = m->msg;
    const uint64_t boff = a.in_off[msg];
    const uint64_t len = a.in_len ? a.in_len[msg] : a.in_off[msg + 1] - boff;
    const uint8_t *blob = a.in + boff;
    const uint32_t np = m->H.np[r], soff = m->H.soff[r];
    const uint32_t p0 = 512u * b + 8u * (uint32_t)lane_id();
    const uint32_t nv = p0 < np ? (np - p0 < 8u ? np - p0 : 8u) : 0u;
    const uint4 pv = nv ? ld16_span(blob + soff + 2ull * p0, (int)(2 * nv), blob + len) : make_uint4(0, 0, 0, 0);
    const uint32_t s2 = (pv.x & 0x00ff00ffu) + (pv.y & 0x00ff00ffu) + (pv.z & 0x00ff00ffu) + (pv.w & 0x00ff00ffu);
    const uint32_t tot = wave_reduce<OpAdd>((s2 & 0xffffu) + (s2 >> 16));
    if (lane_id() == 0) a.bsum[m->blk0 + idx] = tot;
    }
}

// Scan: one wave per large blob and referenced stream: block sums → block start positions
// (in place), the stream's decoded length, and each tile's carry block.
__global__ __launch_bounds__(64) void tdt_decode_lscan_kernel(DecodeArgs a) {
    const uint32_t nl = __builtin_amdgcn_readfirstlane(umin(a.pcnt[lo32(DC_LARGE)], a.lcap));
    const uint32_t r = blockIdx.y;
    for (uint32_t j = blockIdx.x; j < nl; j += gridDim.x) {  // grid-stride over the large blobs
    DMeta *m = a.dmeta + j;
    if (m->msg == kNone || !m->tiled || m->H.kind != 2 || (r == 1 && !m->H.two)) continue;
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t n = m->nb[r], base = m->blk0 + (r ? m->nb[0] : 0u);
    const uint64_t TS = (uint64_t)kDecTileGroups * m->H.seg[r];  // stream positions per tile
    const uint32_t nt = m->ntiles;
    uint32_t *tb = a.tblk + 2ull * m->tile0 + r;
    uint64_t run = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += 64) {
        const uint32_t b = c0 + lane;
        const uint32_t v = b < n ? a.bsum[base + b] : 0u;
        const uint32_t incl = wave_incl_scan<OpAdd>(v);
        const uint64_t st = run + incl - v;
        if (b < n) {
            a.bsum[base + b] = (uint32_t)st;
            // tiles t >= 1 whose position t·TS - 1 lies in [st, st + v)
            for (uint64_t t = (st + TS) / TS; t < nt && t * TS <= st + v; ++t) tb[2 * t] = b;
        }
        run += rdlane(incl, 63);
    }
    if (lane == 0) m->slen[r] = (uint32_t)run;
    }
}
#endif  // PSY_DEC_INST_TU

// Tile pass: one wave per 32 KiB output tile (main launch: tiles [list_base, list_base + grid);
// overflow launch, PS = 1: the tiles past it, grid-stride).
__device__ __forceinline__ void decode_ltile(const DecodeArgs &a, uint8_t *smem, uint32_t slot) {
    const uint32_t j = a.tent[slot];
    if (j == kNone) return;
    const DMeta *m = a.dmeta + j;
    const uint32_t t = slot - m->tile0;
    const uint32_t msg = m->msg;
    const uint64_t boff = a.in_off[msg];
    const uint64_t len = a.in_len ? a.in_len[msg] : a.in_off[msg + 1] - boff;
    const uint8_t *blob = a.in + boff;
    uint8_t *dst = a.out + m->ob;
    const FastHdr H = m->H;
    if (H.kind == 1) {
        const uint64_t o0 = 16ull * kDecTileGroups * t;
        if (o0 < H.osize) {
            const uint64_t nb = H.osize - o0 < 16ull * kDecTileGroups ? H.osize - o0 : 16ull * kDecTileGroups;
            team_copy_g2g<64>(dst + o0, blob + 4 + o0, nb);
        }
        return;
    }
    const uint64_t wbytes = (uint64_t)(H.orig / H.ws) * H.ws;
    const uint32_t ngroups = (uint32_t)((wbytes + 15) / 16);
    const uint32_t g_lo = t * kDecTileGroups;
    if (g_lo >= ngroups) return;
    const uint32_t g_hi = ngroups - g_lo < kDecTileGroups ? ngroups : g_lo + kDecTileGroups;
    uint32_t b0[2] = {0u, 0u}, s0[2] = {0u, 0u};
    if (g_lo > 0) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !H.two) break;
            const uint32_t P = g_lo * H.seg[r];
            if (P - 1u >= m->slen[r]) {
                b0[r] = kNone;
                s0[r] = m->slen[r];
            } else {
                b0[r] = a.tblk[2ull * slot + r];
                s0[r] = a.bsum[m->blk0 + (r ? m->nb[0] : 0u) + b0[r]];
            }
        }
    }
    decode_fast(H, smem, blob, blob + len, dst, ngroups, wbytes, g_lo, g_hi, b0, s0);
}

template <int PS = 0>
__global__ __launch_bounds__(64) void tdt_decode_ltile_kernel(DecodeArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[DecLayout::BYTES];
    const uint32_t nt = __builtin_amdgcn_readfirstlane(umin(a.pcnt[lo32(DC_TILES)], a.tcap));
    const uint32_t i0 = a.list_base + blockIdx.x;
    if constexpr (PS) {
        for (uint32_t i = i0; i < nt; i += gridDim.x) {
            if (i != i0) team_sync<1>();
            decode_ltile(a, smem, i);
        }
    } else {
        if (i0 < nt) decode_ltile(a, smem, i0);
    }
}

// One blob, one workgroup of NW waves (the one-message host call, tdt_decode_host with a single
// blob, protocol_demo.cpp:164-189's per-message decode): the large-blob passes — block sums
// (lblock), their scan (lscan), output tiles through decode_fast (ltile) — in ONE launch with
// the scan in LDS, so a 64 KiB blob is NW waves' tiles, not one wave walking 64 rounds with a
// dependent block load per window.  Every wave parses the header itself (no broadcast); any
// shape decode_fast does not take (UNCP, generic, errors) goes to wave 0's decode_one.
constexpr int kOneWaves = 16;
constexpr uint32_t kOneBlocks = 640;  // block sums in LDS (the host caps the blob at ~514 blocks)
template <int NW>
__global__ __launch_bounds__(64 * NW) void tdt_decode_one_kernel(DecodeArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[NW][DecLayout::BYTES];
    __shared__ uint32_t s_bs[kOneBlocks];  // block sums, then (scan) block start positions
    __shared__ uint32_t s_slen[2];
    const uint32_t w = threadIdx.x >> 6, lane = (uint32_t)lane_id();
    const uint64_t boff = a.in_off[0];
    const uint64_t len = a.in_off[1] - boff;
    const uint8_t *blob = a.in + boff;
    uint8_t *hdrc = smem[w] + DecLayout::OFF_HDR;
    {
        const uint64_t hc = len < (uint64_t)kHdrCache ? len : (uint64_t)kHdrCache;
        const uint32_t o = lane * 4u;
        uint32_t v = 0;
        if (((uintptr_t)blob & 3) == 0 && o + 4 <= hc) {
            v = *reinterpret_cast<const uint32_t *>(blob + o);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (o + i < hc) v |= (uint32_t)blob[o + i] << (8 * i);
        }
        reinterpret_cast<uint32_t *>(hdrc)[lane] = v;
    }
    team_sync<1>();
    const uint32_t hcl = len < (uint64_t)kHdrCache ? (uint32_t)len : (uint32_t)kHdrCache;
    const FastHdr H = parse_fast(blob, len, hdrc, hcl);
    const uint32_t nb0 = (H.np[0] + 511u) / 512u, nb1 = H.two ? (H.np[1] + 511u) / 512u : 0u;
    // (H is the same in every wave: these branches are workgroup-uniform)
    if (H.kind != 2 || nb0 + nb1 > kOneBlocks) {
        if (w == 0) {
            team_sync<1>();  // (the header cache is decode_one's to refill)
            decode_one<0>(a, smem[0], 0);
        }
        return;
    }
    const uint64_t ob = a.slot_off[0];
    const bool fits = H.osize <= a.slot_off[1] - ob;
    if (w == 0 && lane == 0) {
        if (a.out_len) a.out_len[0] = fits ? H.osize : 0;
        if (a.status) a.status[0] = fits ? ST_OK : ST_CAPACITY;
    }
    if (!fits) return;
    uint8_t *dst = a.out + ob;
    const uint64_t wbytes = (uint64_t)(H.orig / H.ws) * H.ws;
    if (w == 0 && H.orig > wbytes) team_zero<64>(dst + wbytes, H.orig - wbytes);
    // ---- block sums (lblock): wave w takes blocks w, w + NW, ...
    for (uint32_t b = w; b < nb0 + nb1; b += NW) {
        const uint32_t r = b < nb0 ? 0u : 1u;
        const uint32_t np = H.np[r], soff = H.soff[r];
        const uint32_t p0 = 512u * (r ? b - nb0 : b) + 8u * lane;
        const uint32_t nv = p0 < np ? (np - p0 < 8u ? np - p0 : 8u) : 0u;
        const uint4 pv = nv ? ld16_span(blob + soff + 2ull * p0, (int)(2 * nv), blob + len) : make_uint4(0, 0, 0, 0);
        const uint32_t s2 = (pv.x & 0x00ff00ffu) + (pv.y & 0x00ff00ffu) + (pv.z & 0x00ff00ffu) + (pv.w & 0x00ff00ffu);
        const uint32_t tot = wave_reduce<OpAdd>((s2 & 0xffffu) + (s2 >> 16));
        if (lane == 0) s_bs[b] = tot;
    }
    __syncthreads();
    // ---- scan (lscan): wave r, stream r's block sums → start positions, in place
    if (w < (H.two ? 2u : 1u)) {
        const uint32_t n = w ? nb1 : nb0, base = w ? nb0 : 0u;
        uint32_t run = 0;
        for (uint32_t c0 = 0; c0 < n; c0 += 64) {
            const uint32_t b = c0 + lane;
            const uint32_t v = b < n ? s_bs[base + b] : 0u;
            const uint32_t incl = wave_incl_scan<OpAdd>(v);
            if (b < n) s_bs[base + b] = run + incl - v;
            run += rdlane(incl, 63);
        }
        if (lane == 0) s_slen[w] = run;
    }
    __syncthreads();
    // ---- tiles (ltile): wave w decodes tiles w, w + NW, ... of TG groups (whole rounds)
    const uint32_t ngroups = (uint32_t)((wbytes + 15) / 16);
    const uint32_t TG = ((ngroups + NW - 1) / NW + 63u) & ~63u;
    const uint32_t nt = (ngroups + TG - 1) / TG;
    for (uint32_t t = w; t < nt; t += NW) {
        if (t != w) team_sync<1>();
        const uint32_t g_lo = t * TG, g_hi = ngroups - g_lo < TG ? ngroups : g_lo + TG;
        uint32_t b0[2] = {0u, 0u}, s0[2] = {0u, 0u};
        if (g_lo > 0) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (r == 1 && !H.two) break;
                const uint32_t P1 = g_lo * H.seg[r] - 1u, slen = s_slen[r];
                const uint32_t n = r ? nb1 : nb0, base = r ? nb0 : 0u;
                if (P1 >= slen) {  // the stream ended before this tile: zeros
                    b0[r] = kNone;
                    s0[r] = slen;
                    continue;
                }
                // the block holding position P1: start <= P1 < the next block's start
                for (uint32_t c0 = 0; c0 < n; c0 += 64) {
                    const uint32_t b = c0 + lane;
                    const uint32_t st = b < n ? s_bs[base + b] : ~0u;
                    const uint32_t en = b + 1 < n ? s_bs[base + b + 1] : slen;
                    const uint64_t hit = __ballot(b < n && st <= P1 && P1 < en);
                    if (hit) {
                        const uint32_t bl = (uint32_t)__builtin_ctzll(hit);
                        b0[r] = c0 + bl;
                        s0[r] = rdlane(st, (int)bl);
                        break;
                    }
                }
            }
        }
        decode_fast(H, smem[w], blob, blob + len, dst, ngroups, wbytes, g_lo, g_hi, b0, s0);
    }
}

// Blob ids: the look-back needs them in dispatch order (atomic ticket); slotted batches take
// them from the plan's list (or, without one, the workgroup id).
// List entries are bounded by the plan's device-side count (main launch: one blob per wave over
// [list_base, list_base + grid); overflow launch, PS = 1: the entries past it, grid-stride).
template <int LB, int WR = kDecWR, int PS = 0, bool PAIR = false>
__global__ __launch_bounds__(64, LB ? 6 : 8) void tdt_decode_kernel(DecodeArgs a) {
    static_assert(!PAIR || !LB, "scattered batches are slotted");
    __shared__ __attribute__((aligned(16))) uint8_t smem[DecLayoutT<WR>::BYTES];
    if constexpr (LB) {
        uint32_t t = 0;
        if (lane_id() == 0) t = atomicAdd(a.ticket, 1u);
        decode_one<LB, WR, PAIR>(a, smem, __builtin_amdgcn_readfirstlane(t));
    } else {
        // (slotted launches always pass the plan's list; the main list's big blobs come first)
        const uint32_t nb = a.blist ? __builtin_amdgcn_readfirstlane(*a.blist_count) : 0u;
        const uint32_t cnt = nb + __builtin_amdgcn_readfirstlane(*a.list_count);
        const uint32_t i0 = a.list_base + blockIdx.x;
        auto entry = [&](uint32_t i) -> uint32_t { return i < nb ? a.blist[i] : a.list[i - nb]; };
        if constexpr (PS) {
            for (uint32_t i = i0; i < cnt; i += gridDim.x) {
                if (i != i0) team_sync<1>();
                decode_one<LB, WR, PAIR>(a, smem, entry(i));
            }
        } else {
            // the list entries are read beside the counts, not after them (i0 < n_msgs = every
            // list's capacity; a stale entry past the count is never used): one dependent trip
            const uint32_t ic = i0 < a.n_msgs ? i0 : a.n_msgs - 1u;
            const uint32_t eb = a.blist ? a.blist[ic] : 0u, el = a.list[ic];
            if (i0 >= cnt) return;
            decode_one<LB, WR, PAIR>(a, smem, i0 < nb ? eb : (nb == 0u ? el : a.list[i0 - nb]));
        }
    }
}

}  // namespace psy
