// tdt_red_tiles.h — the arithmetic of the tiled decode-reduce (tdt_dec_reduce_tiled.h) that is not a
// kernel: tile and block counts, which tiles a 512-pair block's range of a stream covers, and where a
// tile's decode of a stream starts.
//
// A destination of `osize` bytes is gc = ceil(osize / 16) groups, cut into tiles of kRedTileGroups
// groups (a whole number of the decoder's windows, so no window straddles two tiles).  Stream r of a
// peer holds seg_r bytes of every group: tile t >= 1 starts at stream position P = t * TS with
// TS = kRedTileGroups * seg_r, and its decode needs the 512-pair block that holds position P - 1 (the
// carry: the value of the run that reaches into the tile) together with the start position of that
// block's first pair.  The scan walks a stream's block sums once: block b with exclusive start `st`
// and count sum `v` covers positions [st, st + v) and is the carry block of every tile t with
// st <= t * TS - 1 < st + v.  A stream whose counts end at or before P - 1 has no such block: the
// tile's share of it is zeros, which decode_fast takes as block kNone with the stream's length.
//
// Plain host / device C++: tests/cpp/test_red_tiles.cpp drives it against a walk over pair lists.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PSY_RT_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define PSY_RT_HD inline
#endif

namespace psy {

constexpr uint32_t kRedWinRounds = 3;                        // the decoder's rounds per window (kDecWR)
constexpr uint32_t kRedTileWin = 11;                         // windows per tile
constexpr uint32_t kRedTileGroups = kRedTileWin * 64u * kRedWinRounds;  // 2,112 groups
constexpr uint32_t kRedTileBytes = 16u * kRedTileGroups;     // 33,792 bytes (TDT_REDUCE_TILE_BYTES)
constexpr uint32_t kRedBlockPairs = 512;                     // the block decode_fast indexes
constexpr uint32_t kRedNoBlock = 0xffffffffu;                // kNone

// tiles of a destination of osize bytes (osize < 2^35)
PSY_RT_HD uint32_t red_ntiles(uint64_t osize) { return (uint32_t)((osize + kRedTileBytes - 1u) / kRedTileBytes); }
// 512-pair blocks of a stream of np pairs
PSY_RT_HD uint32_t red_nblocks(uint32_t np) { return (np + kRedBlockPairs - 1u) / kRedBlockPairs; }
// the block slots a blob of len bytes can need: at most two referenced streams of len / 2 pairs together
PSY_RT_HD uint64_t red_block_claim(uint64_t len) { return len / 1024u + 3u; }

// the groups [g_lo, g_hi) of tile t of a destination of gc groups (g_lo == g_hi: past its end)
struct RedGroups {
    uint32_t g_lo, g_hi;
};
PSY_RT_HD RedGroups red_tile_groups(uint32_t t, uint32_t gc) {
    const uint64_t a = (uint64_t)t * kRedTileGroups, b = a + kRedTileGroups;
    return RedGroups{(uint32_t)(a < gc ? a : gc), (uint32_t)(b < gc ? b : gc)};
}

// the tiles [t0, t1) in 1..nt whose carry position t * TS - 1 lies in [st, st + v)
struct RedTileSpan {
    uint64_t t0, t1;
};
PSY_RT_HD RedTileSpan red_block_tiles(uint64_t st, uint32_t v, uint64_t TS, uint32_t nt) {
    // t * TS - 1 >= st  <=>  t >= (st + 1) / TS rounded up = (st + TS) / TS; t * TS - 1 < st + v  <=>  t * TS <= st + v
    uint64_t t0 = (st + TS) / TS, t1 = (st + v) / TS + 1u;
    if (t1 > nt) t1 = nt;
    if (t0 > t1) t0 = t1;
    return RedTileSpan{t0, t1};
}

// where tile t >= 1 (stream position P = t * TS) starts in a stream of decoded length slen: block b0
// whose first pair starts at s0, or (kRedNoBlock, slen) when the stream ended at or before P - 1.
// tblk: the block the scan recorded for the tile; bstart(b): the scanned start of block b.
struct RedCarry {
    uint32_t b0, s0;
};
template <class Load>
PSY_RT_HD RedCarry red_tile_carry(uint32_t P, uint32_t slen, uint32_t tblk, Load &&bstart) {
    if (P - 1u >= slen) return RedCarry{kRedNoBlock, slen};
    return RedCarry{tblk, bstart(tblk)};
}

}  // namespace psy
