// tdt_anyws_tiles.h — the arithmetic of the tiled generic-width encode (tdt_anyws.h) that is not a
// kernel: where a tile's bytes lie in a stream, which message byte precedes them, how many pairs a
// run takes, and how the per-tile run records combine into every tile's carried run start and pair
// base.
//
// A message of n bytes (n % ws == 0) at word size ws has a mapping of ws bits, bit p = the stream
// (0 or 1) of byte position p of every word.  Stream s holds k_s = (positions mapped to s) bytes of
// every word, in message order, so message byte j is preceded by
//     pos_s(j) = (j / ws) * k_s + before_s(j % ws)
// bytes of stream s (before_s(p): the positions below p mapped to s).  A tile is message bytes
// [jb, je); its bytes of stream s are the stream's [pos_s(jb), pos_s(je)).  Tile boundaries are not
// word boundaries for most widths.
//
// The run-length code (simple_rle_compress) emits, for every run of L equal bytes, ceil(L / 255)
// pairs (count, value): 255, ..., 255, remainder.  A stream byte that differs from the one before
// it — and the stream's first byte — is a RUN START; each start but the stream's first closes the run
// before it, and the last run closes at the stream's end.  Per (tile, stream) the count pass records
//     first   the tile's first run start as a stream position + 1 (0: the tile has none)
//     last    its last run start + 1 (0: none)
//     inner   the pairs of the runs closed by every start of the tile but the first
// The tile's first start closes a run that began in an earlier tile, at the CARRY: the last run
// start before the tile.  The scan gives every tile its carry (a running maximum of `last`) and
// its PAIR BASE, the pairs written by the tiles before it; the tile itself writes the crossing
// run's pairs and then its inner ones, and the stream's last tile the final run's behind them.
//
// Plain host / device C++, so that a host program can drive it over start sets
// (tests/cpp/test_anyws_tiles.cpp); the kernels are in tdt_anyws.hip.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PSY_AT_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define PSY_AT_HD inline
#endif

namespace psy {

// positions below p (0 <= p <= ws <= 64) mapped to stream s
PSY_AT_HD uint32_t any_before(uint64_t bits, uint32_t s, uint32_t p) {
    const uint64_t below = p >= 64u ? ~0ull : (1ull << p) - 1ull;
    const uint32_t ones = (uint32_t)__builtin_popcountll(bits & below);
    return s ? ones : p - ones;
}

// bytes of stream s before message byte j (j <= n < 2^32, so the result is below 2^32 as well)
PSY_AT_HD uint32_t any_stream_pos(uint32_t j, uint32_t ws, uint64_t bits, uint32_t s) {
    const uint32_t w = j / ws, p = j - w * ws;
    return w * any_before(bits, s, ws) + any_before(bits, s, p);
}

// the stream bytes [b, e) of message bytes [jb, je)
struct AnyRange {
    uint32_t b, e;
};
PSY_AT_HD AnyRange any_tile_range(uint32_t jb, uint32_t je, uint32_t ws, uint64_t bits, uint32_t s) {
    return AnyRange{any_stream_pos(jb, ws, bits, s), any_stream_pos(je, ws, bits, s)};
}

// The message byte that holds the stream byte before stream position pos_s(jb): the nearest
// position below jb mapped to s, at most ws bytes back.  Precondition: pos_s(jb) > 0 (such a byte
// exists); without one the result is jb itself.
PSY_AT_HD uint32_t any_pred_pos(uint32_t jb, uint32_t ws, uint64_t bits, uint32_t s) {
    uint32_t p = jb % ws;
    for (uint32_t d = 1; d <= ws && d <= jb; ++d) {
        p = p ? p - 1u : ws - 1u;
        if (((bits >> p) & 1ull) == s) return jb - d;
    }
    return jb;
}

// pairs of a run of L >= 1 bytes: 255, ..., 255, remainder
PSY_AT_HD uint32_t any_run_pairs(uint32_t L) { return (L + 254u) / 255u; }

// ---- the scan over a stream's tiles -------------------------------------------------------
struct AnyTileRuns {
    uint32_t first, last, inner;  // (see the head of this file)
};
struct AnyCarry {
    uint32_t start;  // the last run start + 1 before the tile (0: the tile begins the stream)
    uint32_t pairs;  // pairs written before the tile's own
};
// pairs of the run a tile's first start closes (none when the start is the stream's first byte)
PSY_AT_HD uint32_t any_cross_pairs(uint32_t first, uint32_t carry) {
    return first && carry ? any_run_pairs(first - carry) : 0u;
}
// what a tile writes: the crossing run, then its inner runs
PSY_AT_HD uint32_t any_tile_pairs(AnyTileRuns t, uint32_t carry) { return any_cross_pairs(t.first, carry) + t.inner; }
// the carry of the next tile (run starts ascend, so the maximum is the latest)
PSY_AT_HD AnyCarry any_scan_step(AnyCarry c, AnyTileRuns t) {
    return AnyCarry{t.last > c.start ? t.last : c.start, c.pairs + any_tile_pairs(t, c.start)};
}
// the run that closes at the end of a stream of S >= 1 bytes, given the carry behind its last tile
PSY_AT_HD uint32_t any_final_pairs(uint32_t S, uint32_t start) { return any_run_pairs(S - (start - 1u)); }

}  // namespace psy
