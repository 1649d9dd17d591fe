// tdt_anyws_dec_tiles.h — the arithmetic of the tiled generic-width decode (tdt_anyws.h) that is
// not a kernel: which words an output tile covers, which decoded bytes of a stream land in it,
// in which 2,048-pair block those bytes begin, and how a pair is cut to a tile.
//
// A blob that blob_check (tdt_decode.h) has passed decodes to `orig` bytes at word size ws:
// wc = orig / ws >= 1 whole words, then orig - wc * ws zero bytes.  A referenced stream r owns the
// byte positions P_r (ascending, k_r = |P_r| of them) of every word, so its share of the output is
// S_r = wc * k_r bytes and decoded byte q of r is output byte
//     (q / k_r) * ws + P_r[q mod k_r]                      for q < min(S_r, sum of the counts);
// every other byte below orig is zero (recombine_byte_streams over its zero-initialised result).
// The stream is np_r = slen_r / 2 pairs (count, value); an odd trailing byte is no pair.
//
// TILES.  Tile t covers words [t * Tw, min((t + 1) * Tw, wc)), Tw = kAnyDecTile / ws: at most
// 32 KiB of output, 512 words at width 64 and 10,922 at width 3.  The bytes past the last whole
// word belong to the last tile.  Tile t's range in stream r is [w0 * k_r, w1 * k_r).
//
// BLOCKS.  Block b of a stream is its pairs [b * kAnyDecBlockPairs, min((b + 1) * kAnyDecBlockPairs, np_r));
// its counts sum to at most 2,048 * 255 = 522,240.  E_r[b] is the exclusive prefix of the block
// sums, CLAMPED at S_r: a stream's counts may sum past 2^32 (16,843,010 pairs of count 255 do),
// S_r = wc * k_r <= orig is below 2^32, and no tile asks for a position at or above S_r.  An
// entry below S_r is therefore exact.
//
// A tile's first block is the LARGEST b with E_r[b] <= q0, q0 the start of its range: blocks that
// hold only count-0 pairs give equal prefixes, and the last of them is the one that still has the
// byte at q0 ahead of it.  With q0 at or past the stream's total the search lands on the last block,
// whose pairs all end at or before q0: the tile gets no byte of that stream, only zeros.
//
// Plain host / device C++, so that a host program can drive it tile by tile against a serial decode
// (tests/cpp/test_anyws_dec_tiles.cpp); the kernels are in tdt_anyws.hip.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PSY_ADT_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define PSY_ADT_HD inline
#endif

namespace psy {

constexpr uint32_t kAnyDecTile = 32768;  // tiled decode: output bytes per tile (the tuned decode's tile)
constexpr uint32_t kAnyDecBlockPairs = 2048;  // pairs per block: the one-workgroup kernel's chunk (kAnyDecPairs, tdt_anyws.h)
constexpr uint32_t kAnyDecBlockMax = kAnyDecBlockPairs * 255u;  // the largest count sum of one block

// words per tile at word size ws (1 <= ws <= 64)
PSY_ADT_HD uint32_t any_dec_tile_words(uint32_t ws, uint32_t tile = kAnyDecTile) { return tile / ws; }
// tiles of wc >= 1 words
PSY_ADT_HD uint32_t any_dec_ntiles(uint32_t wc, uint32_t tw) { return (wc + tw - 1u) / tw; }
// blocks of np pairs
PSY_ADT_HD uint32_t any_dec_nblocks(uint32_t np) { return (np + kAnyDecBlockPairs - 1u) / kAnyDecBlockPairs; }

// the words [w0, w1) of tile t
struct AnyDecWords {
    uint32_t w0, w1;
};
PSY_ADT_HD AnyDecWords any_dec_tile_words_of(uint32_t t, uint32_t wc, uint32_t tw) {
    const uint64_t a = (uint64_t)t * tw, b = a + tw;
    return AnyDecWords{(uint32_t)(a < wc ? a : wc), (uint32_t)(b < wc ? b : wc)};
}
// the output bytes [jb, je) of tile t: its words, and for the last tile the bytes past the last whole word
struct AnyDecBytes {
    uint32_t jb, je;
};
PSY_ADT_HD AnyDecBytes any_dec_tile_bytes(uint32_t t, uint32_t ntiles, AnyDecWords w, uint32_t ws, uint32_t orig) {
    return AnyDecBytes{w.w0 * ws, t + 1u == ntiles ? orig : w.w1 * ws};
}
// the decoded bytes [q0, q1) of a stream with k positions per word that land in words [w0, w1)
struct AnyDecRange {
    uint32_t q0, q1;
};
PSY_ADT_HD AnyDecRange any_dec_stream_range(AnyDecWords w, uint32_t k) { return AnyDecRange{w.w0 * k, w.w1 * k}; }

// the scan's combine: the prefix behind a block of count sum `sum`, clamped at the stream's share S
PSY_ADT_HD uint32_t any_dec_scan_step(uint32_t carry, uint64_t sum, uint32_t S) {
    const uint64_t x = (uint64_t)carry + sum;
    return x < S ? (uint32_t)x : S;
}

// the largest b in [0, nb) with E[b] <= q0 (E ascending, E[0] = 0; nb >= 1)
template <class Load>
PSY_ADT_HD uint32_t any_dec_first_block(Load &&E, uint32_t nb, uint32_t q0) {
    uint32_t lo = 0u, hi = nb;  // E[lo] <= q0; every b >= hi has E[b] > q0
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (E(mid) <= q0) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A pair whose bytes are the stream's [a, a + c) cut to [q0, q1): `n` bytes, the first at q0 + off
struct AnyDecClip {
    uint32_t off, n;
};
PSY_ADT_HD AnyDecClip any_dec_clip(uint64_t a, uint32_t c, uint32_t q0, uint32_t q1) {
    const uint64_t e = a + c;
    const uint64_t lo = a > q0 ? a : (uint64_t)q0, hi = e < q1 ? e : (uint64_t)q1;
    return hi > lo ? AnyDecClip{(uint32_t)(lo - q0), (uint32_t)(hi - lo)} : AnyDecClip{0u, 0u};
}

// output byte (below wc * ws) of decoded byte q of a stream with positions P[0 .. k)
PSY_ADT_HD uint32_t any_dec_out_byte(uint32_t q, uint32_t k, uint32_t ws, const uint8_t *P) {
    const uint32_t w = q / k;
    return w * ws + P[q - w * k];
}

}  // namespace psy
