// tdt_enc_narrow_tiled.h — the tiled form of encode-narrow (tdt_enc_narrow.h): the records and the
// arguments of its passes.  The kernels are in tdt_enc_narrow.hip beside the one-workgroup kernel,
// whose nar_* helpers they share; the arithmetic of the tile records is tdt_anyws_tiles.h's.
//
// A tensor above the large-message threshold leaves its one workgroup and is encoded as tiles of
// kNarTile = kNarResident elements (64 KiB of source: the planes of one tile are the LDS layout of the
// one-workgroup kernel, and the tile edges are its chunk edges), one workgroup per tile.  The source
// is read twice: once to analyse, once to emit.  Passes, all on the caller's stream, in order
// (DESIGN.md §4); the host reads nothing back:
//   plan   one lane per tensor.  The rule: a valid code, source, size (and residual) 4-byte aligned, a wire size
//          below 2^32, a source size above large_min (no 1/4096-of-the-batch term: the one-workgroup
//          path costs three reads however busy the device is).  Such a tensor claims
//          (workgroup-aggregated atomics) one NarLarge record and ceil(ne / kNarTile) NarTile records;
//          within the budgets its record is filled, its tile records get their owner and its mark
//          word is set — tdt_encode_narrow_kernel returns at a marked tensor.  Over a budget: no mark,
//          the tile records it reached are emptied, the one workgroup keeps the tensor.  Claims are
//          counted beyond the budgets too, so that the next call grows them.
//   A      analyse, one workgroup per tile (the tiles of a tensor the routing sends to UNCP skip it):
//          the tile is staged once (nar_stage<true>: load, narrow, planes and 8 histogram copies in
//          LDS); the copies are reduced and added to the tensor's 2 x 256 bins in global memory; and
//          from the same resident planes the run records (first, last, inner: tdt_anyws_tiles.h) of
//          ALL THREE candidate streams — plane 0, plane 1, the interleaved message — are counted in one
//          sweep.  Two byte positions admit the mappings [1,0], [0,1] and [0,0] only, so every stream
//          the mapping can choose is one of the three: counting them before the mapping is known is
//          what makes a third read of the source unnecessary.
//   M      map and scan, one workgroup per large tensor: the entropy chain and the decision of the
//          one-workgroup kernel over the global bins (zeroed again behind the read); the chosen
//          streams' tile records scanned (any_scan_step, any_final_pairs) into every tile's carried run
//          start and pair base and both pair totals; the blob length E, the raw-fallback and capacity
//          decisions, status and length; for a TDT blob the header and the length words.  Every
//          refusal precedes the first store to the blob.
//   E      emit, one workgroup per tile.  A refused tensor's tiles do nothing.  An UNCP tensor's (by
//          the routing, or fallen back) narrow their 32 KiB of wire bytes to dst + 4 + 2 eb, tile 0
//          the marker too.  Otherwise the tile is restaged (nar_stage<false>) and nar_step<true> runs
//          over the chosen stream(s) from the record's carry, writing at pairs[s] + 2 base: the run
//          that crosses into the tile first, and in a stream's last tile the final run behind the rest.
//          With error feedback (tdt_enc_narrow.h) A reads g + r and leaves the halfword of the element
//          before its tile in the record; E takes it from there — that element's residual is another
//          workgroup's to overwrite — and stores r' for its own tile on either route.
//   snap   the counter block to the pinned snapshot (not under capture) and zero again for the next call.
// A run that spans many tiles (an all-zero tensor) is written by the one workgroup whose tile holds
// the start that closes it, or by the last tile: one nar_fill of at most 2 w / 255 bytes.
#pragma once
#include "tdt_enc_narrow.h"
#include "tdt_plan.h"

namespace psy {

constexpr uint32_t kNarTile = kNarResident;  // elements per tile (TDT_NARROW_TILE_ELEMS)
constexpr uint32_t kNarBins = 512;           // u32 bins per large record: 256 per plane

// candidate streams of a tile: plane 0, plane 1, the interleaved message
constexpr int kNarCand = 3;
constexpr uint32_t kNarUncpRouted = 1u, kNarIsBf16 = 2u;     // NarLarge::flags
constexpr uint32_t kNarRefused = 0u, kNarTdt = 1u, kNarRaw = 2u;  // NarLarge::route (pass M)

struct NarLarge {
    const uint8_t *src;
    uint8_t *dst;
    uint64_t cap;
    uint32_t msg, ne;        // tensor id, elements (< 2^31)
    uint32_t tile0, ntiles;  // its tile records [tile0, tile0 + ntiles); ntiles 0: a claim over a budget
    uint32_t flags;
    uint32_t route;          // (M) what the emit pass writes
    uint32_t m0, m1;         // (M) the mapping
    uint32_t pairs[2];       // (M) pairs of either stream
    uint8_t *res;            // the residual of tdt_encode_narrow_ef_v (null: none)
};
struct NarTileRec {  // record tile0 + t of its tensor is the tensor's tile t
    uint32_t owner;                                             // (plan) the NarLarge record, or kNarNoOwner
    uint32_t first[kNarCand], last[kNarCand], inner[kNarCand];  // (A) per candidate, tdt_anyws_tiles.h
    uint32_t carry[2], base[2];                                 // (M) per chosen stream
    uint32_t prev;                                              // (A, with error feedback) the wire halfword of the element before the tile
};
constexpr uint32_t kNarNoOwner = 0xffffffffu;

struct NarTiledArgs {
    NarrowArgs a;
    unsigned long long *cnt;  // the counter block (NarCount, tdt_plan.h), zero between calls
    uint32_t *mark;           // one word per tensor: non-zero = the tile passes have it
    NarLarge *large;
    NarTileRec *tiles;
    uint32_t *bins;           // kNarBins per large record, all zero between calls
    uint32_t lcap, tcap;      // the budgets of this call (0, 0: nothing is tiled, claims are still counted)
    uint32_t grid;            // workgroups of a tile-level launch
    uint64_t large_min;
};

// Each returns a hipError_t as int (0: launched), on stream s.
// plan: ahead of launch_encode_narrow, whose NarrowArgs::mark is t.mark.
int launch_narrow_plan(const NarTiledArgs &t, hipStream_t s);
// A, M and E behind it.
int launch_narrow_tiles(const NarTiledArgs &t, hipStream_t s);
// snap: kPlanSnapBytes of the counter block to `pin` (pinned; null: under capture) and zeroed.
int launch_narrow_snap(const NarTiledArgs &t, uint32_t *pin, hipStream_t s);

}  // namespace psy
