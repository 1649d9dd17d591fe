// tdt_anyws.h — encode and decode for the word sizes the tuned kernels do not cover.
//
// The tuned kernels (tdt_encode.h, tdt_decode.h) are specialised for word sizes 1, 2, 4, 8 and
// 16 (a 16-byte group holds whole words).  Every other width in 1..64 ("generic": 3 for RGB8, 12
// for float3, 24 / 32 / 40 for small structs, ...) goes through the two kernels of
// tdt_anyws.hip, which take the word size as a runtime argument:
//
//   encode   one 256-lane workgroup per message (message id = block index); a message above the
//            batch's large-message threshold runs the tile pipeline below instead.
//            Histograms ws x 256 in LDS, the exact entropy chain (tdt_log2.h), then per stream a
//            split + RLE over chunks of kAnyChunk message bytes.  Stream 0 is emitted where the
//            header ends and its pair count places stream 1, so no separate count pass is needed.
//   decode   blobs whose header carries a generic width are DEFERRED by the tuned decode kernels
//            (blob_check returns ST_DEFER, the kernel appends the blob id to a device list); one
//            follow-up launch, grid-strided over the device-side count, decodes the listed blobs.
//            A batch without such blobs pays that one near-empty launch.  A deferred blob that
//            decodes to more than the batch's large-blob threshold, with one or two referenced
//            streams, leaves that launch for the decode tile pipeline below (32 KiB output tiles).
//
// Reference: include/psyne/protocol/tdt_compression.hpp (line numbers as in tdt_encode.h /
// tdt_decode.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tdt_anyws_dec_tiles.h"

namespace psy {

struct EncodeArgs;
struct DecodeArgs;

constexpr int kAnyWsMax = 64;           // largest word size the library encodes and decodes
constexpr int kAnyTeam = 256;           // lanes per workgroup of both kernels
constexpr uint32_t kAnyChunk = 4096;    // encode: message bytes per split + RLE chunk (16 per lane)
constexpr uint32_t kAnyDecPairs = 2048; // decode: pairs per chunk (8 per lane)
static_assert(kAnyDecPairs == kAnyDecBlockPairs, "a block of the tiled decode is one chunk of pairs");
constexpr uint32_t kAnyTile = 65536;    // tiled encode: message bytes per tile
constexpr uint32_t kAnySpanTiles = 8;   // tiled encode: tile records per histogram workgroup (512 KiB spans)
static_assert(kAnyTile % kAnyChunk == 0, "a tile is a whole number of chunks");

// The tuned kernels' widths (whole words per 16-byte group); everything else in 1..kAnyWsMax is generic.
inline bool anyws_tuned(int ws) { return ws == 1 || ws == 2 || ws == 4 || ws == 8 || ws == 16; }
inline bool anyws_generic(int ws) { return ws >= 1 && ws <= kAnyWsMax && !anyws_tuned(ws); }

// ---- the tiled encode of long messages ---------------------------------------------------
// A message above the batch's large-message threshold (max(large_min, 1/4096 of the batch's bytes),
// the tuned plan's rule) leaves the one-workgroup kernel: a plan kernel (one lane per message) claims
// an AnyLarge record and ceil(n / kAnyTile) AnyTile records for it from the budgets below and sets
// its mark, and tdt_encode_any_kernel returns at a marked message.  Then, every launch a fixed grid
// striding over the device-side counts:
//   histogram  one workgroup per kAnySpanTiles tile records (512 KiB of one message as a rule): ws x
//              256 counts in LDS, the non-zero ones added to the message's histogram in global memory
//   mapping    one workgroup per large message: the entropy chain and the threshold of the
//              one-workgroup kernel over that histogram (which it zeroes again); the mapping bits
//              go into the record.  MODE_MAPPED has the caller's bits there already (the plan
//              validated them) and runs neither of the two.
//   count      per (tile, stream): the chunk loop without stores — first and last run start, pairs
//              of the runs closed inside the tile (tdt_anyws_tiles.h)
//   scan       one workgroup per large message: every tile's carried run start and pair base;
//              the header, the mapping, both streams' length words, the blob length and the
//              status.  MODE_SIZES ends here.
//   emit       per (tile, stream): the chunk loop with its carries from the tile's record; the
//              stream's last tile also writes the final run.  A passthrough (UNCP) message's tiles
//              copy their 64 KiB each (copy_shifted); the plan wrote its marker, length and status.
// A message that finds a budget spent, or an invalid caller mapping, stays unmarked: the
// one-workgroup kernel takes it as before.  The blobs are the one-workgroup kernel's byte for byte.
struct AnyLarge {
    const uint8_t *src;  // the message
    uint8_t *dst;        // its slot (null: the size pass)
    uint64_t cap;        // the slot's capacity
    uint64_t mapbits;    // bit p: the stream of byte position p
    uint32_t msg, n;     // message id, size (< 2^32)
    uint32_t ws;         // word size of the launch that claimed the record (0: a claim that found no tiles)
    uint32_t flags;      // kAnyUncp
    uint32_t tile0, ntiles;
    uint32_t pairs[2];   // (the scan) pairs of either stream
    uint32_t ok;         // (the scan) the blob fits its slot: the emit pass writes it
    uint32_t pad;
};
struct AnyTile {  // record tile0 + t of its message is the message's tile t
    uint32_t first[2], last[2], inner[2];  // (the count pass) per stream, tdt_anyws_tiles.h
    uint32_t carry[2], base[2];            // (the scan) carried run start + 1, pairs before the tile's own
};
constexpr uint32_t kAnyUncp = 1u;
struct AnyTiledArgs {
    AnyLarge *large;
    AnyTile *tiles;
    uint32_t *hist;            // kAnyWsMax x 256 counts per large record, all zero between calls
    uint32_t *mark;            // one word per message of the batch: non-zero = the tile pipeline has it
    unsigned long long *cnt;   // the counter block (AnyCount, tdt_plan.h)
    uint32_t lcap, tcap;       // the budgets of this call (0, 0: nothing is tiled, claims are still counted)
    uint32_t bytes_at;         // pair tables: the counter that holds the batch's bytes
    uint32_t grid;             // workgroups of a tile-level launch
    uint64_t large_min;
};

// Encode (mode MODE_ENCODE / MODE_MAPPED: slotted output, a.slot_off set; MODE_ANALYZE:
// histograms, entropies and mapping, no blob) of a.n_msgs messages at word size ws.
// pair (MODE_ENCODE / MODE_MAPPED): a.in_off and a.slot_off are the (begin, end) pair tables of a
// scattered batch (table_at, tdt_plan.h), and a MODE_MAPPED batch's a.mapping_in holds one u64 of
// mapping bits per message (tdt_mapbits.h); or, pair with MODE_SIZES, the size pass: a.in_off alone
// is a pair table, the blob lengths go to a.out_len (and, a.map_out set, the mapping bits of every
// compressed message there, one u64 each) and nothing else is written.
// tiled (not MODE_ANALYZE): the plan kernel and the tile pipeline run beside the one-workgroup
// kernel; null: every message on the one-workgroup kernel.  Returns a hipError_t as int (0: launched).
int launch_encode_any(const EncodeArgs &a, int ws, int mode, hipStream_t s, bool pair = false,
                      const AnyTiledArgs *tiled = nullptr);

// ---- the tiled decode of long blobs --------------------------------------------------------
// A deferred blob that decodes to more than the batch's large-blob threshold (the tuned decode
// plan's rule: max(large_min, 1/4096 of the batch's blob bytes)), fits its slot (the look-back
// route: out_cap) and has one or two referenced streams — any number of stored ones, any mapping
// shape, mapping_size >= ws — leaves the one-workgroup kernel (the arithmetic: tdt_anyws_dec_tiles.h):
//   plan    one lane per entry of the deferred list: parses the header and the stream table, claims
//           an AnyDecLarge record, ceil(np_r / 2048) block sums per referenced stream and
//           ceil(wc / Tw) tiles from the budgets below, writes the blob's status and length and
//           sets the entry's mark; tdt_decode_any_kernel skips a marked entry
//   blocks  one wave per 2,048-pair block: the sum of its counts
//   scan    one workgroup per long blob: per stream the exclusive prefix of the block sums, in
//           place, clamped at the stream's share of the output
//   tile    one workgroup per 32 KiB output tile: per stream a search of the prefix for the tile's
//           first block, the chunk loop of the one-workgroup kernel from there with every pair cut
//           to the tile, expanded into the stream's plane in LDS (zeroed first); then the planes
//           are recombined through the mapping's rank table, 16 output bytes per lane and store
// Every launch but the plan is a fixed grid striding over the device-side counts.  A blob that finds
// a budget spent, does not fit or has three or more referenced streams stays unmarked: the
// one-workgroup kernel decodes it (or reports it) as before.  The output bytes are that kernel's.
struct AnyDecLarge {
    const uint8_t *blob;  // the blob, and its length (every load is bounded by it)
    uint64_t len;
    uint8_t *dst;         // where it decodes to
    uint32_t orig, ws;    // decoded size, word size (0: a claim that found a budget spent — no launch's record)
    uint32_t tile0, ntiles;
    uint32_t soff[2], np[2];  // per referenced stream: the pairs' offset in the blob, how many
    uint32_t k[2];            // positions per word (k[1] = 0: one referenced stream)
    uint32_t blk0[2], nb[2];  // its block sums [blk0, blk0 + nb); blk0[1] = blk0[0] + nb[0]
    // the mapping's rank table: byte position p of a word is byte (rank[p] & 63) of its stream's k
    // bytes of that word — the inverse of the stream's position table; bit 7: the second stream
    uint8_t rank[kAnyWsMax];
};
constexpr uint32_t kAnyDecSecond = 0x80u;
struct AnyDecArgs {
    AnyDecLarge *large;
    uint32_t *bsum;            // block sums, then (the scan) their clamped exclusive prefixes
    uint32_t *mark;            // one word per entry of the deferred list: non-zero = the tile pipeline has it
    unsigned long long *cnt;   // the counter block (AnyDecCount, tdt_plan.h)
    const unsigned long long *batch_bytes;  // pair tables: the counter that holds the batch's blob bytes
    uint32_t lcap, bcap, tcap; // the budgets of this call (0: nothing is tiled, claims are still counted)
    uint32_t grid;             // workgroups of a tile-level launch
    uint64_t large_min;
};

// Decode the blobs listed in a.dlist[0 .. *a.dcount) (slotted: a.slot_off; compacted: the
// a.out_off the look-back kernel wrote, against a.out_cap); `grid` workgroups stride over them.
// pair: a.slot_off is a scattered batch's pair table.
// tiled: the plan kernel and the tile pipeline run beside the one-workgroup kernel (with budgets of
// 0 the plan alone, counting); null: every blob on the one-workgroup kernel.  seen (may be null):
// pinned, where the one-workgroup kernel leaves the length of a list that is not empty (0 until then).
int launch_decode_any(const DecodeArgs &a, uint32_t grid, hipStream_t s, bool pair = false,
                      const AnyDecArgs *tiled = nullptr, uint32_t *seen = nullptr);

}  // namespace psy
