// tdt_anyws.h — encode and decode for the word sizes the tuned kernels do not cover.
//
// The tuned kernels (tdt_encode.h, tdt_decode.h) are specialised for word sizes 1, 2, 4, 8 and
// 16 (a 16-byte group holds whole words).  Every other width in 1..64 ("generic": 3 for RGB8, 12
// for float3, 24 / 32 / 40 for small structs, ...) goes through the two kernels of
// tdt_anyws.hip, which take the word size as a runtime argument:
//
//   encode   one 256-lane workgroup per message (message id = block index, no plan kernel).
//            Histograms ws x 256 in LDS, the exact entropy chain (tdt_log2.h), then per stream a
//            split + RLE over chunks of kAnyChunk message bytes.  Stream 0 is emitted where the
//            header ends and its pair count places stream 1, so no separate count pass is needed.
//   decode   blobs whose header carries a generic width are DEFERRED by the tuned decode kernels
//            (blob_check returns ST_DEFER, the kernel appends the blob id to a device list); one
//            follow-up launch, grid-strided over the device-side count, decodes the listed blobs.
//            A batch without such blobs pays that one near-empty launch.
//
// Reference: include/psyne/protocol/tdt_compression.hpp (line numbers as in tdt_encode.h /
// tdt_decode.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psy {

struct EncodeArgs;
struct DecodeArgs;

constexpr int kAnyWsMax = 64;           // largest word size the library encodes and decodes
constexpr int kAnyTeam = 256;           // lanes per workgroup of both kernels
constexpr uint32_t kAnyChunk = 4096;    // encode: message bytes per split + RLE chunk (16 per lane)
constexpr uint32_t kAnyDecPairs = 2048; // decode: pairs per chunk (8 per lane)

// The tuned kernels' widths (whole words per 16-byte group); everything else in 1..kAnyWsMax is generic.
inline bool anyws_tuned(int ws) { return ws == 1 || ws == 2 || ws == 4 || ws == 8 || ws == 16; }
inline bool anyws_generic(int ws) { return ws >= 1 && ws <= kAnyWsMax && !anyws_tuned(ws); }

// Encode (mode MODE_ENCODE / MODE_MAPPED: slotted output, a.slot_off set; MODE_ANALYZE:
// histograms, entropies and mapping, no blob) of a.n_msgs messages at word size ws.
// pair (MODE_ENCODE / MODE_MAPPED): a.in_off and a.slot_off are the (begin, end) pair tables of a
// scattered batch (table_at, tdt_plan.h), and a MODE_MAPPED batch's a.mapping_in holds one u64 of
// mapping bits per message (tdt_mapbits.h); or, pair with MODE_SIZES, the size pass: a.in_off alone
// is a pair table, the blob lengths go to a.out_len (and, a.map_out set, the mapping bits of every
// compressed message there, one u64 each) and nothing else is written.  Returns a hipError_t as
// int (0: launched).
int launch_encode_any(const EncodeArgs &a, int ws, int mode, hipStream_t s, bool pair = false);

// Decode the blobs listed in a.dlist[0 .. *a.dcount) (slotted: a.slot_off; compacted: the
// a.out_off the look-back kernel wrote, against a.out_cap); `grid` workgroups stride over them.
// pair: a.slot_off is a scattered batch's pair table.
int launch_decode_any(const DecodeArgs &a, uint32_t grid, hipStream_t s, bool pair = false);

}  // namespace psy
