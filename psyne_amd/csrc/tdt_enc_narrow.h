// tdt_enc_narrow.h — encode-narrow (tdt_encode_narrow_v): fp32 tensors to the width-2 blobs of their
// bf16 / fp16 narrowing, in one pass.  The kernel and its launcher are in tdt_enc_narrow.hip, a
// translation unit of its own (psyne_amd/build.py).
//
// One 256-lane workgroup per tensor (message id = block index).  The narrowed message never exists
// in HBM: it lives as its two byte planes in LDS — plane 0 the low bytes, plane 1 the high bytes of
// kNarResident elements — through every phase, so a tensor of at most that many elements is read
// from HBM exactly once:
//   H  a lane loads 4 floats per step, narrows them, packs the low and the high bytes with one
//      v_perm_b32 each and writes one dword per plane; the 2 x 256 bins are counted on the way, in
//      kNarHistCopies copies picked by the lane (a gradient's high bytes take a handful of values:
//      one copy would serialise), a lane's four equal high bytes as one add of 4
//   M  the exact entropy chain (tdt_entropy.h) on waves 0 and 1, entropy > in-order sum / 2.  Two
//      positions give three mappings: under [1,0] and [0,1] a stream IS a plane, under [0,0] the
//      one stream is the message itself — a lane's 16 stream bytes are 8 bytes of each plane
//      under v_perm
//   C  count: per stream, 16 consecutive stream bytes per lane from LDS; SWAR run starts, the run
//      entering a lane from a team max-scan, ceil(L / 255) pairs per closed run, an add-scan.  Both
//      streams are counted before anything is stored, so the blob length E — and with it stream
//      1's place, the raw-fallback decision (E > w + 4) and the capacity decision — is known up
//      front, and no store needs a bound of its own
//   E  emit: the same arithmetic; a step's pairs are staged in LDS at their rank and flushed as
//      dword stores between the byte stores of the unaligned edges.  A run of more than
//      kNarLaneFull full pairs is filled by the whole workgroup.  The UNCP form is the marker and
//      the planes interleaved, 16 bytes per lane and store.
// A longer tensor takes the same phases over chunks of kNarResident elements, restaged from the
// source for C and for E (three reads of 4 bytes per element, on one workgroup); the run carries
// cross the chunks.  Blobs, lengths and statuses are the width-2 encode's of the narrowed bytes.
// Above the large-message threshold a tensor leaves this kernel for the tile passes of
// tdt_enc_narrow_tiled.h (two reads, one workgroup per chunk); its bytes are the same.
//
// Error feedback (tdt_encode_narrow_ef_v) is a second instance of every kernel that reads the source
// (template <bool EF>; the instances without it are the code they were).  Where a tensor has a residual
// r, every read of the source g becomes a read of g and r and one v_add_f32, v = g + r, and the narrowed
// halfword h is v's.  r' = v - widen(h) is stored by the LAST pass that reads the element, behind the
// status decision, by a lane that has read it in that pass — r is updated in place, so no read of r[e]
// may follow the write of r'[e]:
//   longer than kNarResident   H and C form v again from g and r (the sum is deterministic); the emit
//                              pass's restaging of a chunk stores the chunk's r' (the byte before a chunk
//                              travels in NarCarry::lastb, not through memory); on the UNCP routes the
//                              group copy stores it.  3 x (4 + 4) bytes read, 4 written per element
//   resident                   the planes are staged in H, before length and capacity are known, and v
//                              is not kept (64 VGPRs a lane): behind the decision one more pass reads g
//                              and r, narrows again and stores r'.  2 x (4 + 4) read, 4 written
//   tiles                      A reads g + r, E stores its own tile's r' on both routes and reads no
//                              residual outside its tile: the halfword before the tile comes from the
//                              tile record (NarTileRec::prev, written by A).  2 x (4 + 4) read, 4 written
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psy {

constexpr int kNarTeam = 256;              // lanes per workgroup
constexpr uint32_t kNarResident = 16384;   // elements whose planes stay in LDS (2 x 16 KiB: a 64 KiB fp32 tensor)
constexpr uint32_t kNarStep = 4096;        // stream bytes per count / emit step (16 per lane)
constexpr uint32_t kNarHistCopies = 8;     // copies of the 2 x 256 bins
constexpr uint32_t kNarLaneFull = 16;      // full pairs one lane stages itself
constexpr uint32_t kNarBF16 = 0x13, kNarF16 = 0x12;  // TDT_ELEM_BF16_FROM_F32, TDT_ELEM_F16_FROM_F32
constexpr int32_t kNarStElement = 13;      // TDT_E_ELEMENT

struct NarrowArgs {
    const uint64_t *msgs;        // source addresses (fp32, 4-byte aligned)
    const uint64_t *sizes;       // source bytes
    uint32_t n_msgs;
    const uint8_t *elem_codes;   // null: `elem` for every message
    uint32_t elem;
    const uint64_t *blobs;       // blob addresses, any alignment
    const uint64_t *blob_cap;
    uint64_t *out_len;
    int32_t *status;
    uint64_t min_tensor;
    int32_t policy_on;           // as EncodeArgs::policy_on
    int32_t raw_fallback;        // TDT_OPT_RAW_FALLBACK
    const uint32_t *mark;        // null, or one word per message: non-zero = the tile passes have it (tdt_enc_narrow_tiled.h)
    const uint64_t *resid;       // null: tdt_encode_narrow_v; else the residual addresses of tdt_encode_narrow_ef_v (0: none)
};

// One launch per 2^24 - 1 messages on stream s.  Returns a hipError_t as int (0: launched).
int launch_encode_narrow(const NarrowArgs &a, hipStream_t s);

}  // namespace psy
