// tdt_enc_lmap.h — the head of the tile pipeline when the caller gives the mappings (the known-mapping
// scattered encode, tdt_encode_mapped_v / _vp: DESIGN.md §4 "Known mappings").
//
// The ordinary pipeline starts with the span pass (TL 1: span histograms, the count under the
// speculated mapping, and the copy of a large passthrough message) and the map pass (TL 4: the
// mapping from the span histograms, and the count pass's tile list).  With the mapping known neither
// has anything to compute.  Two small kernels stand in for them:
//   tdt_encode_lmap_kernel   one wave per large-message record: LMeta::mapbits from the caller's
//                            bits, every tile of the message on the count pass's list (rtiles /
//                            EC_RECOUNT) and marked kRecount — no span pass has counted it, so the
//                            count pass must not take its "already counted" shortcut; a bad mapping
//                            is reported here (TDT_E_BAD_MAPPING, length 0) and the record is taken
//                            out (msg = kNone), which the count list, the scan and the emit pass skip;
//   tdt_encode_lcopy_kernel  one team per span of a large PASSTHROUGH message: the span pass's copy
//                            branch alone.
// Then the count pass (TL 2), the scan and the emit pass (TL 3) run as they are: they read the
// mapping from LMeta, whoever wrote it.  Both kernels read the batch through its pair tables (the
// mapped encode is a scattered call) and are bounded by the plan's device-side counts.
// (Non-template kernels: this header is included once, by tdt_api.hip.)
#pragma once
#include "tdt_encode.h"

namespace psy {

// should_transform :186-201 + compress_tdt's size guard :364-367, as encode_one evaluates them
__device__ __forceinline__ bool lmap_compresses(const EncodeArgs &a, uint64_t n, uint32_t ws) {
    return a.policy_on && n >= a.min_tensor && (n % 4 == 0) && n >= 64 && (n % ws == 0) && n > 0 && n < (1ull << 32);
}

__global__ __launch_bounds__(64) void tdt_encode_lmap_kernel(EncodeArgs a, uint32_t ws) {
    const uint32_t nl = umin(a.pcnt[lo32(EC_LARGE)], a.lcap);
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t *mapbits = reinterpret_cast<const uint64_t *>(a.mapping_in);
    for (uint32_t j = blockIdx.x; j < nl; j += gridDim.x) {
        LMeta *lm = a.lmeta + j;
        const uint32_t msg = lm->msg;
        if (msg == kNone || msg >= a.n_msgs) continue;  // fell back to the whole-message kernel
        const uint64_t n = a.in_off[table_at<true>(msg, 1)] - a.in_off[table_at<true>(msg, 0)];
        if (!lmap_compresses(a, n, ws)) continue;  // passthrough: tdt_encode_lcopy_kernel copies it
        const uint64_t bits = mapbits[msg];
        const uint32_t nt = lm->ntiles, t0 = lm->tile0;
        if (!mapbits_ok(bits, (int)ws)) {
            if (lane == 0) {
                if (a.status) a.status[msg] = ST_BAD_MAPPING;
                if (a.out_len) a.out_len[msg] = 0;
                lm->msg = kNone;
            }
            continue;
        }
        uint32_t base = 0;
        if (lane == 0) {
            lm->mapbits = (uint32_t)bits;  // (tuned widths: at most 16 positions)
            base = (uint32_t)atomicAdd(a.rcount, (unsigned long long)nt);
        }
        base = rdlane(base, 0);
        // (the plan claimed this message's tiles inside the budget: tile0 + ntiles <= tcap, and the
        // listed tiles of all messages are at most the claimed ones; the tests keep a logic error
        // from becoming a wild write)
        for (uint32_t t = lane; t < nt; t += 64u) {
            if (base + t < a.tcap) a.rtiles[base + t] = ((uint64_t)t << 32) | j;
            if (t0 + t < a.tcap) a.trec[t0 + t].clean = kRecount;
        }
    }
}

__global__ __launch_bounds__(512) void tdt_encode_lcopy_kernel(EncodeArgs a, uint32_t ws) {
    const uint32_t ns = umin(a.pcnt[lo32(EC_SPANS)], a.tcap / kSpanTiles);
    const uint32_t tid = threadIdx.x;
    constexpr uint64_t kSpanBytes = 16ull * kTileGroups * kSpanTiles;
    for (uint32_t i = blockIdx.x; i < ns; i += gridDim.x) {
        const uint64_t e = a.spans[i];
        const uint32_t lj = (uint32_t)e, span = (uint32_t)(e >> 32);
        if (lj == kNone || lj >= a.lcap) continue;  // a message that did not fit the budgets
        const uint32_t msg = a.lmeta[lj].msg;
        if (msg == kNone || msg >= a.n_msgs) continue;
        const uint64_t off0 = a.in_off[table_at<true>(msg, 0)];
        const uint64_t n = a.in_off[table_at<true>(msg, 1)] - off0;
        if (lmap_compresses(a, n, ws)) continue;
        const uint64_t slot_b = a.slot_off[table_at<true>(msg, 0)], slot_e = a.slot_off[table_at<true>(msg, 1)];
        const uint64_t E = n + 4, t0 = kSpanBytes * span;
        const bool fits = E <= slot_e - slot_b;
        if (span == 0 && tid == 0) {
            if (a.status) a.status[msg] = fits ? ST_OK : ST_CAPACITY;
            if (a.out_len) a.out_len[msg] = fits ? E : 0;
        }
        if (!fits || t0 >= n) continue;
        uint8_t *dst = a.out + slot_b;
        if (span == 0 && tid < 4) dst[tid] = (uint8_t)(kMagicUNCP >> (8 * tid));
        team_copy_g2g<512>(dst + 4 + t0, a.in + off0 + t0, n - t0 < kSpanBytes ? n - t0 : kSpanBytes);
    }
}

}  // namespace psy
