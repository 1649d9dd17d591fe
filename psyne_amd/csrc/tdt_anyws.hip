// tdt_anyws.hip — the generic-word-size encode and decode kernels (tdt_anyws.h) and their
// launchers.  A translation unit of its own, compiled beside tdt_api.hip and the per-word-size
// encode objects (psyne_amd/build.py).
//
// Reference lines restated here (include/psyne/protocol/tdt_compression.hpp):
//   should_transform :186-201, compress_tdt :363-399 (size guard :364-367), extract_features
//   :434-468, calculate_entropy :470-480, perform_clustering :507-525, separate_byte_streams
//   :527-549, simple_rle_compress :557-582, serialize :81-117;
//   deserialize :119-170, simple_rle_decompress :596-612, recombine_byte_streams :614-637.
// (the headers' non-template kernels are defined once, in tdt_api.hip)
#define PSY_ENC_INST_TU 1
#define PSY_DEC_INST_TU 1
#include "tdt_anyws.h"

#include <algorithm>

#include "tdt_anyws_tiles.h"
#include "tdt_copy.h"
#include "tdt_decode.h"
#include "tdt_encode.h"

// The mapping decision is bit-exact only if nothing below is contracted (tdt_log2.h).
#pragma clang fp contract(off)

namespace psy {
namespace {

constexpr int kAW = kAnyTeam / 64;  // waves per workgroup

// 16 message bytes at p (any alignment), bytes at index >= valid read as 0 and are not touched;
// nothing below `lo` or at / past `lim` is read.
__device__ __forceinline__ uint4 ld16_msg(const uint8_t *p, int valid, const uint8_t *lo, const uint8_t *lim) {
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    const uintptr_t a = (uintptr_t)p;
    if (valid >= 16) {
        if ((a & 15) == 0) {
            const u32x4_t v = gload<u32x4_t>(p);
            return make_uint4(v.x, v.y, v.z, v.w);
        }
        const uintptr_t a0 = a & ~(uintptr_t)3;
        if (a0 >= (uintptr_t)lo && a0 + 20 <= (uintptr_t)lim) {
            const uint32_t *q = reinterpret_cast<const uint32_t *>(a0);
            const uint32_t sh = (uint32_t)(a & 3);
            const uint32_t w0 = gload<uint32_t>(q), w1 = gload<uint32_t>(q + 1), w2 = gload<uint32_t>(q + 2),
                           w3 = gload<uint32_t>(q + 3);
            if (sh == 0) return make_uint4(w0, w1, w2, w3);
            const uint32_t w4 = gload<uint32_t>(q + 4);
            return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                              __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
        }
    }
    return ld16_any(p, valid);
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[4], int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// ---------------------------------------------------------------------------------------
// One chunk of one stream: split into LDS, SWAR run starts, the two team scans, pair stores.  The
// one-workgroup kernel walks a whole message with it; the tile passes walk one tile each.
//   CH_ENCODE  the one-workgroup kernel (put8 stores, or is empty in the size pass)
//   CH_COUNT   a tile's count pass: the carries begin at zero, so the tile's first run start finds
//              no start before it — it goes to *s_first (+ 1) and its run is not counted here
//   CH_EMIT    a tile's emit pass: the carries come from the tile's record.  A closed run of more
//              than 16 full pairs (longer than a chunk, so at most one per chunk) is handed to the
//              whole workgroup through *s_big instead of one lane's loop
enum : int { CH_ENCODE = 0, CH_COUNT = 1, CH_EMIT = 2 };
struct AnyRunCarry {  // uniform, carried across chunks
    uint32_t cstart;  // last run start + 1 (0: none yet)
    uint32_t cpairs;  // pairs emitted
    uint32_t lastb;   // the last stream byte so far
};
struct AnyBigRun {
    uint64_t po;         // where its 255-count pairs go
    uint32_t full, val;  // how many, of which value
};
constexpr uint32_t kAnyLaneFull = 16;  // full pairs one lane stores itself in the emit pass

template <int KIND, class Put8>
__device__ __forceinline__ void any_chunk(const uint8_t *base, const uint8_t *lim, uint64_t n, uint32_t ws, uint32_t s,
                                          uint32_t ks, uint64_t dpos, uint64_t cb64, const uint32_t *s_map,
                                          const uint32_t (*s_before)[kAnyWsMax + 1], uint8_t *s_buf,
                                          uint32_t (*s_slots)[kAW], AnyRunCarry &c, Put8 put8, uint32_t *s_first,
                                          AnyBigRun *s_big) {
    const uint32_t tid = threadIdx.x, n32 = (uint32_t)n;
    // this lane's 16 message bytes, their word and position
    const uint32_t cb = (uint32_t)cb64;
    const uint32_t j0 = cb + 16u * tid;
    const int valid = cb64 + 16u * tid >= n ? 0 : (n32 - j0 >= 16u ? 16 : (int)(n32 - j0));
    // the chunk's stream bytes [B, B + Lc): stream index of message byte j =
    // (j / ws)·ks + s_before[s][j % ws]
    const uint32_t ce = n32 - cb < kAnyChunk ? n32 : cb + kAnyChunk;
    const uint32_t wcb = cb / ws, pcb = cb - wcb * ws;
    const uint32_t wce = ce / ws, pce = ce - wce * ws;
    const uint32_t B = wcb * ks + s_before[s][pcb];
    const uint32_t Lc = wce * ks + s_before[s][pce] - B;
    if (valid) {
        const uint4 v = ld16_msg(base + j0, valid, base, lim);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t wj = j0 / ws, p = j0 - wj * ws;
        uint32_t rel = wj * ks - B;  // + s_before[s][p]: index in the chunk's stream bytes
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < valid && s_map[p] == s) s_buf[16u + rel + s_before[s][p]] = (uint8_t)byte_of(w, i);
            if (++p == ws) {
                p = 0u;
                rel += ks;
            }
        }
    }
    __syncthreads();
    if constexpr (KIND == CH_EMIT) {
        if (tid == 0) s_big->full = 0u;  // (every lane has read the chunk before's; this chunk's is written behind two more barriers)
    }
    // ---- RLE (simple_rle_compress :557-582) of the chunk's stream bytes, 16 per
    // lane.  A stream byte that differs from the one before it starts a run; every
    // run start closes the run before it, which began at the last run start so far
    // (a max-scan over the lanes, carried across chunks) and emits ceil(L / 255)
    // pairs: 255, ..., 255, remainder.  An add-scan of the pair counts places them.
    const uint32_t q0 = 16u * tid;
    const uint32_t m = q0 >= Lc ? 0u : (Lc - q0 >= 16u ? 16u : Lc - q0);
    const uint4 xv = *reinterpret_cast<const uint4 *>(s_buf + 16u + q0);
    const uint32_t x[4] = {xv.x, xv.y, xv.z, xv.w};
    const uint32_t prev = s_buf[15u + q0];
    if (Lc) c.lastb = s_buf[15u + Lc];
    uint32_t sm = neq_prev_mask4(x[0], prev << 24) | (neq_prev_mask4(x[1], x[0]) << 4) |
                  (neq_prev_mask4(x[2], x[1]) << 8) | (neq_prev_mask4(x[3], x[2]) << 12);
    if (B + q0 == 0u) sm |= 1u;  // the stream's first byte
    sm &= (1u << m) - 1u;
    uint32_t vmax[1] = {sm ? B + q0 + (31u - (uint32_t)__builtin_clz(sm)) + 1u : 0u}, tmax[1];
    team_excl_scan<kAW, 1, OpMax>(vmax, tmax, s_slots[0]);
    const uint32_t cur = vmax[0] > c.cstart ? vmax[0] : c.cstart;  // run start + 1 entering this lane
    // only a lane's first run start can close a run longer than its 16 bytes
    uint32_t first_full = 0u, first_rem = 0u, np = 0u;
    if (sm) {
        const uint32_t qf = B + q0 + (uint32_t)__builtin_ctz(sm);
        np = (uint32_t)__builtin_popcount(sm);
        if (KIND == CH_COUNT ? cur == 0u : qf == 0u) {
            --np;  // nothing before the stream's first byte (the count pass: nothing known before the tile's first start)
            if constexpr (KIND == CH_COUNT) *s_first = qf + 1u;
        } else {
            const uint32_t Lr = qf - (cur - 1u);
            first_full = (Lr - 1u) / 255u;
            first_rem = Lr - 255u * first_full;
            np += first_full;
        }
    }
    uint32_t vadd[1] = {np}, tadd[1];
    team_excl_scan<kAW, 1, OpAdd>(vadd, tadd, s_slots[1]);
    if constexpr (KIND != CH_COUNT) {
        if (sm) {
            uint64_t po = dpos + 2ull * (c.cpairs + vadd[0]);
            uint32_t rs = cur;  // start + 1 of the run being closed
            bool first = true;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (!((sm >> i) & 1u)) continue;
                const uint32_t q = B + q0 + (uint32_t)i;
                const uint32_t val = i ? byte_of(x, i - 1) : prev;
                if (q != 0u) {
                    uint32_t cnt = q - (rs - 1u);
                    if (first) {
                        if (KIND == CH_EMIT && first_full > kAnyLaneFull) {
                            s_big->po = po;
                            s_big->val = val;
                            s_big->full = first_full;
                            po += 2ull * first_full;
                        } else {
                            for (uint32_t f = 0; f < first_full; ++f) {
                                put8(po, 255u);
                                put8(po + 1, val);
                                po += 2;
                            }
                        }
                        cnt = first_rem;
                    }
                    put8(po, cnt);
                    put8(po + 1, val);
                    po += 2;
                }
                first = false;
                rs = q + 1u;
            }
        }
    }
    if constexpr (KIND == CH_EMIT) {
        __syncthreads();
        const uint32_t full = s_big->full;
        if (full) {  // (uniform) a run longer than a chunk: its 255-count pairs by every lane
            const uint64_t po = s_big->po;
            const uint32_t val = s_big->val;
            for (uint32_t f = tid; f < full; f += kAnyTeam) {
                put8(po + 2ull * f, 255u);
                put8(po + 2ull * f + 1, val);
            }
        }
    }
    c.cstart = tmax[0] > c.cstart ? tmax[0] : c.cstart;
    c.cpairs += tadd[0];
    if (tid == 0 && Lc) s_buf[15] = (uint8_t)c.lastb;  // (only lane 0 reads it)
}

// The entropy of one byte position (calculate_entropy :470-480): the exact chain only.  Lane l of
// a wave holds the counts of bins l, l + 64, l + 128, l + 192 and computes their (-prob, log2 prob)
// (0, 0 for an empty bin: fma(0, 0, e) == e for the non-negative running sum), then every lane
// runs the chain over the bins in order 0..255.
__device__ __forceinline__ double any_entropy(const uint32_t (&c)[4], double total) {
    double np[4], L[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        np[k] = 0.0;
        L[k] = 0.0;
        if (c[k]) {
            const double prob = (double)c[k] / total;
            L[k] = psy_log2_glibc(prob, c_log2_tab, c_log2_tab2);
            np[k] = -prob;
        }
    }
    double e = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int l = 0; l < 64; ++l) e = __builtin_fma(readlane_f64(np[k], l), readlane_f64(L[k], l), e);
    return e;
}

// ---------------------------------------------------------------------------------------
// Encode.  HP: histogram positions held in LDS (>= ws; 1 for MODE_MAPPED, which has none).
// MODE_SIZES: the size pass — the same analysis, mapping and split + RLE loop of both streams with
// every store to the blob compiled out (stream 0's pair count places stream 1, so there is no
// separate count to stop at); the length goes to out_len, and there is no slot.
// mark (null: none): a non-zero word = the message belongs to the tile pipeline below.
template <int MODE, int HP, bool PAIR = false>
__global__ __launch_bounds__(kAnyTeam) void tdt_encode_any_kernel(EncodeArgs a, uint32_t ws, const uint32_t *mark) {
    __shared__ uint32_t s_hist[HP * 256];
    __shared__ double s_ent[kAnyWsMax];
    __shared__ uint32_t s_map[kAnyWsMax];           // mapping[b] in {0, 1}
    __shared__ uint32_t s_before[2][kAnyWsMax + 1]; // positions < p mapped to stream s
    __shared__ __attribute__((aligned(16))) uint8_t s_buf[16 + kAnyChunk + 16];  // [15]: the byte before the chunk
    __shared__ uint32_t s_slots[2][kAW];
    __shared__ uint32_t s_bad;

    const uint32_t tid = threadIdx.x, lane = (uint32_t)lane_id(), wv = tid >> 6;
    const uint32_t msg = blockIdx.x;
    if (msg >= a.n_msgs) return;
    if (mark && mark[msg]) return;  // (uniform) a long message: the tile pipeline's
    const uint64_t off0 = a.in_off[table_at<PAIR>(msg, 0)];
    // (a mixed-width batch: this message belongs to another width's pipeline — nothing is touched)
    if (PAIR && pair_absent(off0, a.in_off[table_at<PAIR>(msg, 1)])) return;
    const uint64_t n = a.in_off[table_at<PAIR>(msg, 1)] - off0;
    const uint8_t *base = a.in + off0;
    const uint8_t *lim = base + n;

    bool compress;
    if constexpr (MODE == MODE_ANALYZE) {
        compress = n > 0 && n % ws == 0 && n < (1ull << 32);
        if (!compress) {
            if (tid == 0 && a.status) a.status[msg] = ST_ARG;
            return;
        }
    } else {
        // should_transform :186-201, then compress_tdt's size guard :364-367 (→ the UNCP fallback)
        compress = a.policy_on && n >= a.min_tensor && (n % 4 == 0) && n >= 64 && (n % ws == 0) && n > 0 &&
                   n < (1ull << 32);
    }
    uint64_t slot_b = 0, cap = 0;
    if constexpr (MODE == MODE_SIZES) {
        if (!compress) {
            if (tid == 0) {
                if (a.status) a.status[msg] = ST_OK;
                if (a.out_len) a.out_len[msg] = n + 4;
            }
            return;
        }
    } else if constexpr (MODE != MODE_ANALYZE) {
        slot_b = a.slot_off[table_at<PAIR>(msg, 0)];
        cap = a.slot_off[table_at<PAIR>(msg, 1)] - slot_b;
        if (!compress) {
            const uint64_t E = n + 4;
            const bool fits = E <= cap;
            if (tid == 0) {
                if (a.status) a.status[msg] = fits ? ST_OK : ST_CAPACITY;
                if (a.out_len) a.out_len[msg] = fits ? E : 0;
            }
            if (fits) {
                uint8_t *dst = a.out + slot_b;
                if (tid < 4) dst[tid] = (uint8_t)(kMagicUNCP >> (8 * tid));
                team_copy_g2g<kAnyTeam>(dst + 4, base, n);
            }
            return;
        }
    }
    const uint32_t n32 = (uint32_t)n, wc = n32 / ws;

    if constexpr (MODE == MODE_MAPPED) {
        if (tid == 0) s_bad = 0u;
        __syncthreads();
        if constexpr (PAIR) {
            // scattered batches: one u64 of mapping bits per message; a bit at or above ws is a bad mapping
            const uint64_t bits = reinterpret_cast<const uint64_t *>(a.mapping_in)[msg];
            if (tid == 0 && !mapbits_ok(bits, (int)ws)) s_bad = 1u;
            if (tid < ws) s_map[tid] = mapbits_at(bits, (int)tid);
        } else if (tid < ws) {
            const int32_t m = a.mapping_in[(uint64_t)msg * ws + tid];
            if (m < 0 || m > 1) s_bad = 1u;
            s_map[tid] = (uint32_t)(m & 1);
        }
        __syncthreads();
        if (s_bad) {  // invalid caller mapping: an empty output for this message
            if (tid == 0) {
                if (a.out_len) a.out_len[msg] = 0;
                if (a.status) a.status[msg] = ST_BAD_MAPPING;
            }
            return;
        }
    } else {
        // ---- histograms (extract_features :441-446, every word): byte j counts at position j mod ws
        for (uint32_t i = tid; i < ws * 256u; i += kAnyTeam) s_hist[i] = 0u;
        __syncthreads();
        {
            const uint32_t step = kAnyChunk % ws;
            uint32_t p0 = (16u * tid) % ws;
            for (uint64_t j0 = 16ull * tid; j0 < n; j0 += kAnyChunk) {
                const int valid = n - j0 >= 16 ? 16 : (int)(n - j0);
                const uint4 v = ld16_msg(base + j0, valid, base, lim);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                uint32_t p = p0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (i < valid) atomicAdd(&s_hist[p * 256u + byte_of(w, i)], 1u);
                    p = p + 1u == ws ? 0u : p + 1u;
                }
                p0 += step;
                if (p0 >= ws) p0 -= ws;
            }
        }
        __syncthreads();
        // ---- entropies (any_entropy): a wave takes one position at a time
        const double total = (double)wc;
        for (uint32_t b = wv; b < ws; b += kAW) {
            uint32_t c[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                c[k] = s_hist[b * 256u + 64u * k + lane];
                if constexpr (MODE == MODE_ANALYZE) {
                    if (a.hist_out) a.hist_out[((uint64_t)msg * ws + b) * 256 + 64u * k + lane] = c[k];
                }
            }
            const double e = any_entropy(c, total);
            if (lane == 0) s_ent[b] = e;
        }
        __syncthreads();
        // ---- mapping (perform_clustering :507-525): entropy > in-order sum / ws
        if (tid == 0) {
            double sum = 0.0;
            for (uint32_t b = 0; b < ws; ++b) sum += s_ent[b];
            const double thr = sum / (double)ws;
            for (uint32_t b = 0; b < ws; ++b) s_map[b] = s_ent[b] > thr ? 1u : 0u;
        }
        __syncthreads();
        if constexpr (MODE == MODE_ANALYZE) {
            if (tid < ws) {
                if (a.ent_out) a.ent_out[(uint64_t)msg * ws + tid] = s_ent[tid];
                if (a.map_out) a.map_out[(uint64_t)msg * ws + tid] = (int32_t)s_map[tid];
            }
            if (tid == 0 && a.status) a.status[msg] = ST_OK;
            return;
        }
    }

    if constexpr (MODE != MODE_ANALYZE) {
        // ---- stream layout: s_before[s][p] = positions below p mapped to stream s
        if (tid == 0) {
            uint32_t k[2] = {0u, 0u};
            for (uint32_t p = 0; p < ws; ++p) {
                s_before[0][p] = k[0];
                s_before[1][p] = k[1];
                k[s_map[p]]++;
            }
            s_before[0][ws] = k[0];
            s_before[1][ws] = k[1];
            s_buf[15] = 0;
        }
        __syncthreads();
        const uint32_t ns = s_before[1][ws] ? 2u : 1u;  // separate_byte_streams :527-549: max(mapping) + 1
        uint8_t *dst = a.out + slot_b;
        // every store is bounded by the slot: a blob that does not fit is reported, not written past it
        auto put8 = [&](uint64_t o, uint32_t v) __attribute__((always_inline)) {
            if constexpr (MODE == MODE_SIZES) return;  // (the size pass writes no blob byte)
            if (o < cap) dst[o] = (uint8_t)v;
        };
        auto put32 = [&](uint64_t o, uint32_t v) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) put8(o + i, v >> (8 * i));
        };
        // ---- header (serialize :81-117): magic, original size, streams, word size, mapping
        if (tid == 0) {
            put32(0, kMagicTDT);
            put32(4, n32);
            put32(8, ns);
            put32(12, ws);
            put32(16, ws);
        }
        if (tid < ws) put32(20 + 4ull * tid, s_map[tid]);
        uint64_t o = 20 + 4ull * ws;  // the next stream's length word

        for (uint32_t s = 0; s < ns; ++s) {
            const uint32_t ks = s_before[s][ws];
            const uint64_t dpos = o + 4;  // the stream's pairs
            AnyRunCarry c{0u, 0u, 0u};  // carries across chunks (uniform)
            if (ks) {
                for (uint64_t cb64 = 0; cb64 < n; cb64 += kAnyChunk)  // (n < 2^32; cb + 4096 may not be)
                    any_chunk<CH_ENCODE>(base, lim, n, ws, s, ks, dpos, cb64, s_map, s_before, s_buf, s_slots, c, put8,
                                         nullptr, nullptr);
                // the last run closes at the end of the stream
                const uint32_t S = wc * ks;
                const uint32_t Lr = S - (c.cstart - 1u);
                const uint32_t full = (Lr - 1u) / 255u;
                if (tid == 0) {
                    uint64_t po = dpos + 2ull * c.cpairs;
                    for (uint32_t f = 0; f < full; ++f) {
                        put8(po, 255u);
                        put8(po + 1, c.lastb);
                        po += 2;
                    }
                    put8(po, Lr - 255u * full);
                    put8(po + 1, c.lastb);
                    s_buf[15] = 0;
                }
                c.cpairs += full + 1u;
                __syncthreads();  // the next stream's chunks reuse s_buf
            }
            const uint32_t cpairs = c.cpairs;
            if (tid == 0) put32(o, 2u * cpairs);
            o = dpos + 2ull * cpairs;
        }
        const bool fits = MODE == MODE_SIZES || o <= cap;
        if (tid == 0) {
            if (a.status) a.status[msg] = fits ? ST_OK : ST_CAPACITY;
            if (a.out_len) a.out_len[msg] = fits ? o : 0;
            if constexpr (MODE == MODE_SIZES) {
                if (a.map_out) {  // (tdt_mappings_v: the mapping bits beside the size)
                    uint64_t bits = 0;
                    for (uint32_t p = 0; p < ws; ++p) bits |= (uint64_t)s_map[p] << p;
                    reinterpret_cast<uint64_t *>(a.map_out)[msg] = bits;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// The tiled encode of long messages (tdt_anyws.h).  Every kernel below but the plan runs a fixed
// grid striding over the records the plan claimed; their counts stay in device memory.

// the records in use: what the plan claimed, within the budgets it ran with
__device__ __forceinline__ uint32_t any_claimed(const AnyTiledArgs &t, AnyCount k, uint32_t cap) {
    const unsigned long long c = t.cnt[k];
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(c < cap ? (uint32_t)c : cap));
}
// The message of tile record e among the nl large records of this launch's width — each owns the
// records [tile0, tile0 + ntiles) it claimed — and the tile's index in it; null: a hole left by a
// failed claim, or another width's.  Every wave of the workgroup searches alike, 64 records a step
// (one plan lane writing a long message's thousands of tile entries took 115 us of a 1.6 ms call).
__device__ __forceinline__ const AnyLarge *any_tile_owner(const AnyTiledArgs &t, uint32_t nl, uint32_t e, uint32_t ws,
                                                          uint32_t &tile) {
    const uint32_t lane = (uint32_t)lane_id();
    for (uint32_t L0 = 0; L0 < nl; L0 += 64u) {  // (uniform)
        const uint32_t L = L0 + lane;
        bool hit = false;
        if (L < nl) {
            const AnyLarge &g = t.large[L];
            hit = g.ws == ws && e - g.tile0 < g.ntiles;
        }
        const uint64_t m = __ballot(hit);
        if (m) {
            const AnyLarge *g = t.large + L0 + (uint32_t)__builtin_ctzll(m);
            tile = e - (uint32_t)__builtin_amdgcn_readfirstlane((int)g->tile0);
            return g;
        }
    }
    return nullptr;
}

// ---- plan: one lane per message
template <bool PAIR>
__global__ __launch_bounds__(256) void tdt_any_plan_kernel(EncodeArgs a, AnyTiledArgs t, uint32_t ws, int mode) {
    const uint32_t msg = blockIdx.x * 256u + threadIdx.x;
    if (msg >= a.n_msgs) return;
    uint32_t mark = 0u;
    const uint64_t off0 = a.in_off[table_at<PAIR>(msg, 0)], off1 = a.in_off[table_at<PAIR>(msg, 1)];
    // the tiled path's threshold, as the tuned plan's (tdt_encode_plan_kernel)
    const uint64_t share = (PAIR ? t.cnt[t.bytes_at] : a.in_off[a.n_msgs] - a.in_off[0]) / 4096;
    const uint64_t thr = share > t.large_min ? share : t.large_min;
    const uint64_t n = off1 - off0;
    // (a message of 4 GiB or more stays where it is: UNCP on one workgroup)
    if (!(PAIR && pair_absent(off0, off1)) && n > thr && n < (1ull << 32)) {
        const bool sizes = mode == MODE_SIZES;
        const bool compress = a.policy_on && n >= a.min_tensor && (n % 4 == 0) && n >= 64 && (n % ws == 0);
        uint64_t bits = 0;
        bool bad = false;
        if (compress && mode == MODE_MAPPED) {
            if constexpr (PAIR) {
                bits = reinterpret_cast<const uint64_t *>(a.mapping_in)[msg];
                bad = !mapbits_ok(bits, (int)ws);
            } else {
                for (uint32_t p = 0; p < ws; ++p) {
                    const int32_t m = a.mapping_in[(uint64_t)msg * ws + p];
                    bad = bad || m < 0 || m > 1;
                    bits |= (uint64_t)(m & 1) << p;
                }
            }
        }
        uint64_t slot_b = 0, cap = ~0ull;
        if (!sizes) {
            slot_b = a.slot_off[table_at<PAIR>(msg, 0)];
            cap = a.slot_off[table_at<PAIR>(msg, 1)] - slot_b;
        }
        bool claim = !bad;  // (an invalid mapping: the one-workgroup kernel reports it)
        if (!compress) {
            if (sizes || n + 4 > cap) {  // nothing to copy: the passthrough's length, or a slot too small for it
                const bool fits = n + 4 <= cap;
                if (a.status) a.status[msg] = fits ? ST_OK : ST_CAPACITY;
                if (a.out_len) a.out_len[msg] = fits ? n + 4 : 0;
                claim = false;
                mark = 1u;
            }
        }
        if (claim) {
            const uint32_t nt = (uint32_t)((n + kAnyTile - 1) / kAnyTile);
            const unsigned long long L = atomicAdd(t.cnt + AC_LARGE, 1ull);
            const unsigned long long T = atomicAdd(t.cnt + AC_TILES, (unsigned long long)nt);
            if (L < t.lcap && T + nt <= t.tcap) {
                AnyLarge g{};
                g.src = a.in + off0;
                g.dst = sizes ? nullptr : a.out + slot_b;
                g.cap = cap;
                g.mapbits = bits;
                g.msg = msg;
                g.n = (uint32_t)n;
                g.ws = ws;
                g.flags = compress ? 0u : kAnyUncp;
                g.tile0 = (uint32_t)T;
                g.ntiles = nt;
                t.large[L] = g;  // (its tile records [T, T + nt) are found through it: any_tile_owner)
                if (!compress) {  // the passthrough blob's marker, length and status; its tiles copy the payload
                    if (a.status) a.status[msg] = ST_OK;
                    if (a.out_len) a.out_len[msg] = n + 4;
#pragma unroll
                    for (int i = 0; i < 4; ++i) g.dst[i] = (uint8_t)(kMagicUNCP >> (8 * i));
                }
                mark = 1u;
            } else if (L < t.lcap) {  // a budget is spent: the one-workgroup kernel keeps the message
                AnyLarge g{};
                t.large[L] = g;  // (ws 0, no tiles: no launch's record)
            }
        }
    }
    t.mark[msg] = mark;
}

// ---- histograms: ws x 256 counts of the tiles of kAnySpanTiles records, added to their message's.
// kAnyHistTeam lanes: a span is one workgroup's serial walk, and a 256 MiB message has 512 of them
// on 256 CUs — two 4-wave workgroups a CU left the LDS atomics' latency uncovered
constexpr uint32_t kAnyHistTeam = 1024;
template <int HP>
__global__ __launch_bounds__(kAnyHistTeam) void tdt_any_hist_kernel(AnyTiledArgs t, uint32_t ws) {
    __shared__ uint32_t s_hist[HP * 256];
    const uint32_t tid = threadIdx.x;
    const uint32_t nt = any_claimed(t, AC_TILES, t.tcap), nl = any_claimed(t, AC_LARGE, t.lcap);
    for (uint32_t i = tid; i < ws * 256u; i += kAnyHistTeam) s_hist[i] = 0u;
    __syncthreads();
    // the LDS counts → the message's histogram (integer adds: any order gives the same counts)
    auto flush = [&](const AnyLarge *g) __attribute__((always_inline)) {
        __syncthreads();
        uint32_t *h = t.hist + (size_t)(g - t.large) * (kAnyWsMax * 256);
        for (uint32_t i = tid; i < ws * 256u; i += kAnyHistTeam) {
            const uint32_t c = s_hist[i];
            if (c) {
                atomicAdd(h + i, c);
                s_hist[i] = 0u;
            }
        }
        __syncthreads();
    };
    constexpr uint32_t kStride = 16u * kAnyHistTeam;  // message bytes per step of the workgroup
    for (uint32_t e0 = blockIdx.x * kAnySpanTiles; e0 < nt; e0 += gridDim.x * kAnySpanTiles) {
        const AnyLarge *cur = nullptr;
        for (uint32_t e = e0; e < nt && e < e0 + kAnySpanTiles; ++e) {  // (uniform)
            uint32_t tt = 0;
            const AnyLarge *g = any_tile_owner(t, nl, e, ws, tt);
            if (g && (g->flags & kAnyUncp)) g = nullptr;
            if (g != cur) {
                if (cur) flush(cur);
                cur = g;
            }
            if (!g) continue;
            const uint8_t *base = g->src;
            const uint64_t n = g->n;
            const uint64_t jb = (uint64_t)tt * kAnyTile, je = n - jb < kAnyTile ? n : jb + kAnyTile;
            // byte j counts at position j mod ws
            const uint32_t step = kStride % ws;
            uint32_t p0 = (uint32_t)((jb + 16ull * tid) % ws);
            for (uint64_t j0 = jb + 16ull * tid; j0 < je; j0 += kStride) {
                const int valid = je - j0 >= 16 ? 16 : (int)(je - j0);
                const uint4 v = ld16_msg(base + j0, valid, base, base + n);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                uint32_t p = p0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (i < valid) atomicAdd(&s_hist[p * 256u + byte_of(w, i)], 1u);
                    p = p + 1u == ws ? 0u : p + 1u;
                }
                p0 += step;
                if (p0 >= ws) p0 -= ws;
            }
        }
        if (cur) flush(cur);
    }
}

// ---- mapping: the one-workgroup kernel's entropies and threshold over a large message's histogram
__global__ __launch_bounds__(kAnyTeam) void tdt_any_map_kernel(AnyTiledArgs t, uint32_t ws) {
    __shared__ double s_ent[kAnyWsMax];
    const uint32_t tid = threadIdx.x, lane = (uint32_t)lane_id(), wv = tid >> 6;
    const uint32_t nl = any_claimed(t, AC_LARGE, t.lcap);
    for (uint32_t L = blockIdx.x; L < nl; L += gridDim.x) {
        AnyLarge *g = t.large + L;
        if ((uint32_t)__builtin_amdgcn_readfirstlane((int)g->ws) != ws || (g->flags & kAnyUncp)) continue;  // (uniform)
        uint32_t *h = t.hist + (size_t)L * (kAnyWsMax * 256);
        const double total = (double)(g->n / ws);
        for (uint32_t b = wv; b < ws; b += kAW) {
            uint32_t c[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                c[k] = h[b * 256u + 64u * k + lane];
                h[b * 256u + 64u * k + lane] = 0u;  // (all zero again for the next call)
            }
            const double e = any_entropy(c, total);
            if (lane == 0) s_ent[b] = e;
        }
        __syncthreads();
        // perform_clustering :507-525: entropy > in-order sum / ws
        if (tid == 0) {
            double sum = 0.0;
            for (uint32_t b = 0; b < ws; ++b) sum += s_ent[b];
            const double thr = sum / (double)ws;
            uint64_t bits = 0;
            for (uint32_t b = 0; b < ws; ++b) bits |= (uint64_t)(s_ent[b] > thr ? 1u : 0u) << b;
            g->mapbits = bits;
        }
        __syncthreads();
    }
}

// ---- count (EMIT false) and emit (EMIT true): the chunks of one tile, stream after stream
template <bool EMIT>
__global__ __launch_bounds__(kAnyTeam) void tdt_any_tile_kernel(AnyTiledArgs t, uint32_t ws) {
    __shared__ uint32_t s_map[kAnyWsMax];
    __shared__ uint32_t s_before[2][kAnyWsMax + 1];
    __shared__ __attribute__((aligned(16))) uint8_t s_buf[16 + kAnyChunk + 16];
    __shared__ uint32_t s_slots[2][kAW];
    __shared__ uint32_t s_first;
    __shared__ AnyBigRun s_big;
    const uint32_t tid = threadIdx.x;
    const uint32_t nt = any_claimed(t, AC_TILES, t.tcap), nl = any_claimed(t, AC_LARGE, t.lcap);
    for (uint32_t e = blockIdx.x; e < nt; e += gridDim.x) {  // (uniform)
        AnyTile &r = t.tiles[e];
        uint32_t tt = 0;
        const AnyLarge *g = any_tile_owner(t, nl, e, ws, tt);
        if (!g) continue;
        const uint8_t *base = g->src;
        const uint64_t n = g->n;
        const uint64_t jb = (uint64_t)tt * kAnyTile, je = n - jb < kAnyTile ? n : jb + kAnyTile;
        if (g->flags & kAnyUncp) {  // a passthrough message: the tile's payload bytes behind the marker
            if constexpr (EMIT) copy_shifted<1, false>(g->dst + 4 + jb, base + jb, je - jb, tid, kAnyTeam);
            continue;
        }
        if (EMIT && !g->ok) continue;  // the blob does not fit its slot: nothing is written
        const uint64_t bits = g->mapbits;
        __syncthreads();  // (the tile before is done with the arrays)
        if (tid < ws) s_map[tid] = mapbits_at(bits, (int)tid);
        if (tid <= ws) {
            s_before[0][tid] = any_before(bits, 0u, tid);
            s_before[1][tid] = any_before(bits, 1u, tid);
        }
        __syncthreads();
        const uint32_t ns = s_before[1][ws] ? 2u : 1u;
        uint8_t *dst = g->dst;
        const uint64_t cap = g->cap;
        auto put8 = [&](uint64_t o, uint32_t v) __attribute__((always_inline)) {
            if (o < cap) dst[o] = (uint8_t)v;  // (every store is bounded by the slot)
        };
        for (uint32_t s = 0; s < ns; ++s) {
            const uint32_t ks = s_before[s][ws];
            if (!ks) continue;  // (an empty stream 0: its length word is the scan's)
            // the stream's pairs: behind the header, the mapping and the length word(s); stream 0's total places stream 1
            const uint64_t dpos = 20 + 4ull * ws + 4 + (s ? 2ull * g->pairs[0] + 4 : 0ull);
            const AnyRange R = any_tile_range((uint32_t)jb, (uint32_t)je, ws, bits, s);
            // the stream byte before the tile's first: at most ws message bytes back
            const uint32_t pb = R.b ? base[any_pred_pos((uint32_t)jb, ws, bits, s)] : 0u;
            AnyRunCarry c{EMIT ? r.carry[s] : 0u, EMIT ? r.base[s] : 0u, pb};
            if (tid == 0) {
                s_buf[15] = (uint8_t)pb;
                s_first = 0u;
            }
            __syncthreads();
            for (uint64_t cb64 = jb; cb64 < je; cb64 += kAnyChunk)
                any_chunk<EMIT ? CH_EMIT : CH_COUNT>(base, base + n, n, ws, s, ks, dpos, cb64, s_map, s_before, s_buf, s_slots, c,
                                                     put8, &s_first, &s_big);
            __syncthreads();  // (s_first is written; the next stream's chunks reuse s_buf)
            if constexpr (!EMIT) {
                if (tid == 0) {
                    r.first[s] = s_first;
                    r.last[s] = c.cstart;
                    r.inner[s] = c.cpairs;
                }
            } else if (tt + 1u == g->ntiles) {  // the stream's last tile: the run that closes at the stream's end
                const uint32_t S = (g->n / ws) * ks;
                const uint32_t Lr = S - (c.cstart - 1u);
                const uint32_t full = (Lr - 1u) / 255u;
                const uint64_t po = dpos + 2ull * c.cpairs;
                for (uint32_t f = tid; f < full; f += kAnyTeam) {
                    put8(po + 2ull * f, 255u);
                    put8(po + 2ull * f + 1, c.lastb);
                }
                if (tid == 0) {
                    put8(po + 2ull * full, Lr - 255u * full);
                    put8(po + 2ull * full + 1, c.lastb);
                }
            }
        }
    }
}

// ---- scan: one workgroup per large message over its tile records; the blob's fixed words
__global__ __launch_bounds__(kAnyTeam) void tdt_any_scan_kernel(EncodeArgs a, AnyTiledArgs t, uint32_t ws, int mode) {
    __shared__ uint32_t s_slots[2][2 * kAW];
    const uint32_t tid = threadIdx.x;
    const uint32_t nl = any_claimed(t, AC_LARGE, t.lcap);
    for (uint32_t L = blockIdx.x; L < nl; L += gridDim.x) {
        AnyLarge *g = t.large + L;
        if ((uint32_t)__builtin_amdgcn_readfirstlane((int)g->ws) != ws || (g->flags & kAnyUncp)) continue;  // (uniform)
        const uint64_t bits = g->mapbits;
        const uint32_t n32 = g->n, wc = n32 / ws, nt = g->ntiles;
        const uint32_t k[2] = {any_before(bits, 0u, ws), any_before(bits, 1u, ws)};
        const uint32_t ns = k[1] ? 2u : 1u;
        AnyTile *tiles = t.tiles + g->tile0;
        uint32_t carry[2] = {0u, 0u}, base[2] = {0u, 0u};  // (uniform) behind the tiles so far
        for (uint32_t i0 = 0; i0 < nt; i0 += kAnyTeam) {
            const uint32_t i = i0 + tid;
            AnyTileRuns runs[2] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
            if (i < nt) {
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    if ((uint32_t)s < ns && k[s]) runs[s] = AnyTileRuns{tiles[i].first[s], tiles[i].last[s], tiles[i].inner[s]};
            }
            uint32_t vmax[2] = {runs[0].last, runs[1].last}, tmax[2];
            team_excl_scan<kAW, 2, OpMax>(vmax, tmax, s_slots[0]);
            uint32_t vadd[2], tadd[2], cin[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                cin[s] = vmax[s] > carry[s] ? vmax[s] : carry[s];
                vadd[s] = any_tile_pairs(runs[s], cin[s]);
            }
            team_excl_scan<kAW, 2, OpAdd>(vadd, tadd, s_slots[1]);
            if (i < nt) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    tiles[i].carry[s] = cin[s];
                    tiles[i].base[s] = base[s] + vadd[s];
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                carry[s] = tmax[s] > carry[s] ? tmax[s] : carry[s];
                base[s] += tadd[s];
            }
        }
        // the run that closes at either stream's end; stream 0's total places stream 1
        uint32_t pairs[2] = {0u, 0u};
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if ((uint32_t)s < ns && k[s]) pairs[s] = base[s] + any_final_pairs(wc * k[s], carry[s]);
        const bool sizes = mode == MODE_SIZES;
        uint8_t *dst = g->dst;
        const uint64_t cap = g->cap;
        auto put32 = [&](uint64_t o, uint32_t v) __attribute__((always_inline)) {
            if (sizes) return;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (o + i < cap) dst[o + i] = (uint8_t)(v >> (8 * i));
        };
        const uint64_t o0 = 20 + 4ull * ws, o1 = o0 + 4 + 2ull * pairs[0];
        const uint64_t o = ns == 2u ? o1 + 4 + 2ull * pairs[1] : o1;
        const bool fits = sizes || o <= cap;
        // header (serialize :81-117): magic, original size, streams, word size, mapping; the length words
        if (tid < ws) put32(20 + 4ull * tid, mapbits_at(bits, (int)tid));
        if (tid == 0) {
            put32(0, kMagicTDT);
            put32(4, n32);
            put32(8, ns);
            put32(12, ws);
            put32(16, ws);
            put32(o0, 2u * pairs[0]);
            if (ns == 2u) put32(o1, 2u * pairs[1]);
            g->pairs[0] = pairs[0];
            g->pairs[1] = pairs[1];
            g->ok = fits ? 1u : 0u;
            const uint32_t msg = g->msg;
            if (a.status) a.status[msg] = fits ? ST_OK : ST_CAPACITY;
            if (a.out_len) a.out_len[msg] = fits ? o : 0;
            if (sizes && a.map_out) reinterpret_cast<uint64_t *>(a.map_out)[msg] = bits;  // (tdt_mappings_v)
        }
        __syncthreads();  // (the slots of the next message's scans)
    }
}

// ---------------------------------------------------------------------------------------
// Decode of the deferred blobs.  blob_check (tdt_decode.h) has passed each of them: header,
// mapping (>= ws entries, each < num_streams) and stream table lie inside the blob, 1 <= ws <= 64
// and at least one whole word.  Every output byte is written exactly once: by the pair that
// covers it, or as zero (a stream shorter than its share of the words, the bytes past the
// last whole word: recombine_byte_streams :614-637 over its zero-initialised result).
// mark (null: none): a non-zero word = the list entry belongs to the decode tile pipeline below.
// seen (null: none): pinned memory for the next call's host — the length of the last list that was not empty.
template <bool PAIR = false>
__global__ __launch_bounds__(kAnyTeam) void tdt_decode_any_kernel(DecodeArgs a, const uint32_t *mark, uint32_t *seen) {
    __shared__ uint32_t s_map[kAnyWsMax], s_soff[kAnyWsMax], s_slen[kAnyWsMax], s_ptab[kAnyWsMax];
    __shared__ uint32_t s_slots[2][kAW];
    const uint32_t tid = threadIdx.x, lane = (uint32_t)lane_id();
    const uint32_t listed = __builtin_amdgcn_readfirstlane(*a.dcount);
    const uint32_t cnt = listed < a.n_msgs ? listed : a.n_msgs;
    // (sticky: a context that has listed a blob once keeps its plan; an unknown word (~0) takes the first length)
    if (seen && blockIdx.x == 0 && tid == 0 && (listed || *seen == ~0u)) *seen = listed;
    for (uint32_t it = blockIdx.x; it < cnt; it += gridDim.x) {
        if (it != blockIdx.x) __syncthreads();
        if (mark && mark[it]) continue;  // (uniform) a long blob: the tile pipeline's
        const uint32_t msg = a.dlist[it];
        const uint64_t boff = a.in_off[msg];
        const uint64_t len = a.in_len ? a.in_len[msg] : a.in_off[msg + 1] - boff;
        const uint8_t *blob = a.in + boff;
        const uint8_t *blim = blob + len;
        const uint32_t orig = ld_u32_bytes(blob + 4), ns = ld_u32_bytes(blob + 8), ws = ld_u32_bytes(blob + 12),
                       msize = ld_u32_bytes(blob + 16);
        uint64_t ob;
        bool fits;
        if (a.slot_off) {
            ob = a.slot_off[table_at<PAIR>(msg, 0)];
            fits = orig <= a.slot_off[table_at<PAIR>(msg, 1)] - ob;
        } else {
            ob = a.out_off[msg];  // (the look-back kernel placed it)
            fits = ob + orig <= a.out_cap;
        }
        if (tid == 0) {
            if (a.status) a.status[msg] = fits ? ST_OK : ST_CAPACITY;
            if (a.slot_off && a.out_len) a.out_len[msg] = fits ? orig : 0;
        }
        if (!fits || ws == 0u || ws > (uint32_t)kAnyWsMax) continue;  // (the width: blob_check's, restated)
        uint8_t *dst = a.out + ob;
        // mapping and stream table: lane b of wave 0 keeps position b's stream
        if (tid < 64) {
            const uint32_t mp = lane < ws ? ld_u32_bytes(blob + 20 + 4 * lane) : 0xffffffffu;
            uint64_t off = 20 + 4ull * msize;
            uint32_t my_off = 0, my_len = 0;
            for (uint32_t s = 0; s < ns; ++s) {  // uniform
                const uint32_t sl = ld_u32_bytes(blob + off);
                off += 4;
                if (mp == s) {
                    my_off = (uint32_t)off;
                    my_len = sl;
                }
                off += sl;
            }
            if (lane < ws) {
                s_map[lane] = mp;
                s_soff[lane] = my_off;
                s_slen[lane] = my_len;
            }
        }
        __syncthreads();
        const uint32_t wc = orig / ws, wbytes = wc * ws;
        for (uint32_t k = wbytes + tid; k < orig; k += kAnyTeam) dst[k] = 0;
        uint32_t alt = 0u;
        for (uint32_t b0 = 0; b0 < ws; ++b0) {  // every referenced stream once, at its first position
            const uint32_t s = s_map[b0];
            bool seen = false;
            for (uint32_t bb = 0; bb < b0; ++bb) seen = seen || s_map[bb] == s;
            if (seen) continue;  // uniform
            // the stream's positions in word order: byte q of the decoded stream is byte
            // s_ptab[q % k] of word q / k
            uint32_t k = 0u, rank = 0u;
            for (uint32_t bb = 0; bb < ws; ++bb) {
                const bool same = s_map[bb] == s;
                k += same ? 1u : 0u;
                rank += same && bb < tid ? 1u : 0u;
            }
            if (tid < ws && s_map[tid] == s) s_ptab[rank] = tid;
            __syncthreads();
            const uint32_t soff = s_soff[b0], np = s_slen[b0] / 2u;  // (an odd trailing byte is ignored :600)
            const uint32_t S = wc * k;                                 // the stream's share of the output
            uint64_t sbase = 0;                                        // decoded bytes before this chunk
            for (uint32_t pc = 0; pc < np && sbase < S; pc += kAnyDecPairs) {
                const uint32_t p0 = pc + 8u * tid;
                const uint32_t nv = p0 < np ? (np - p0 < 8u ? np - p0 : 8u) : 0u;
                const uint4 pv = nv ? ld16_span(blob + soff + 2ull * p0, (int)(2 * nv), blim) : make_uint4(0, 0, 0, 0);
                const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w};
                const uint32_t s2 = (pw[0] & 0x00ff00ffu) + (pw[1] & 0x00ff00ffu) + (pw[2] & 0x00ff00ffu) +
                                    (pw[3] & 0x00ff00ffu);
                uint32_t v[1] = {(s2 & 0xffffu) + (s2 >> 16)}, tot[1];
                const uint32_t mine = v[0];
                team_excl_scan<kAW, 1, OpAdd>(v, tot, s_slots[alt]);
                alt ^= 1u;
                uint64_t q64 = sbase + v[0];
                if (mine && q64 < S) {
                    uint32_t q = (uint32_t)q64;
                    uint32_t w = q / k, t = q - w * k;
                    uint8_t *row = dst + (uint64_t)w * ws;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const uint32_t pr = pw[i >> 1] >> (16 * (i & 1));
                        const uint32_t c = pr & 0xffu;  // (count 0 emits nothing :602)
                        const uint8_t val = (uint8_t)(pr >> 8);
                        for (uint32_t r = 0; r < c && q < S; ++r, ++q) {
                            row[s_ptab[t]] = val;
                            if (++t == k) {
                                t = 0u;
                                row += ws;
                            }
                        }
                    }
                }
                sbase += tot[0];
            }
            // a stream shorter than its share leaves zeros (recombine :626-631)
            for (uint64_t q = sbase + tid; q < S; q += kAnyTeam) {
                const uint32_t w = (uint32_t)q / k, t = (uint32_t)q - w * k;
                dst[(uint64_t)w * ws + s_ptab[t]] = 0;
            }
            __syncthreads();  // s_ptab is rebuilt for the next stream
        }
    }
}

// ---------------------------------------------------------------------------------------
// The tiled decode of long blobs (tdt_anyws.h; the arithmetic: tdt_anyws_dec_tiles.h).  Every
// kernel below but the plan runs a fixed grid striding over what the plan claimed.

// what the plan claimed, within the budgets it ran with
__device__ __forceinline__ uint32_t anyd_claimed(const AnyDecArgs &t, AnyDecCount k, uint32_t cap) {
    const unsigned long long c = t.cnt[k];
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(c < cap ? (uint32_t)c : cap));
}
// The long blob that owns tile (BLOCKS: block sum) e among the nl records — each owns the range it
// claimed — and e's index in that range; null: a hole left by a failed claim.  Every wave searches
// alike, 64 records a step (any_tile_owner).
template <bool BLOCKS>
__device__ __forceinline__ const AnyDecLarge *anyd_owner(const AnyDecArgs &t, uint32_t nl, uint32_t e, uint32_t &idx) {
    const uint32_t lane = (uint32_t)lane_id();
    for (uint32_t L0 = 0; L0 < nl; L0 += 64u) {  // (uniform)
        const uint32_t L = L0 + lane;
        bool hit = false;
        if (L < nl) {
            const AnyDecLarge &g = t.large[L];
            hit = g.ws != 0u && (BLOCKS ? e - g.blk0[0] < g.nb[0] + g.nb[1] : e - g.tile0 < g.ntiles);
        }
        const uint64_t m = __ballot(hit);
        if (m) {
            const AnyDecLarge *g = t.large + L0 + (uint32_t)__builtin_ctzll(m);
            idx = e - (uint32_t)__builtin_amdgcn_readfirstlane((int)(BLOCKS ? g->blk0[0] : g->tile0));
            return g;
        }
    }
    return nullptr;
}

// ---- plan: one lane per entry of the deferred list
template <bool PAIR>
__global__ __launch_bounds__(256) void tdt_anyd_plan_kernel(DecodeArgs a, AnyDecArgs t) {
    const uint32_t listed = *a.dcount;
    const uint32_t cnt = listed < a.n_msgs ? listed : a.n_msgs;
    // the tiled path's threshold, as the tuned plan's (tdt_decode_plan_kernel)
    uint64_t thr = t.large_min;
    if (a.n_msgs) {
        uint64_t bytes;
        if constexpr (PAIR) {
            bytes = *t.batch_bytes;
        } else {  // (the look-back route has no in_len: in_off[n] - in_off[0])
            const uint64_t last = a.in_len ? a.in_off[a.n_msgs - 1] + a.in_len[a.n_msgs - 1] : a.in_off[a.n_msgs];
            bytes = last - a.in_off[0];
        }
        const uint64_t share = bytes / 4096;
        thr = share > thr ? share : thr;
    }
    for (uint32_t it = blockIdx.x * 256u + threadIdx.x; it < cnt; it += gridDim.x * 256u) {
        uint32_t mark = 0u;
        const uint32_t msg = a.dlist[it];
        const uint64_t boff = a.in_off[msg];
        const uint64_t len = a.in_len ? a.in_len[msg] : a.in_off[msg + 1] - boff;
        const uint8_t *blob = a.in + boff;
        // (blob_check has passed: header, mapping and stream table lie inside the blob)
        const uint32_t orig = ld_u32_bytes(blob + 4), ns = ld_u32_bytes(blob + 8), ws = ld_u32_bytes(blob + 12),
                       msize = ld_u32_bytes(blob + 16);
        if (orig > thr && ws != 0u && ws <= (uint32_t)kAnyWsMax) {
            uint64_t ob;
            bool fits;
            if (a.slot_off) {
                ob = a.slot_off[table_at<PAIR>(msg, 0)];
                fits = orig <= a.slot_off[table_at<PAIR>(msg, 1)] - ob;
            } else {
                ob = a.out_off[msg];
                fits = ob + orig <= a.out_cap;
            }
            // the referenced streams: the first is position 0's
            uint32_t id[2] = {0u, 0u}, k[2] = {0u, 0u}, nref = 0u;
            bool many = false;
            for (uint32_t p = 0; p < ws; ++p) {
                const uint32_t m = ld_u32_bytes(blob + 20 + 4 * p);
                if (nref > 0u && m == id[0]) ++k[0];
                else if (nref > 1u && m == id[1]) ++k[1];
                else if (nref < 2u) {
                    id[nref] = m;
                    k[nref++] = 1u;
                } else many = true;
            }
            if (fits && !many) {
                uint32_t soff[2] = {0u, 0u}, np[2] = {0u, 0u};
                uint64_t off = 20 + 4ull * msize;
                for (uint32_t s = 0; s < ns; ++s) {
                    const uint32_t sl = ld_u32_bytes(blob + off);
                    off += 4;
#pragma unroll
                    for (int r = 0; r < 2; ++r)
                        if ((uint32_t)r < nref && id[r] == s) {
                            soff[r] = (uint32_t)off;
                            np[r] = sl / 2u;  // (an odd trailing byte is ignored :600)
                        }
                    off += sl;
                }
                const uint32_t wc = orig / ws, tw = any_dec_tile_words(ws);
                const uint32_t nt = any_dec_ntiles(wc, tw);
                const uint32_t nb[2] = {any_dec_nblocks(np[0]), nref > 1u ? any_dec_nblocks(np[1]) : 0u};
                const unsigned long long L = atomicAdd(t.cnt + ADC_LARGE, 1ull);
                const unsigned long long B = atomicAdd(t.cnt + ADC_BLOCKS, (unsigned long long)nb[0] + nb[1]);
                const unsigned long long T = atomicAdd(t.cnt + ADC_TILES, (unsigned long long)nt);
                if (L < t.lcap && B + nb[0] + nb[1] <= t.bcap && T + nt <= t.tcap) {
                    AnyDecLarge *g = t.large + L;
                    g->blob = blob;
                    g->len = len;
                    g->dst = a.out + ob;
                    g->orig = orig;
                    g->ws = ws;
                    g->tile0 = (uint32_t)T;
                    g->ntiles = nt;
                    uint32_t seen[2] = {0u, 0u};
                    for (uint32_t p = 0; p < ws; ++p) {  // the rank table: position p is byte seen[r] of its stream's k[r]
                        const uint32_t r = nref > 1u && ld_u32_bytes(blob + 20 + 4 * p) == id[1] ? 1u : 0u;
                        g->rank[p] = (uint8_t)(seen[r]++ | (r ? kAnyDecSecond : 0u));
                    }
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        g->soff[r] = soff[r];
                        g->np[r] = np[r];
                        g->k[r] = (uint32_t)r < nref ? k[r] : 0u;
                        g->nb[r] = nb[r];
                    }
                    g->blk0[0] = (uint32_t)B;
                    g->blk0[1] = (uint32_t)B + nb[0];
                    if (a.status) a.status[msg] = ST_OK;
                    if (a.slot_off && a.out_len) a.out_len[msg] = orig;
                    mark = 1u;
                } else if (L < t.lcap) {  // a budget is spent: the one-workgroup kernel keeps the blob
                    t.large[L].ws = 0u;  // (no launch's record)
                }
            }
        }
        t.mark[it] = mark;
    }
}

// ---- block sums: one wave per 2,048-pair block, 64 B (32 pairs) per lane
__global__ __launch_bounds__(kAnyTeam) void tdt_anyd_block_kernel(AnyDecArgs t) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t nbk = anyd_claimed(t, ADC_BLOCKS, t.bcap), nl = anyd_claimed(t, ADC_LARGE, t.lcap);
    for (uint32_t e = blockIdx.x * (uint32_t)kAW + (threadIdx.x >> 6); e < nbk; e += gridDim.x * (uint32_t)kAW) {  // (per wave)
        uint32_t idx = 0;
        const AnyDecLarge *g = anyd_owner<true>(t, nl, e, idx);
        if (!g) continue;
        const uint32_t r = idx < g->nb[0] ? 0u : 1u, b = r ? idx - g->nb[0] : idx;
        const uint32_t np = g->np[r];
        const uint8_t *src = g->blob + g->soff[r], *lim = g->blob + g->len;
        uint32_t s2 = 0u;
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            const uint32_t p0 = kAnyDecPairs * b + 32u * lane + 8u * q;
            const uint32_t nv = p0 < np ? (np - p0 < 8u ? np - p0 : 8u) : 0u;
            const uint4 pv = nv ? ld16_span(src + 2ull * p0, (int)(2 * nv), lim) : make_uint4(0, 0, 0, 0);
            s2 += (pv.x & 0x00ff00ffu) + (pv.y & 0x00ff00ffu) + (pv.z & 0x00ff00ffu) + (pv.w & 0x00ff00ffu);
        }
        const uint32_t tot = wave_reduce<OpAdd>((s2 & 0xffffu) + (s2 >> 16));
        if (lane == 0) t.bsum[e] = tot;
    }
}

// ---- scan: one workgroup per long blob; per stream the block sums → their exclusive prefixes, clamped
__global__ __launch_bounds__(kAnyTeam) void tdt_anyd_scan_kernel(AnyDecArgs t) {
    __shared__ uint32_t s_slots[2][kAW];
    const uint32_t tid = threadIdx.x;
    const uint32_t nl = anyd_claimed(t, ADC_LARGE, t.lcap);
    uint32_t alt = 0u;
    for (uint32_t L = blockIdx.x; L < nl; L += gridDim.x) {
        const AnyDecLarge *g = t.large + L;
        const uint32_t ws = (uint32_t)__builtin_amdgcn_readfirstlane((int)g->ws);
        if (ws == 0u) continue;  // (uniform)
        const uint32_t wc = g->orig / ws;
        for (uint32_t r = 0; r < 2u; ++r) {
            const uint32_t k = g->k[r], nb = g->nb[r];
            if (!k) continue;
            const uint32_t S = wc * k;
            uint32_t *E = t.bsum + g->blk0[r];
            uint32_t carry = 0u;  // (uniform) the clamped prefix behind the blocks so far
            for (uint32_t i0 = 0; i0 < nb; i0 += kAnyTeam) {
                const uint32_t i = i0 + tid;
                uint32_t v[1] = {i < nb ? E[i] : 0u}, tot[1];
                team_excl_scan<kAW, 1, OpAdd>(v, tot, s_slots[alt]);  // (256 blocks: below 2^28)
                alt ^= 1u;
                if (i < nb) E[i] = any_dec_scan_step(carry, v[0], S);
                carry = any_dec_scan_step(carry, tot[0], S);
            }
        }
    }
}

// ---- tile: one workgroup per 32 KiB of output
__global__ __launch_bounds__(kAnyTeam) void tdt_anyd_tile_kernel(AnyDecArgs t) {
    // the referenced streams' planes: the decoded stream bytes of the tile's range, stream 1's
    // behind stream 0's at the next multiple of 16 (Σ k_r = ws: at most kAnyDecTile bytes together)
    __shared__ __attribute__((aligned(16))) uint8_t s_plane[kAnyDecTile + 16];
    __shared__ uint8_t s_rank[kAnyWsMax];
    __shared__ uint32_t s_slots[2][kAW];
    const uint32_t tid = threadIdx.x;
    const uint32_t nt = anyd_claimed(t, ADC_TILES, t.tcap), nl = anyd_claimed(t, ADC_LARGE, t.lcap);
    uint32_t alt = 0u;
    for (uint32_t e = blockIdx.x; e < nt; e += gridDim.x) {  // (uniform)
        uint32_t tt = 0;
        const AnyDecLarge *g = anyd_owner<false>(t, nl, e, tt);
        if (!g) continue;
        const uint32_t ws = (uint32_t)__builtin_amdgcn_readfirstlane((int)g->ws);
        const uint32_t orig = (uint32_t)__builtin_amdgcn_readfirstlane((int)g->orig);
        const uint32_t ntiles = (uint32_t)__builtin_amdgcn_readfirstlane((int)g->ntiles);
        const uint32_t kk[2] = {(uint32_t)__builtin_amdgcn_readfirstlane((int)g->k[0]),
                                (uint32_t)__builtin_amdgcn_readfirstlane((int)g->k[1])};
        const uint32_t wc = orig / ws, wbytes = wc * ws;
        const AnyDecWords W = any_dec_tile_words_of(tt, wc, any_dec_tile_words(ws));
        const AnyDecBytes J = any_dec_tile_bytes(tt, ntiles, W, ws, orig);
        const uint32_t nw = W.w1 - W.w0;
        const uint32_t off1 = (nw * kk[0] + 15u) & ~15u;  // stream 1's plane
        const uint32_t used = off1 + nw * kk[1];           // (<= kAnyDecTile + 15)
        __syncthreads();  // (the tile before is done with the planes)
        for (uint32_t i = 16u * tid; i < used; i += 16u * kAnyTeam)  // zero: a short or empty stream leaves zeros
            *reinterpret_cast<uint4 *>(s_plane + i) = make_uint4(0, 0, 0, 0);
        if (tid < ws) s_rank[tid] = g->rank[tid];
        __syncthreads();
        const uint8_t *blob = g->blob, *blim = blob + g->len;
        for (uint32_t r = 0; r < 2u; ++r) {
            const uint32_t k = kk[r];
            const uint32_t np = (uint32_t)__builtin_amdgcn_readfirstlane((int)g->np[r]);
            if (!k || !np) continue;  // (uniform)
            const AnyDecRange R = any_dec_stream_range(W, k);
            const uint32_t *E = t.bsum + g->blk0[r];
            const uint32_t b = any_dec_first_block([&](uint32_t i) { return gload<uint32_t>(E + i); },
                                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)g->nb[r]), R.q0);
            uint64_t sbase = gload<uint32_t>(E + b);  // decoded bytes before this chunk (exact: below the stream's share)
            const uint8_t *src = blob + g->soff[r];
            uint8_t *plane = s_plane + (r ? off1 : 0u);
            for (uint32_t pc = b * kAnyDecPairs; pc < np && sbase < R.q1; pc += kAnyDecPairs) {
                const uint32_t p0 = pc + 8u * tid;
                const uint32_t nv = p0 < np ? (np - p0 < 8u ? np - p0 : 8u) : 0u;
                const uint4 pv = nv ? ld16_span(src + 2ull * p0, (int)(2 * nv), blim) : make_uint4(0, 0, 0, 0);
                const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w};
                const uint32_t s2 = (pw[0] & 0x00ff00ffu) + (pw[1] & 0x00ff00ffu) + (pw[2] & 0x00ff00ffu) +
                                    (pw[3] & 0x00ff00ffu);
                uint32_t v[1] = {(s2 & 0xffffu) + (s2 >> 16)}, tot[1];
                const uint32_t mine = v[0];
                team_excl_scan<kAW, 1, OpAdd>(v, tot, s_slots[alt]);
                alt ^= 1u;
                uint64_t q = sbase + v[0];
                if (mine && q < R.q1 && q + mine > R.q0) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const uint32_t pr = pw[i >> 1] >> (16 * (i & 1));
                        const uint32_t c = pr & 0xffu;  // (count 0 emits nothing :602)
                        const uint8_t val = (uint8_t)(pr >> 8);
                        const AnyDecClip cl = any_dec_clip(q, c, R.q0, R.q1);
                        for (uint32_t j = 0; j < cl.n; ++j) plane[cl.off + j] = val;
                        q += c;
                    }
                }
                sbase += tot[0];
            }
        }
        __syncthreads();
        // ---- recombine: output byte j of word w, position p, is byte (w - w0) * k_r + rank[p] of its stream's plane
        uint8_t *dst = g->dst;
        auto byte_at = [&](uint32_t j) -> uint32_t {
            if (j >= wbytes) return 0u;  // past the last whole word
            const uint32_t w = j / ws, p = j - w * ws, rk = s_rank[p];
            return s_plane[((rk & kAnyDecSecond) ? off1 + (w - W.w0) * kk[1] : (w - W.w0) * kk[0]) + (rk & 63u)];
        };
        // the bytes before the first 16-byte boundary of the destination and behind the last, one lane each
        const uint32_t nbytes = J.je - J.jb;
        const uint32_t mis = (uint32_t)(16u - ((uintptr_t)(dst + J.jb) & 15u)) & 15u;
        const uint32_t head = mis < nbytes ? mis : nbytes;
        const uint32_t ngroups = (nbytes - head) / 16u;
        const uint32_t jt = J.jb + head + 16u * ngroups;  // the tail's first byte
        if (tid < head) dst[J.jb + tid] = (uint8_t)byte_at(J.jb + tid);
        if (tid >= 64u && jt + (tid - 64u) < J.je) dst[jt + (tid - 64u)] = (uint8_t)byte_at(jt + (tid - 64u));
        for (uint32_t gi = tid; gi < ngroups; gi += kAnyTeam) {
            const uint32_t j = J.jb + head + 16u * gi;
            const uint32_t w = j / ws;
            uint32_t p = j - w * ws;  // wraps at ws: no division per byte
            uint32_t a0 = (w - W.w0) * kk[0], a1 = off1 + (w - W.w0) * kk[1];
            uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (j + (uint32_t)i < wbytes) {
                    const uint32_t rk = s_rank[p];
                    o[i >> 2] |= (uint32_t)s_plane[((rk & kAnyDecSecond) ? a1 : a0) + (rk & 63u)] << (8 * (i & 3));
                }
                if (++p == ws) {
                    p = 0u;
                    a0 += kk[0];
                    a1 += kk[1];
                }
            }
            st16_nt(dst + j, make_uint4(o[0], o[1], o[2], o[3]));  // aligned in the destination
        }
    }
}

}  // namespace

int launch_encode_any(const EncodeArgs &a, int ws, int mode, hipStream_t s, bool pair, const AnyTiledArgs *tiled) {
    if (a.n_msgs == 0) return 0;
    if (pair ? mode != MODE_ENCODE && mode != MODE_SIZES && mode != MODE_MAPPED : mode == MODE_SIZES)
        return (int)hipErrorInvalidValue;
    const dim3 g(a.n_msgs), t(kAnyTeam);
    const uint32_t w = (uint32_t)ws;
    const uint32_t *mark = nullptr;
    if (mode == MODE_ANALYZE) tiled = nullptr;
    if (tiled) {  // the long messages' records and marks first: the kernel below returns at a marked message
        const dim3 pg((a.n_msgs + 255u) / 256u), pt(256);
        if (pair) hipLaunchKernelGGL(tdt_any_plan_kernel<true>, pg, pt, 0, s, a, *tiled, w, mode);
        else hipLaunchKernelGGL(tdt_any_plan_kernel<false>, pg, pt, 0, s, a, *tiled, w, mode);
        mark = tiled->mark;
    }
#define PSY_ANY_HP(MODE_, PAIR_)                                                                                    \
    do {                                                                                                            \
        if (ws <= 8) hipLaunchKernelGGL((tdt_encode_any_kernel<MODE_, 8, PAIR_>), g, t, 0, s, a, w, mark);          \
        else if (ws <= 16) hipLaunchKernelGGL((tdt_encode_any_kernel<MODE_, 16, PAIR_>), g, t, 0, s, a, w, mark);   \
        else if (ws <= 32) hipLaunchKernelGGL((tdt_encode_any_kernel<MODE_, 32, PAIR_>), g, t, 0, s, a, w, mark);   \
        else hipLaunchKernelGGL((tdt_encode_any_kernel<MODE_, 64, PAIR_>), g, t, 0, s, a, w, mark);                 \
    } while (0)
    if (pair && mode == MODE_SIZES) PSY_ANY_HP(MODE_SIZES, true);
    else if (pair && mode == MODE_MAPPED) hipLaunchKernelGGL((tdt_encode_any_kernel<MODE_MAPPED, 1, true>), g, t, 0, s, a, w, mark);
    else if (pair) PSY_ANY_HP(MODE_ENCODE, true);
    else if (mode == MODE_ENCODE) PSY_ANY_HP(MODE_ENCODE, false);
    else if (mode == MODE_ANALYZE) PSY_ANY_HP(MODE_ANALYZE, false);
    else hipLaunchKernelGGL((tdt_encode_any_kernel<MODE_MAPPED, 1>), g, t, 0, s, a, w, mark);
#undef PSY_ANY_HP
    if (tiled && tiled->lcap && tiled->tcap) {  // the tile pipeline: fixed grids over the plan's device-side counts
        const AnyTiledArgs &T = *tiled;
        const uint32_t grid = T.grid ? T.grid : 1u;
        const dim3 gl(std::min(grid, T.lcap)), gt(std::min(grid, T.tcap));
        const dim3 gh(std::min(grid, (T.tcap + kAnySpanTiles - 1) / kAnySpanTiles));
        if (mode != MODE_MAPPED) {  // (a known mapping is in the record already)
            if (ws <= 8) hipLaunchKernelGGL(tdt_any_hist_kernel<8>, gh, dim3(kAnyHistTeam), 0, s, T, w);
            else if (ws <= 16) hipLaunchKernelGGL(tdt_any_hist_kernel<16>, gh, dim3(kAnyHistTeam), 0, s, T, w);
            else if (ws <= 32) hipLaunchKernelGGL(tdt_any_hist_kernel<32>, gh, dim3(kAnyHistTeam), 0, s, T, w);
            else hipLaunchKernelGGL(tdt_any_hist_kernel<64>, gh, dim3(kAnyHistTeam), 0, s, T, w);
            hipLaunchKernelGGL(tdt_any_map_kernel, gl, t, 0, s, T, w);
        }
        hipLaunchKernelGGL(tdt_any_tile_kernel<false>, gt, t, 0, s, T, w);
        hipLaunchKernelGGL(tdt_any_scan_kernel, gl, t, 0, s, a, T, w, mode);
        if (mode != MODE_SIZES) hipLaunchKernelGGL(tdt_any_tile_kernel<true>, gt, t, 0, s, T, w);
    }
    return (int)hipGetLastError();
}

int launch_decode_any(const DecodeArgs &a, uint32_t grid, hipStream_t s, bool pair, const AnyDecArgs *tiled, uint32_t *seen) {
    const uint32_t *mark = nullptr;
    if (tiled) {  // the long blobs' records and marks first: the kernel below skips a marked entry
        const dim3 pg(std::max(1u, std::min((a.n_msgs + 255u) / 256u, tiled->grid ? tiled->grid : 1u))), pt(256);
        if (pair) hipLaunchKernelGGL(tdt_anyd_plan_kernel<true>, pg, pt, 0, s, a, *tiled);
        else hipLaunchKernelGGL(tdt_anyd_plan_kernel<false>, pg, pt, 0, s, a, *tiled);
        mark = tiled->mark;
    }
    if (pair) hipLaunchKernelGGL(tdt_decode_any_kernel<true>, dim3(grid ? grid : 1u), dim3(kAnyTeam), 0, s, a, mark, seen);
    else hipLaunchKernelGGL(tdt_decode_any_kernel<false>, dim3(grid ? grid : 1u), dim3(kAnyTeam), 0, s, a, mark, seen);
    if (tiled && tiled->lcap && tiled->bcap && tiled->tcap) {  // the tile pipeline: fixed grids over the plan's device-side counts
        const AnyDecArgs &T = *tiled;
        const uint32_t g = T.grid ? T.grid : 1u;
        hipLaunchKernelGGL(tdt_anyd_block_kernel, dim3(std::min(g, (T.bcap + kAW - 1) / kAW)), dim3(kAnyTeam), 0, s, T);
        hipLaunchKernelGGL(tdt_anyd_scan_kernel, dim3(std::min(g, T.lcap)), dim3(kAnyTeam), 0, s, T);
        hipLaunchKernelGGL(tdt_anyd_tile_kernel, dim3(std::min(g, T.tcap)), dim3(kAnyTeam), 0, s, T);
    }
    return (int)hipGetLastError();
}

}  // namespace psy
