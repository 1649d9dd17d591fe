// tdt_dec_reduce_tiled.h — the tiled form of decode-reduce: a destination of tdt_decode_reduce_v whose
// decoded size is above the batch's large-message threshold (the tuned plan's rule: max(large_min,
// 1/4096 of the batch's decoded bytes), taken on the device) is summed as tiles of kRedTileBytes of
// output, one workgroup per tile and one wave per peer, so one long tensor spreads over the chip.  The
// bits are the one-workgroup kernel's: the same decode_fast, the same staging and acc4 chain in peer
// order (RedSink), cut at tile edges that are whole windows.
//
// Passes, all on the caller's stream, in order; the host reads nothing back:
//   sum     one lane per destination: the decoded size peer 0's blob claims (its magic and size
//           word); a partial sum per workgroup.  Workgroup 0 clears the counter block.
//   plan    one lane per destination: threshold from the partial sums; a destination above it claims
//           (workgroup-aggregated atomics) one record, ceil(size / tile) tile entries and
//           sum_k (len_k / 1024 + 3) block sums, and sets its mark word.  A claim is a hint: over a
//           budget means no mark, and the destination stays on the one-workgroup kernel.
//   prep    one workgroup per claimed record, wave k on peer k: the header phase of the one-workgroup
//           kernel (red_header, red_verdict).  TDT_OK and fused: the record is filled and status, length
//           and peer statuses are written.  Anything else (a refusal, the serial path): the mark is
//           cleared and the record's tile and block entries are emptied — the one-workgroup kernel,
//           which runs next over the whole grid and returns at a marked destination, does what it
//           always did.  A refused destination is untouched because prep precedes the tile launch.
//   blocks  one wave per 512-pair block of every (peer, referenced stream): the block's count sum.
//   scan    one wave per (record, peer, stream): block sums to exclusive start positions in place, the
//           stream's decoded length, and for every tile t >= 1 the block that holds position
//           t * TS - 1 (tdt_red_tiles.h).  Peers differ in mapping, so the tables are per peer.
//   tiles   tdt_decode_reduce_tile_kernel<NW>: a workgroup strides over the tile entries; wave k runs
//           decode_fast over the tile's groups [g_lo, g_hi) with its peer's carries, an UNCP wave
//           fills its slice from blob + 4 + 16 g, a wave without a peer walks the same windows.
//
// BARRIERS of the tile kernel.  Every wave of a workgroup meets every workgroup barrier the same
// number of times:
//   1. the loop over tile entries has a trip count from blockIdx, gridDim and the device-side tile
//      count alone; the entry, its record and the tile's group range are read from the same words by
//      every wave and held in scalar registers, so `continue` is taken by all waves or none, and the
//      barrier between two entries is met by all;
//   2. inside a tile the barriers are all in RedSink::window, which every wave calls exactly once per
//      window: from decode_fast's window loop (`for gwin = g_lo; gwin < g_hi; gwin += 64 WR`), from
//      the UNCP loop and from the idle loop (`for win = 0; win < nwin`, nwin = ceil((g_hi - g_lo) /
//      kRedWinGroups)).  The trip counts come from the tile's group range alone, never from a peer's
//      header, stream lengths or pair counts: a wave whose streams have ended keeps walking windows
//      and stages zeros.  The three callers are selected by wave-uniform scalars (the wave index and
//      the record's kind), and none of them leaves its loop early.
//
// A tile is kRedTileWin whole windows, so no window straddles two tiles and only a tensor's last
// window is partial; it starts a multiple of 16 bytes into an element-aligned destination, so it
// holds whole elements, and two tiles never share a group.
//
// WIDE destinations (a widening code: 2-byte wire elements summed into fp32, tdt_dec_reduce.h).  The
// sum, plan, block and scan passes work in decoded wire bytes and are the same: the threshold is held
// against decoded bytes and a destination claims ceil(w / kRedTileBytes) tiles.  A tile is still
// kRedTileWin wire windows; the wide sink writes 2 kRedTileBytes = 67,584 destination bytes for it,
// from destination group 2 g_lo to min(2 g_hi, the destination's end).  The record keeps the decoded
// size; prep reports 2 w as the length.  Prep always takes the widening header checks (red_header<true>:
// a narrow call cannot hold a widening code, so it decides as before), and a wide destination with a peer
// off the fast path is not tiled: its mark is cleared and the one-workgroup kernel refuses it.  The
// tile kernel has a second set of instances (tdt_decode_reduce_tile_wide_kernel) launched when the
// call's codes may widen, so the narrow instances keep their registers.
#pragma once
#include "tdt_dec_reduce.h"
#include "tdt_red_tiles.h"

namespace psy {

static_assert(kRedWinRounds == (uint32_t)kRedWR, "tdt_red_tiles.h restates the decoder's window");
static_assert(kRedTileGroups % kRedWinGroups == 0, "a tile is whole windows");
static_assert(8 * (RC_TILED_TILES + 1) <= kPlanSnapBytes, "every counter is zeroed per call and snapshotted");

constexpr uint32_t kRedTblk = 2u * kRedMaxPeers;  // carry blocks per tile: (peer, stream)

// A peer of a tiled destination: its parsed header and blob (prep), per referenced stream the first
// block sum (relative to the record's blk0) and the block count (prep) and the decoded length (scan)
struct RedPeer {
    FastHdr H;
    uint64_t blob, len;
    uint32_t bbase[2], nb[2], slen[2];
};
struct RedRec {
    uint32_t msg;    // the destination, or kNone: over a budget (the plan emptied its ranges)
    uint32_t tiled;  // prep: 1 when the tile pass sums it
    uint32_t elem, n_peers;
    uint32_t tile0, ntiles, blk0, nbs;  // the claimed ranges (plan)
    uint64_t dst, osize;
    RedPeer p[kRedMaxPeers];
};

struct RedTiledArgs {
    ReduceArgs a;             // (a.mark: one u32 per destination)
    unsigned long long *cnt;  // the counter block (RedCount, tdt_plan.h)
    uint64_t *part;           // the sum pass's partial sums, one per 1,024 destinations
    RedRec *rec;
    uint32_t *tent, *bent;    // tile and block entries: the record's index, or kNone
    uint32_t *bsum;           // per block: count sum, then (scan) start position
    uint32_t *tblk;           // kRedTblk per tile entry
    uint32_t lcap, tcap, bcap;  // (0, 0, 0: count only)
    uint64_t large_min;
};

// counter k of the block (u64 words), bounded by the budget the plan ran with: what a pass strides over
__device__ __forceinline__ uint32_t red_count(const RedTiledArgs &p, RedCount k, uint32_t cap) {
    const unsigned long long c = p.cnt[k];
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(c < cap ? (uint32_t)c : cap));
}

__global__ void tdt_decode_reduce_sum_kernel(RedTiledArgs p);
__global__ void tdt_decode_reduce_plan_kernel(RedTiledArgs p);
__global__ void tdt_decode_reduce_block_kernel(RedTiledArgs p);
__global__ void tdt_decode_reduce_scan_kernel(RedTiledArgs p);

#ifdef PSY_DEC_REDUCE_TU
// the decoded size peer 0's blob of destination i claims (its magic and size word, unchecked), as
// tdt_decode_plan_kernel reads it
__device__ __forceinline__ uint64_t red_claimed_size(const ReduceArgs &a, uint32_t i) {
    const uint64_t len = a.blob_len[i];
    if (len < 4) return 0;
    const uint8_t *bp = reinterpret_cast<const uint8_t *>(a.blobs[i]);
    uint32_t magic, w1 = 0;
    if (len >= 8 && ((uintptr_t)bp & 7) == 0) {  // (one 8-byte load instead of eight byte loads)
        const uint2 v = *reinterpret_cast<const uint2 *>(bp);
        magic = v.x;
        w1 = v.y;
    } else {
        magic = ld_u32_bytes(bp);
        if (len >= 8) w1 = ld_u32_bytes(bp + 4);
    }
    if (magic == kMagicUNCP) return len - 4;
    return magic == kMagicTDT && len >= 20 ? (uint64_t)w1 : 0ull;
}

// the sum of x over the workgroup's 1,024 threads, in every thread (lds: 16 words)
__device__ __forceinline__ uint64_t red_wg_sum(uint64_t x, uint64_t *lds) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    uint64_t s = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += lds[q];
    __syncthreads();  // (lds is reused)
    return s;
}

__global__ __launch_bounds__(1024) void tdt_decode_reduce_sum_kernel(RedTiledArgs p) {
    __shared__ uint64_t lds[16];
    const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
    const uint64_t s = red_wg_sum(i < p.a.n_msgs ? red_claimed_size(p.a, i) : 0ull, lds);
    if (threadIdx.x == 0) p.part[blockIdx.x] = s;
    // (the claims are the next launch's: the counters of this call start from zero)
    if (blockIdx.x == 0 && threadIdx.x < kPlanSnapBytes / 8) p.cnt[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(1024) void tdt_decode_reduce_plan_kernel(RedTiledArgs p) {
    __shared__ uint64_t lds[3 * (16 + 1)];
    const uint32_t n = p.a.n_msgs, i = blockIdx.x * 1024u + threadIdx.x;
    // one workgroup per destination keeps the chip busy while a destination is at most ~1/4096 of the
    // batch's bytes; only larger ones (and only above large_min) are worth the tiled passes
    uint64_t tot = 0;
    for (uint32_t q = threadIdx.x; q < (n + 1023u) / 1024u; q += 1024u) tot += p.part[q];
    tot = red_wg_sum(tot, lds);
    const uint64_t share = tot / 4096, thr = share > p.large_min ? share : p.large_min;
    uint64_t A[3][1] = {{0}, {0}, {0}}, SA[3][1];
    if (i < n) {
        const uint64_t osz = red_claimed_size(p.a, i);
        if (osz > thr && (osz >> 35) == 0) {  // (2^35 and more: refused by the header's checks)
            A[0][0] = 1;
            A[1][0] = red_ntiles(osz);
            for (uint32_t k = 0; k < p.a.n_peers; ++k) A[2][0] += red_block_claim(p.a.blob_len[(uint64_t)k * n + i]);
        }
    }
    {
        constexpr int ia[3] = {RC_LARGE, RC_TILES, RC_BLOCKS};
        wg_claim_n<3, 1>(A, SA, p.cnt, ia, lds);
    }
    if (i >= n || !p.a.mark) return;
    const uint64_t j = SA[0][0], t0 = SA[1][0], b0 = SA[2][0], nt = A[1][0], nb = A[2][0];
    bool large = false;
    if (A[0][0]) {
        large = j < p.lcap && t0 + nt <= p.tcap && b0 + nb <= p.bcap;
        if (large) {
            RedRec *m = p.rec + j;
            m->msg = i;
            m->tiled = 0;
            m->tile0 = (uint32_t)t0;
            m->ntiles = (uint32_t)nt;
            m->blk0 = (uint32_t)b0;
            m->nbs = (uint32_t)nb;
        } else {  // over a budget: the one-workgroup kernel; the ranges it claimed stay empty
            if (j < p.lcap) p.rec[j].msg = kNone;
            for (uint64_t t = t0; t < t0 + nt && t < p.tcap; ++t) p.tent[t] = kNone;
            for (uint64_t b = b0; b < b0 + nb && b < p.bcap; ++b) p.bent[b] = kNone;
        }
    }
    const_cast<uint32_t *>(p.a.mark)[i] = large ? 1u : 0u;
}

// Block pass: one wave per 512-pair block (8 pairs per lane): the block's count sum.
__global__ __launch_bounds__(256) void tdt_decode_reduce_block_kernel(RedTiledArgs p) {
    const uint32_t nslots = red_count(p, RC_BLOCKS, p.bcap);
    for (uint32_t slot = blockIdx.x * 4u + (threadIdx.x >> 6); slot < nslots; slot += gridDim.x * 4u) {
        const uint32_t j = p.bent[slot];
        if (j == kNone) continue;
        const RedRec *m = p.rec + j;
        const uint32_t idx = slot - m->blk0;
        // the (peer, stream) whose blocks hold the slot (at most one: their ranges are disjoint)
        uint32_t pk = kNone, pr = 0, b = 0;
        for (uint32_t k = 0; k < m->n_peers; ++k)
#pragma unroll
            for (uint32_t r = 0; r < 2; ++r) {
                const uint32_t o = idx - m->p[k].bbase[r];
                if (o < m->p[k].nb[r]) pk = k, pr = r, b = o;
            }
        if (pk == kNone) continue;
        const RedPeer &P = m->p[pk];
        const uint8_t *blob = reinterpret_cast<const uint8_t *>(P.blob);
        const uint32_t np = P.H.np[pr], soff = P.H.soff[pr];
        const uint32_t p0 = kRedBlockPairs * b + 8u * (uint32_t)lane_id();
        const uint32_t nv = p0 < np ? (np - p0 < 8u ? np - p0 : 8u) : 0u;
        const uint4 pv = nv ? ld16_span(blob + soff + 2ull * p0, (int)(2 * nv), blob + P.len) : make_uint4(0, 0, 0, 0);
        const uint32_t s2 = (pv.x & 0x00ff00ffu) + (pv.y & 0x00ff00ffu) + (pv.z & 0x00ff00ffu) + (pv.w & 0x00ff00ffu);
        const uint32_t tot = wave_reduce<OpAdd>((s2 & 0xffffu) + (s2 >> 16));
        if (lane_id() == 0) p.bsum[m->blk0 + idx] = tot;
    }
}

// Scan: one wave per (record, peer, stream), blockIdx.y = 2 peer + stream.
__global__ __launch_bounds__(64) void tdt_decode_reduce_scan_kernel(RedTiledArgs p) {
    const uint32_t nl = red_count(p, RC_LARGE, p.lcap);
    const uint32_t k = blockIdx.y >> 1, r = blockIdx.y & 1u;
    for (uint32_t j = blockIdx.x; j < nl; j += gridDim.x) {
        RedRec *m = p.rec + j;
        if (m->msg == kNone || !m->tiled || k >= m->n_peers) continue;
        RedPeer &P = m->p[k];
        if (P.H.kind != 2u || (r == 1u && !P.H.two)) continue;
        const uint32_t lane = (uint32_t)lane_id();
        const uint32_t n = P.nb[r], base = m->blk0 + P.bbase[r];
        const uint64_t TS = (uint64_t)kRedTileGroups * P.H.seg[r];  // stream positions per tile
        const uint32_t nt = m->ntiles;
        uint32_t *tb = p.tblk + (uint64_t)kRedTblk * m->tile0 + 2u * k + r;
        uint64_t run = 0;
        for (uint32_t c0 = 0; c0 < n; c0 += 64) {
            const uint32_t b = c0 + lane;
            const uint32_t v = b < n ? p.bsum[base + b] : 0u;
            const uint32_t incl = wave_incl_scan<OpAdd>(v);
            const uint64_t st = run + incl - v;
            if (b < n) {
                p.bsum[base + b] = (uint32_t)st;
                const RedTileSpan s = red_block_tiles(st, v, TS, nt);
                for (uint64_t t = s.t0; t < s.t1; ++t) tb[kRedTblk * t] = b;
            }
            run += rdlane(incl, 63);
        }
        // (no tile asks for a position at or above 2^32: a longer stream reads as that long)
        if (lane == 0) P.slen[r] = run < 0xffffffffull ? (uint32_t)run : 0xffffffffu;
    }
}
#endif  // PSY_DEC_REDUCE_TU

// Prep: one workgroup per claimed record (a grid striding over the device-side count).
template <int NW>
__global__ __launch_bounds__(64 * NW) void tdt_decode_reduce_prep_kernel(RedTiledArgs p) {
    __shared__ __attribute__((aligned(16))) uint8_t hdrs[NW][kHdrCache];
    __shared__ __attribute__((aligned(16))) uint32_t rec[4 * kRedMaxPeers];
    __shared__ uint32_t s_nb[2 * kRedMaxPeers];
    const ReduceArgs &a = p.a;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t n_peers = a.n_peers;
    const uint32_t nl = red_count(p, RC_LARGE, p.lcap);
    for (uint32_t j = blockIdx.x; j < nl; j += gridDim.x) {
        if (j != blockIdx.x) __syncthreads();  // (the LDS records of the previous one are read)
        RedRec *m = p.rec + j;
        const uint32_t msg = (uint32_t)__builtin_amdgcn_readfirstlane((int)m->msg);
        if (msg == kNone) continue;  // over a budget
        const uint32_t elem =
            (uint32_t)__builtin_amdgcn_readfirstlane((int)(a.elem_codes ? (uint32_t)a.elem_codes[msg] : a.elem));
        uint8_t *dst = reinterpret_cast<uint8_t *>(a.outs[msg]);
        RedHead P{};
        if (w < n_peers) P = red_header<true>(a, msg, w, elem, dst, a.out_cap[msg], hdrs[w], rec);
        if (lane == 0 && w < kRedMaxPeers) {
            const bool fast = w < n_peers && P.H.kind == 2u;
            s_nb[2 * w] = fast ? red_nblocks(P.H.np[0]) : 0u;
            s_nb[2 * w + 1] = fast && P.H.two ? red_nblocks(P.H.np[1]) : 0u;
        }
        __syncthreads();  // header barrier: every wave, once per record
        const RedVerdict V = red_verdict(rec, n_peers);
        uint32_t before = 0, total = 0;  // this wave's first block, and the destination's blocks
        for (uint32_t q = 0; q < 2u * n_peers; ++q) {
            if (q < 2u * w) before += s_nb[q];
            total += s_nb[q];
        }
        const uint32_t ntiles = m->ntiles, nbs = m->nbs;
        // (the claims came from peer 0's size word and the blob lengths: a verdict of TDT_OK agrees with them)
        const bool tiled = V.st == ST_OK && V.fused && red_ntiles(V.osize) == ntiles && total <= nbs;
        if (tiled && w < n_peers && lane == 0) {
            RedPeer &R = m->p[w];
            R.H = P.H;
            R.blob = (uint64_t)(uintptr_t)P.blob;
            R.len = P.len;
            R.bbase[0] = before;
            R.bbase[1] = before + s_nb[2 * w];
            R.nb[0] = s_nb[2 * w];
            R.nb[1] = s_nb[2 * w + 1];
            R.slen[0] = R.slen[1] = 0u;
        }
        if (w == 0 && lane == 0) {
            m->tiled = tiled ? 1u : 0u;
            if (tiled) {
                m->elem = elem;
                m->n_peers = n_peers;
                m->dst = (uint64_t)(uintptr_t)dst;
                m->osize = V.osize;
                a.status[msg] = (int32_t)ST_OK;
                if (a.out_len) a.out_len[msg] = red_wide(elem) ? 2ull * V.osize : V.osize;
                atomicAdd(p.cnt + RC_TILED, 1ull);
                atomicAdd(p.cnt + RC_TILED_TILES, (unsigned long long)ntiles);
            } else {
                const_cast<uint32_t *>(a.mark)[msg] = 0u;  // the one-workgroup kernel takes it, whatever it is
            }
        }
        const uint32_t ev = tiled ? j : kNone;
        for (uint32_t i = threadIdx.x; i < ntiles; i += 64u * NW) p.tent[m->tile0 + i] = ev;
        for (uint32_t i = threadIdx.x; i < nbs; i += 64u * NW) p.bent[m->blk0 + i] = ev;
    }
}

// Tile pass: a workgroup of NW waves per tile entry (a grid striding over the device-side count).
template <int NW, bool WIDE>
__device__ __forceinline__ void red_tiles(const RedTiledArgs &p) {
    using Lay = RedLayout<NW>;
    __shared__ __attribute__((aligned(16))) uint8_t smem[Lay::BYTES];
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = (uint32_t)lane_id();
    uint8_t *dec = smem + w * (uint32_t)Lay::DEC;
    const bool set = (p.a.flags & kRedSet) != 0u;
    const uint32_t nt = red_count(p, RC_TILES, p.tcap);
    for (uint32_t slot = blockIdx.x; slot < nt; slot += gridDim.x) {
        if (slot != blockIdx.x) __syncthreads();  // (every wave is done with the previous tile's LDS)
        const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.tent[slot]);
        if (j == kNone) continue;
        const RedRec *m = p.rec + j;
        const uint32_t t = slot - (uint32_t)__builtin_amdgcn_readfirstlane((int)m->tile0);
        const uint64_t osize = m->osize;
        const uint32_t gc = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((osize + 15) / 16));
        const RedGroups G = red_tile_groups(t, gc);
        if (G.g_lo >= G.g_hi) continue;
        const uint32_t g_lo = G.g_lo, g_hi = G.g_hi;
        const uint32_t nwin = (g_hi - g_lo + kRedWinGroups - 1) / kRedWinGroups;
        const uint32_t n_peers = (uint32_t)__builtin_amdgcn_readfirstlane((int)m->n_peers);
        uint8_t *dst = reinterpret_cast<uint8_t *>(m->dst);
        using Sink = RedSinkT<NW, WIDE>;
        Sink S;
        S.stage = smem + Lay::OFF_STAGE;
        S.mine = S.stage + w * kRedSlice;
        S.dst = dst;
        S.osize = osize;
        S.gc = g_hi;  // (the sink's bound: the tile's end)
        S.gbase = g_lo;
        S.n_peers = n_peers;
        S.elem = (uint32_t)__builtin_amdgcn_readfirstlane((int)m->elem);
        S.tid = threadIdx.x;
        S.set = set;
        S.dal16 = ((uintptr_t)dst & 15) == 0;
#pragma unroll
        for (int q = 0; q < Sink::NPF; ++q) S.dpre[q] = make_uint4(0, 0, 0, 0);
        S.prefetch(0);
        const RedPeer &P = m->p[w < n_peers ? w : 0u];
        const uint32_t kind = (uint32_t)__builtin_amdgcn_readfirstlane((int)(w < n_peers ? P.H.kind : 0u));
        const uint8_t *blob = reinterpret_cast<const uint8_t *>(P.blob), *blim = blob + P.len;
        if (kind == 2u) {
            const FastHdr H = P.H;
            const uint64_t wbytes = (uint64_t)(H.orig / H.ws) * H.ws;
            uint32_t b0[2] = {0u, 0u}, s0[2] = {0u, 0u};
            if (g_lo > 0) {
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    if (r == 1 && !H.two) break;
                    const uint32_t *bs = p.bsum + m->blk0 + P.bbase[r];
                    const RedCarry c = red_tile_carry(g_lo * H.seg[r], P.slen[r], p.tblk[(uint64_t)kRedTblk * slot + 2u * w + r],
                                                      [&](uint32_t b) { return bs[b]; });
                    b0[r] = c.b0;
                    s0[r] = c.s0;
                }
            }
            // window loop inside: gwin = g_lo, g_lo + 64 WR, ... < g_hi, S.window(win) at the end of each
            decode_fast<kRedWR, false, Sink>(H, dec, blob, blim, nullptr, gc, wbytes, g_lo, g_hi, b0, s0, nullptr, 0u, 0u, &S);
        } else if (kind == 1u) {
            for (uint32_t win = 0; win < nwin; ++win) {
#pragma unroll
                for (uint32_t rl = 0; rl < (uint32_t)kRedWR; ++rl) {
                    const uint32_t g = g_lo + win * kRedWinGroups + rl * 64u + lane;
                    uint4 v = make_uint4(0, 0, 0, 0);
                    if (g < g_hi) {
                        const uint64_t left = osize - 16ull * g;
                        v = ld16_span(blob + 4 + 16ull * g, left >= 16 ? 16 : (int)left, blim);
                    }
                    S.put(rl * 64u + lane, v);
                }
                S.window(win);
            }
        } else {
            for (uint32_t win = 0; win < nwin; ++win) S.window(win);  // a wave without a peer
        }
    }
}
template <int NW>
__global__ __launch_bounds__(64 * NW) void tdt_decode_reduce_tile_kernel(RedTiledArgs p) {
    red_tiles<NW, false>(p);
}
template <int NW>
__global__ __launch_bounds__(64 * NW) void tdt_decode_reduce_tile_wide_kernel(RedTiledArgs p) {
    red_tiles<NW, true>(p);
}

#define PSY_DEC_REDUCE_TILED_INSTANCES(X)          \
    X(psy::tdt_decode_reduce_prep_kernel<2>)       \
    X(psy::tdt_decode_reduce_prep_kernel<4>)       \
    X(psy::tdt_decode_reduce_prep_kernel<8>)       \
    X(psy::tdt_decode_reduce_tile_kernel<2>)       \
    X(psy::tdt_decode_reduce_tile_kernel<4>)       \
    X(psy::tdt_decode_reduce_tile_kernel<8>)       \
    X(psy::tdt_decode_reduce_tile_wide_kernel<2>)  \
    X(psy::tdt_decode_reduce_tile_wide_kernel<4>)  \
    X(psy::tdt_decode_reduce_tile_wide_kernel<8>)

}  // namespace psy
