// tdt_dec_reduce.h — decode-reduce (tdt_decode_reduce_v): the blobs of up to 8 peers for one
// destination are decoded and summed into it in one pass, dst = ((dst + b0) + b1) + ... in the
// destination's element type (or, with TDT_REDUCE_SET, dst = (b0 + b1) + ...), the bits of that
// many tdt_decode_accumulate_v calls in peer order.  With a widening code (TDT_ELEM_F32_FROM_BF16 /
// _F16) the blobs hold 2-byte elements and the destination fp32 of twice the bytes: the same decode and
// staging, a sum stage that widens (RedSinkT, WIDE), in instances of their own; the fused path only —
// the serial kernel below sums through decode_one's ACC stores, which have no widening form, and
// psyne's encoder writes fast-path blobs only, so a wide destination with a peer off the fast path is
// TDT_E_UNSUPPORTED.
//
// Work split: one workgroup per destination, one 64-lane wave per peer; NW, the
// workgroup's wave count, is the smallest of 2, 4, 8 that holds the peers.  A wave without a peer
// stages nothing but keeps the barrier schedule and takes its share of the sums.
//
//   header   wave k parses peer k's blob (parse_fast; blob_check for every other shape), checks it
//            against the destination (capacity, element alignment and size: acc_status) and
//            publishes (kind, status, decoded size) to LDS.  One workgroup barrier; every wave then
//            reads all records and takes the same decision: refused (nothing is written), serial,
//            or fused.
//   fused    every peer is UNCP or a fast-path TDT blob.  The output is walked in the decoder's
//            windows of kRedWR rounds of 64 16-byte groups.  Wave k runs decode_fast on its blob with
//            a SINK: where a round's 16 recombined bytes per lane would be stored, they go to the
//            wave's LDS slice (1 KiB per round), bytes past the blob's last whole word as zeros.  An
//            UNCP wave fills its slice from blob + 4 (aligned dwords, funnel-shifted).  At the end of
//            a window (RedSink::window): barrier A, every lane of the workgroup takes groups of the
//            window, chains acc4 over the staged groups in peer order onto the destination group
//            (loaded before the window's decode, so its trip to memory lies under it) and stores it
//            once; barrier B frees the slices.  Destinations off 16 bytes and the last partial group
//            take 2-byte loads and stores around the same chain.
//   serial   some peer is valid but no fast-path blob (three or more referenced streams, odd
//            segments, more than 16 stored streams): the workgroup marks the destination and leaves;
//            a second launch on the same stream (tdt_decode_reduce_serial_kernel, below) runs the
//            one-wave accumulate decode (decode_one, ACC) over its peers in order.  Correct and slow;
//            psyne's encoder writes fast-path blobs.
//
// BARRIERS.  Every wave of a workgroup meets every workgroup barrier the same number of times:
//   1. the header barrier is unconditional (tdt_decode_reduce_kernel, "header barrier");
//   2. the refused / serial / fused decision is computed by every wave from the same LDS records
//      with the same code (red_verdict) and held in scalar registers; the refused and the serial
//      destination's workgroup returns there, all its waves at once;
//   3. the fused path's barriers are all in RedSink::window, which every wave calls exactly once per
//      window: from decode_fast's window loop (trip count: g_hi = the destination's common group
//      count `gc`, never a peer's header, stream lengths or pair counts; a wave whose streams have
//      ended keeps walking windows and stages zeros), from the UNCP loop and from the idle loop,
//      both `for (win = 0; win < nwin; ++win)` with nwin computed from gc alone.  The three callers
//      are selected by wave-uniform scalars (the wave index and the record's kind, through
//      readfirstlane), and none of them leaves its loop early.
//
// A long destination (above the batch's large-message threshold) is not walked by this kernel: the
// tiled form (tdt_dec_reduce_tiled.h) marks it, sums it as tiles over the whole device with the same
// sink, and the workgroup here returns at the mark (ReduceArgs::mark).  Without marks (a null array:
// TDT_OPT_REDUCE_TILED 0, a cold workspace under capture) and for every destination the tiled form
// leaves alone — short, refused, serial, over a budget — one workgroup walks the destination as
// described above, however long it is.
#pragma once
#include "tdt_decode.h"

namespace psy {

constexpr int kRedMaxPeers = 8;       // TDT_REDUCE_MAX_PEERS
constexpr uint32_t kRedSet = 1u;      // TDT_REDUCE_SET
constexpr uint32_t ST_MISMATCH = 14;  // TDT_E_MISMATCH
// d_status between the two launches: a valid destination left to the serial kernel.  Never reported.
constexpr uint32_t ST_RED_SERIAL = 0x101;
constexpr int kRedWR = kDecWR;        // rounds per window: the decoder's own
constexpr uint32_t kRedWinGroups = 64u * kRedWR;
constexpr uint32_t kRedSlice = 1024u * kRedWR;  // a peer's staged window

struct ReduceArgs {
    const uint64_t *blobs;     // [n_peers][n_msgs] blob addresses (peer-major)
    const uint64_t *blob_len;  // [n_peers][n_msgs]
    uint32_t n_msgs, n_peers;
    const uint64_t *outs;  // [n_msgs] destination addresses
    const uint64_t *out_cap;
    const uint8_t *elem_codes;  // [n_msgs], or null: `elem` for every destination
    uint32_t elem, flags;
    uint64_t *out_len;
    int32_t *status;
    int32_t *peer_status;  // [n_peers][n_msgs] or null
    // [n_msgs] or null: a destination with a set word is summed by the tile pass
    // (tdt_dec_reduce_tiled.h), and the one-workgroup kernel returns at it
    const uint32_t *mark;
};

// LDS of a workgroup of NW waves: each wave's decode state (the decoder's own layout), the staged
// windows and the peers' records.
template <int NW>
struct RedLayout {
    static constexpr int DEC = (DecLayoutT<kRedWR>::BYTES + 15) / 16 * 16;
    static constexpr int OFF_STAGE = NW * DEC;
    static constexpr int OFF_REC = OFF_STAGE + NW * (int)kRedSlice;
    static constexpr int BYTES = OFF_REC + 16 * kRedMaxPeers;  // a record: kind, status, size (u64)
    static_assert(BYTES <= 80 * 1024, "two workgroups per CU at 8 waves");
};

// 16 bytes of an element-aligned destination that is not 16-byte aligned, or the partial last
// group: dwords when 4-aligned and whole, else 2-byte accesses (every element size is a multiple of
// 2 and `valid` a whole number of elements); bytes at and past `valid` read as zero and stay untouched
__device__ __forceinline__ uint4 red_ld16(const uint8_t *p, uint32_t valid) {
    if (valid >= 16u && ((uintptr_t)p & 3) == 0) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
        return make_uint4(q[0], q[1], q[2], q[3]);
    }
    uint32_t w[4] = {0, 0, 0, 0};
    const uint16_t *q = reinterpret_cast<const uint16_t *>(p);
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i)
        if (2u * i < valid) w[i >> 1] |= (uint32_t)q[i] << (16u * (i & 1u));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void red_st16(uint8_t *p, uint4 v, uint32_t valid) {
    if (valid >= 16u && ((uintptr_t)p & 3) == 0) {
        uint32_t *q = reinterpret_cast<uint32_t *>(p);
        q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
        return;
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint16_t *q = reinterpret_cast<uint16_t *>(p);
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i)
        if (2u * i < valid) q[i] = (uint16_t)(w[i >> 1] >> (16u * (i & 1u)));
}

// The widening codes (TDT_ELEM_F32_FROM_BF16, TDT_ELEM_F32_FROM_F16): the destination's code in the
// low nibble, the wire's in the high one.  Decode-reduce's own: the accumulate kernels (acc_status,
// kElemMax) know neither.
constexpr uint32_t kElemF32FromBF16 = kElemF32 | kElemBF16 << 4, kElemF32FromF16 = kElemF32 | kElemF16 << 4;
__device__ __forceinline__ bool red_wide(uint32_t e) { return e == kElemF32FromBF16 || e == kElemF32FromF16; }

// Four wire elements (8 bytes of a staged slice) as fp32, exactly: bf16 is the upper half of an fp32
// (a shift and a mask per dword), fp16 goes through v_cvt_f32_f16, which keeps subnormals (the fp16
// denormal mode of these kernels is IEEE)
typedef float psy_f4 __attribute__((ext_vector_type(4)));
template <bool BF>
__device__ __forceinline__ psy_f4 red_widen(uint2 x) {
    psy_f4 r;
    if constexpr (BF) {
        r.x = __uint_as_float(x.x << 16);
        r.y = __uint_as_float(x.x & 0xffff0000u);
        r.z = __uint_as_float(x.y << 16);
        r.w = __uint_as_float(x.y & 0xffff0000u);
    } else {
        r.x = (float)__builtin_bit_cast(_Float16, (uint16_t)x.x);
        r.y = (float)__builtin_bit_cast(_Float16, (uint16_t)(x.x >> 16));
        r.z = (float)__builtin_bit_cast(_Float16, (uint16_t)x.y);
        r.w = (float)__builtin_bit_cast(_Float16, (uint16_t)(x.y >> 16));
    }
    return r;
}
__device__ __forceinline__ psy_f4 red_f4(uint4 v) {
    psy_f4 r;
    r.x = __uint_as_float(v.x), r.y = __uint_as_float(v.y), r.z = __uint_as_float(v.z), r.w = __uint_as_float(v.w);
    return r;
}

// red_ld16 / red_st16 of a wide destination: 4-byte aligned, `valid` a multiple of 4 (fp32 elements)
__device__ __forceinline__ uint4 red_ld16w(const uint8_t *p, uint32_t valid) {
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
        if (4u * i < valid) w[i] = q[i];
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void red_st16w(uint8_t *p, uint4 v, uint32_t valid) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t *q = reinterpret_cast<uint32_t *>(p);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
        if (4u * i < valid) q[i] = w[i];
}

// decode_fast's sink of the fused path (and the UNCP and idle waves' window step).  All fields but
// `tid` and `dpre` are uniform over the workgroup.
//
// WIDE instances also sum a destination with a widening code (red_wide(elem), a scalar branch taken
// once per prefetch and once per window, outside the peer loop): the wire elements are 2 bytes, the
// destination's fp32.  Nothing changes on the decode side: wave k stages the same window of
// kRedWinGroups wire groups in its slice, and gbase, gc and osize stay in WIRE groups and bytes.  What
// doubles is the destination: the window's 192 wire groups are 384 destination groups (6 KiB), the
// destination ends at 2 osize bytes, and window `win` starts at destination group 2 (gbase + 192 win).
//   - Destination group h of the window is wire bytes [8h, 8h + 8) of every peer's slice.  A lane
//     takes the groups h = tid + q T (NPF = 3 / 2 / 1 of them at NW = 2 / 4 / 8), and per peer issues
//     one ds_read_b64 at stage + k kRedSlice + 8h.
//   - Banks: the lanes of a wave read consecutive 8-byte words, 512 contiguous bytes per instruction.
//     The LDS serves a b64 read in passes of lanes that together cover a contiguous, 8-byte-aligned
//     span no longer than the banks' 4-byte stride times their count, so no two lanes of a pass meet
//     in a bank: the read runs at the width's own rate, whatever k (kRedSlice only moves the base).
//   - Adds: four v_add_f32 per peer and group.  This object is built without the packed fp32 forms
//     (build.py: DEC_ACC_FLAGS), so the 4-vector add below never becomes v_pk_add_f32; the
//     disassembly of the wide instances shows v_add_f32 only.
//   - Stores: one st16_nt of 16 consecutive destination bytes per lane where the group is whole and
//     16-byte aligned; otherwise (a destination 4 or 12 bytes off, the last group of 4, 8 or 12
//     bytes) dword loads and stores (red_ld16w / red_st16w) with `valid` from 2 osize, so no byte at or past 2 osize is touched.
//     A wire window that ends on half a wire group (osize % 16 in 1..8) ends one destination group
//     earlier: the bound is min(2 gc, ceil(2 osize / 16)).
//   - BARRIERS: as for the narrow sink.  prefetch and window keep their place, two barriers per
//     window, and every wave calls window once per window; the callers' trip counts come from the
//     destination's WIRE group count alone (gc, or a tile's range), which the widening does not
//     change, and the wide / narrow branch is on a scalar that every wave of the workgroup holds.
template <int NW, bool WIDE>
struct RedSinkT {
    static constexpr bool on = true;
    static constexpr uint32_t T = 64u * NW;                          // lanes of the workgroup
    static constexpr int NPFN = (int)((kRedWinGroups + T - 1) / T);  // groups per lane and window
    static constexpr int NPFW = (int)((2u * kRedWinGroups + T - 1) / T);  // ... of a wide destination
    static constexpr int NPF = WIDE ? NPFW : NPFN;
    uint8_t *stage;  // the workgroup's staged windows; peer k's slice at k * kRedSlice
    uint8_t *mine;   // this wave's slice
    uint8_t *dst;
    uint64_t osize;  // decoded (wire) bytes
    uint32_t gc;     // the end of the walk: the decoded size's 16-byte groups (the last may be partial), or a tile's end
    uint32_t gbase;  // the first group of the walk (0, or a tile's first group): window `win` starts kRedWinGroups * win past it
    uint32_t n_peers, elem, tid;
    bool set, dal16;
    uint4 dpre[NPF];  // the destination groups of the coming window (whole aligned groups, not under SET)

    // group j of the window from this wave's blob (lane l of round rl: j = 64 rl + l)
    __device__ __forceinline__ void put(uint32_t j, uint4 v) { *reinterpret_cast<uint4 *>(mine + 16u * j) = v; }

    __device__ __forceinline__ bool whole(uint32_t g) const { return dal16 && 16ull * g + 16ull <= osize; }

    // a wide destination: its bytes, the end of the walk in its groups, and whether group g is whole
    __device__ __forceinline__ uint64_t wsize() const { return 2ull * osize; }
    __device__ __forceinline__ uint32_t wend() const {
        const uint32_t a = 2u * gc, b = (uint32_t)((wsize() + 15ull) / 16ull);  // (osize < 2^34: red_header)
        return a < b ? a : b;
    }
    __device__ __forceinline__ bool wwhole(uint32_t g) const { return dal16 && 16ull * g + 16ull <= wsize(); }

    // the destination loads of window `win`, issued before its decode
    __device__ __forceinline__ void prefetch(uint32_t win) {
        if (set) return;
        if constexpr (WIDE) {
            if (red_wide(elem)) {
                if constexpr (NPFW > 2) dpre[2] = prefetch_wide(win, 2u, dpre[2]);
                if constexpr (NPFW > 1) dpre[1] = prefetch_wide(win, 1u, dpre[1]);
                dpre[0] = prefetch_wide(win, 0u, dpre[0]);
                return;
            }
        }
        if constexpr (NPFN > 1) dpre[1] = prefetch_group(win, 1u, dpre[1]);
        dpre[0] = prefetch_group(win, 0u, dpre[0]);
    }

    // The lane's groups are written out, last to first, on both walks, and a prefetch returns the
    // group it keeps.  With loops, or with stores under the tests, hipcc 7.2 merged the tails of the
    // two walks into stores through a pointer chosen between dpre's entries, which kept dpre in scratch
    // in the instances where the walks differ in length; ending both on dpre[0] leaves nothing to choose.
    static_assert(NPFN <= 2 && NPFW <= 3, "prefetch and window write the lane's groups out");
    __device__ __forceinline__ uint4 prefetch_group(uint32_t win, uint32_t q, uint4 pre) const {
        const uint32_t j = tid + q * T, g = gbase + win * kRedWinGroups + j;
        return j < kRedWinGroups && g < gc && whole(g) ? acc_ld16(dst + 16ull * g) : pre;
    }
    __device__ __forceinline__ uint4 prefetch_wide(uint32_t win, uint32_t q, uint4 pre) const {
        const uint32_t j = tid + q * T, g = 2u * (gbase + win * kRedWinGroups) + j;
        return j < 2u * kRedWinGroups && g < wend() && wwhole(g) ? acc_ld16(dst + 16ull * g) : pre;
    }

    // the sums of window `win` into a wide destination (BF: the wire is bf16, else fp16): the lane's
    // q-th group, `pre` its prefetched bytes
    template <bool BF>
    __device__ __forceinline__ void sum_wide_group(uint32_t win, uint32_t q, uint4 pre) {
        const uint32_t j = tid + q * T, g = 2u * (gbase + win * kRedWinGroups) + j;
        if (j < 2u * kRedWinGroups && g < wend()) {
            uint8_t *p = dst + 16ull * g;
            const bool wh = wwhole(g);
            const uint64_t left = wsize() - 16ull * g;
            const uint32_t valid = left >= 16ull ? 16u : (uint32_t)left;  // (4, 8 or 12 in the last group)
            const uint2 *sv = reinterpret_cast<const uint2 *>(stage + 8u * j);
            psy_f4 d = red_widen<BF>(sv[0]);
            if (!set) {
                uint4 b = pre;
                if (!wh) b = red_ld16w(p, valid);
                d = red_f4(b) + d;
            }
            for (uint32_t k = 1u; k < n_peers; ++k) d = d + red_widen<BF>(sv[k * (kRedSlice / 8u)]);
            const uint4 o = make_uint4(__float_as_uint(d.x), __float_as_uint(d.y), __float_as_uint(d.z), __float_as_uint(d.w));
            if (wh) st16_nt(p, o);
            else red_st16w(p, o, valid);
        }
    }
    template <bool BF>
    __device__ __forceinline__ void sum_wide(uint32_t win) {
        if constexpr (NPFW > 2) sum_wide_group<BF>(win, 2u, dpre[2]);
        if constexpr (NPFW > 1) sum_wide_group<BF>(win, 1u, dpre[1]);
        sum_wide_group<BF>(win, 0u, dpre[0]);
    }

    // the sums of window `win` in the destination's own type: the lane's q-th group
    __device__ __forceinline__ void sum_group(uint32_t win, uint32_t q, uint4 pre) {
        const uint32_t j = tid + q * T, g = gbase + win * kRedWinGroups + j;
        if (j < kRedWinGroups && g < gc) {
            uint8_t *p = dst + 16ull * g;
            const bool wh = whole(g);
            const uint64_t left = osize - 16ull * g;
            const uint32_t valid = left >= 16ull ? 16u : (uint32_t)left;
            const uint4 *sv = reinterpret_cast<const uint4 *>(stage + 16u * j);
            uint4 d = sv[0];
            if (!set) d = acc4(wh ? pre : red_ld16(p, valid), d, elem);
            for (uint32_t k = 1u; k < n_peers; ++k) d = acc4(d, sv[k * (kRedSlice / 16u)], elem);
            if (wh) st16_nt(p, d);
            else red_st16(p, d, valid);
        }
    }

    // the end of window `win`: every wave of the workgroup calls this once per window
    __device__ __forceinline__ void window(uint32_t win) {
        __syncthreads();  // A: every peer's slice of this window is staged
        bool done = false;
        if constexpr (WIDE) {
            if (elem == kElemF32FromBF16) sum_wide<true>(win), done = true;
            else if (elem == kElemF32FromF16) sum_wide<false>(win), done = true;
        }
        if (!done) {
            if constexpr (NPFN > 1) sum_group(win, 1u, dpre[1]);
            sum_group(win, 0u, dpre[0]);
        }
        __syncthreads();  // B: the slices may be written again
        prefetch(win + 1u);
    }
};
template <int NW>
using RedSink = RedSinkT<NW, false>;

// What every wave concludes from the peers' records (the same code over the same LDS words)
struct RedVerdict {
    uint32_t st;  // the destination's status
    bool fused;   // every peer is UNCP or a fast-path blob
    uint64_t osize;
};
__device__ __forceinline__ RedVerdict red_verdict(const uint32_t *rec, uint32_t n_peers) {
    RedVerdict v{ST_OK, true, 0};
    v.osize = *reinterpret_cast<const uint64_t *>(rec + 2);
    bool differ = false;
    for (uint32_t k = 0; k < n_peers; ++k) {
        const uint32_t kind = rec[4 * k], st = rec[4 * k + 1];
        if (v.st == ST_OK && st != ST_OK) v.st = st;  // the lowest-numbered failing peer
        if (kind == 0u) v.fused = false;
        if (*reinterpret_cast<const uint64_t *>(rec + 4 * k + 2) != v.osize) differ = true;
    }
    if (v.st == ST_OK && differ) v.st = ST_MISMATCH;
    // (the same in every lane and wave; kept in scalar registers, so the branches on them are scalar)
    v.st = (uint32_t)__builtin_amdgcn_readfirstlane((int)v.st);
    v.fused = __builtin_amdgcn_readfirstlane((int)v.fused) != 0;
    v.osize = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v.osize) |
              (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v.osize >> 32)) << 32;
    return v;
}

// The header phase of wave w < n_peers: peer w's blob of destination msg is parsed (parse_fast;
// blob_check for every other shape) and checked against the destination (capacity, the 2^35 limit,
// element alignment and size: acc_status); (kind, status, decoded size) go to the LDS record rec[4 w ..]
// and the status to peer_status.  hdrc: kHdrCache bytes of the wave's own LDS.  Shared by the
// one-workgroup kernel and the tiled form's prep pass, so both refuse and accept the same blobs.
//
// WIDE (the instances that take the widening codes; every other instance answers them TDT_E_ARG as any
// unknown code): under a widening code the decoded size w is the wire's and the destination holds 2 w
// bytes of fp32, so the capacity is held against 2 w, the destination must be 4-byte aligned and w
// even, and w < 2^34 keeps the destination's group indices in 32 bits.  The record's size stays w:
// TDT_E_MISMATCH is decided on decoded sizes.
struct RedHead {
    FastHdr H;
    const uint8_t *blob;
    uint64_t len;
};
template <bool WIDE>
__device__ __forceinline__ RedHead red_header(const ReduceArgs &a, uint32_t msg, uint32_t w, uint32_t elem, uint8_t *dst,
                                              uint64_t cap, uint8_t *hdrc, uint32_t *rec) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t bi = (uint64_t)w * a.n_msgs + msg;
    const uint8_t *blob = reinterpret_cast<const uint8_t *>(a.blobs[bi]);
    const uint64_t len = a.blob_len[bi];
    const uint32_t hcl = len < (uint64_t)kHdrCache ? (uint32_t)len : (uint32_t)kHdrCache;
    {
        static_assert(kHdrCache == 256, "one dword per lane");
        const uint32_t o = lane * 4u;
        uint32_t v = 0;
        if (((uintptr_t)blob & 3) == 0 && o + 4u <= hcl) {
            v = *reinterpret_cast<const uint32_t *>(blob + o);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                if (o + i < hcl) v |= (uint32_t)blob[o + i] << (8u * i);
        }
        reinterpret_cast<uint32_t *>(hdrc)[lane] = v;
    }
    team_sync<1>();
    const FastHdr H = parse_fast(blob, len, hdrc, hcl);
    uint32_t st = ST_OK;
    uint64_t osize = H.osize;
    if (H.kind == 0u) {
        // every other shape, errors included: the reference's checks (every lane the same words)
        auto rd32 = [&](uint64_t off) -> uint32_t {
            if (off + 4 <= hcl) return ld_u32_bytes(hdrc + off);
            return ld_u32_bytes(blob + off);
        };
        uint32_t uncp;
        st = blob_check(rd32, len, uncp, osize);
    }
    st = (uint32_t)__builtin_amdgcn_readfirstlane((int)st);
    const bool wide = WIDE && red_wide(elem);  // (uniform)
    if (st == ST_DEFER) {  // a generic word size: no accumulate form
        st = !wide && (elem > kElemMax || elem == kElemStore) ? (uint32_t)ST_ARG : (uint32_t)ST_UNSUPPORTED;
    } else if (wide) {
        if (st == ST_OK && osize > (cap >> 1)) st = ST_CAPACITY;  // (2 osize > cap)
        if (st == ST_OK && (osize >> 34) != 0) st = ST_UNSUPPORTED;
        if (st == ST_OK && ((((uintptr_t)dst & 3) | (osize & 1)) != 0)) st = ST_ELEMENT;
    } else {
        if (st == ST_OK && osize > cap) st = ST_CAPACITY;
        if (st == ST_OK && (osize >> 35) != 0) st = ST_UNSUPPORTED;  // (group indices are 32 bits wide)
        if (st == ST_OK && elem == kElemStore) st = ST_ARG;
        st = acc_status(st, elem, dst, osize);
    }
    if (st != ST_OK) osize = 0;
    if (lane == 0) {
        rec[4 * w] = H.kind;
        rec[4 * w + 1] = st;
        *reinterpret_cast<uint64_t *>(rec + 4 * w + 2) = osize;
        if (a.peer_status) a.peer_status[bi] = (int32_t)st;
    }
    return RedHead{H, blob, len};
}

// The one-workgroup kernel's body.  WIDE: an instance that also sums destinations with a widening
// code; its sink carries both sums, and a valid wide destination with a peer off the fast path is
// refused (TDT_E_UNSUPPORTED: the serial kernel sums through decode_one's ACC stores, which have no
// widening form) where a narrow one is left to the serial kernel.
template <int NW, bool WIDE>
__device__ __forceinline__ void red_one_workgroup(const ReduceArgs &a) {
    using Lay = RedLayout<NW>;
    using Dec = DecLayoutT<kRedWR>;
    __shared__ __attribute__((aligned(16))) uint8_t smem[Lay::BYTES];
    const uint32_t msg = blockIdx.x;
    if (a.mark && a.mark[msg]) return;  // (uniform) the tile pass sums it
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t n_peers = a.n_peers;
    uint8_t *dec = smem + w * (uint32_t)Lay::DEC;
    uint32_t *rec = reinterpret_cast<uint32_t *>(smem + Lay::OFF_REC);
    const bool set = (a.flags & kRedSet) != 0u;
    const uint32_t elem =
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(a.elem_codes ? (uint32_t)a.elem_codes[msg] : a.elem));
    uint8_t *dst = reinterpret_cast<uint8_t *>(a.outs[msg]);
    const uint64_t cap = a.out_cap[msg];

    // ------------------------------------------------ header: wave k checks peer k's blob
    RedHead P{};
    if (w < n_peers) P = red_header<WIDE>(a, msg, w, elem, dst, cap, dec + Dec::OFF_HDR, rec);
    const FastHdr &H = P.H;
    const uint8_t *const blob = P.blob, *const blim = P.blob + P.len;
    __syncthreads();  // header barrier: every wave, once
    const bool wide = WIDE && red_wide(elem);
    RedVerdict V = red_verdict(rec, n_peers);
    if (wide && V.st == ST_OK && !V.fused) V.st = ST_UNSUPPORTED;
    if (w == 0 && lane == 0) {
        // (a valid destination with a peer off the fast path: left to the serial kernel that follows)
        a.status[msg] = (int32_t)(V.st == ST_OK && !V.fused ? ST_RED_SERIAL : V.st);
        if (a.out_len) a.out_len[msg] = V.st == ST_OK ? (wide ? 2ull * V.osize : V.osize) : 0;
    }
    if (V.st != ST_OK || !V.fused) return;  // refused: nothing of the destination is read or written

    // ------------------------------------------------ fused
    const uint64_t osize = V.osize;
    const uint32_t gc = (uint32_t)((osize + 15) / 16);
    const uint32_t nwin = (gc + kRedWinGroups - 1) / kRedWinGroups;
    using Sink = RedSinkT<NW, WIDE>;
    Sink S;
    S.stage = smem + Lay::OFF_STAGE;
    S.mine = S.stage + w * kRedSlice;
    S.dst = dst;
    S.osize = osize;
    S.gc = gc;
    S.gbase = 0u;
    S.n_peers = n_peers;
    S.elem = elem;
    S.tid = threadIdx.x;
    S.set = set;
    S.dal16 = ((uintptr_t)dst & 15) == 0;
#pragma unroll
    for (int q = 0; q < Sink::NPF; ++q) S.dpre[q] = make_uint4(0, 0, 0, 0);
    S.prefetch(0);
    const uint32_t kind = (uint32_t)__builtin_amdgcn_readfirstlane((int)(w < n_peers ? H.kind : 0u));
    if (kind == 2u) {
        // window loop inside: gwin = 0, 64 WR, ... < gc, S.window(win) at the end of each
        const uint64_t wbytes = (uint64_t)(H.orig / H.ws) * H.ws;
        decode_fast<kRedWR, false, Sink>(H, dec, blob, blim, nullptr, gc, wbytes, 0, gc, nullptr, nullptr, nullptr, 0u, 0u,
                                         &S);
    } else if (kind == 1u) {
        for (uint32_t win = 0; win < nwin; ++win) {
#pragma unroll
            for (uint32_t rl = 0; rl < (uint32_t)kRedWR; ++rl) {
                const uint32_t g = win * kRedWinGroups + rl * 64u + lane;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (g < gc) {
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
template <int NW>
__global__ __launch_bounds__(64 * NW) void tdt_decode_reduce_kernel(ReduceArgs a) {
    red_one_workgroup<NW, false>(a);
}
// (launched when the call's codes may widen: a widening `elem`, or codes per destination)
template <int NW>
__global__ __launch_bounds__(64 * NW) void tdt_decode_reduce_wide_kernel(ReduceArgs a) {
    red_one_workgroup<NW, true>(a);
}

// The serial path: the destinations the kernel above marked ST_RED_SERIAL (every blob valid, the
// sizes equal, some peer no fast-path blob).  One wave per block; a wave reads 64 statuses at a
// time, and for each marked destination runs the one-wave accumulate decode (decode_one, ACC) over
// the peers in order, adding straight into the destination; under TDT_REDUCE_SET peer 0 is stored.
// Then the status becomes TDT_OK.  A launch of its own, so that the fused kernel keeps its registers:
// with decode_one inlined beside decode_fast hipcc 7.2 either crashed (SimplifyCFG) or, behind a
// call, gave the fused path the callee's 184 VGPRs and a stack.
__global__ void tdt_decode_reduce_serial_kernel(ReduceArgs a);
#ifdef PSY_DEC_REDUCE_TU
// (behind a call: inlined into the loop below, hipcc 7.2's SimplifyCFG crashes on this instance)
__device__ __noinline__ void red_decode_one(const DecodeArgs &d, uint8_t *smem) {
    decode_one<0, kRedWR, true, true>(d, smem, 0);
}
__global__ __launch_bounds__(64) void tdt_decode_reduce_serial_kernel(ReduceArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[DecLayoutT<kRedWR>::BYTES];
    __shared__ uint64_t tab[4];  // the one-message tables: blob, length, slot begin, slot end
    const uint32_t lane = (uint32_t)lane_id();
    const bool set = (a.flags & kRedSet) != 0u;
    DecodeArgs d{};
    d.n_msgs = 1;
    d.in_off = tab;
    d.in_len = tab + 1;
    d.slot_off = tab + 2;
    for (uint32_t base = blockIdx.x * 64u; base < a.n_msgs; base += gridDim.x * 64u) {
        const uint32_t i = base + lane;
        uint64_t pend = __ballot(i < a.n_msgs && a.status[i] == (int32_t)ST_RED_SERIAL);
        while (pend) {
            const uint32_t msg = base + (uint32_t)__builtin_ctzll(pend);
            pend &= pend - 1;
            const uint32_t elem =
                (uint32_t)__builtin_amdgcn_readfirstlane((int)(a.elem_codes ? (uint32_t)a.elem_codes[msg] : a.elem));
            for (uint32_t k = 0; k < a.n_peers; ++k) {
                team_sync<1>();  // (the previous decode is done with the LDS)
                if (lane == 0) {
                    tab[0] = a.blobs[(uint64_t)k * a.n_msgs + msg];
                    tab[1] = a.blob_len[(uint64_t)k * a.n_msgs + msg];
                    tab[2] = a.outs[msg];
                    tab[3] = a.outs[msg] + a.out_cap[msg];
                }
                team_sync<1>();
                d.elem = set && k == 0 ? kElemStore : elem;
                red_decode_one(d, smem);
            }
            if (lane == 0) a.status[msg] = (int32_t)ST_OK;
        }
    }
}
#endif

#define PSY_DEC_REDUCE_INSTANCES(X)           \
    X(psy::tdt_decode_reduce_kernel<2>)       \
    X(psy::tdt_decode_reduce_kernel<4>)       \
    X(psy::tdt_decode_reduce_kernel<8>)       \
    X(psy::tdt_decode_reduce_wide_kernel<2>)  \
    X(psy::tdt_decode_reduce_wide_kernel<4>)  \
    X(psy::tdt_decode_reduce_wide_kernel<8>)

}  // namespace psy
