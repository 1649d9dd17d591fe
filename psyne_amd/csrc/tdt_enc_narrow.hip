// tdt_enc_narrow.hip — the encode-narrow kernel (tdt_encode_narrow_v, tdt_enc_narrow.h) and its
// launcher.  A translation unit of its own, compiled beside the others (psyne_amd/build.py) without
// packed fp32 forms.
//
// Reference lines restated here (include/psyne/protocol/tdt_compression.hpp), as tdt_anyws.hip:
//   should_transform :186-201, compress_tdt :363-399 (size guard :364-367), calculate_entropy
//   :470-480, perform_clustering :507-525, separate_byte_streams :527-549, simple_rle_compress
//   :557-582, serialize :81-117.
// (the headers' non-template kernels are defined once, in tdt_api.hip)
#define PSY_ENC_INST_TU 1
#include "tdt_enc_narrow.h"

#include <algorithm>

#include "tdt_encode.h"
#include "tdt_entropy.h"

// The mapping decision is bit-exact only if nothing below is contracted (tdt_log2.h).
#pragma clang fp contract(off)

namespace psy {
namespace {

constexpr int kNW = kNarTeam / 64;  // waves per workgroup
static_assert(kNarResident % kNarStep == 0 && kNarStep == 16u * kNarTeam, "a chunk is whole steps of 16 bytes per lane");
// a step's staged pairs: one per byte, the full pairs of the runs that began in it (their lengths sum
// to at most the step) and of the run that entered it
constexpr uint32_t kNarStagePairs = kNarStep + kNarStep / 255u + 1u + kNarLaneFull;
static_assert(2u * kNarStagePairs + 8u <= 4u * kNarHistCopies * 512u, "the stage reuses the histogram copies (+ a dword of slack)");

struct NarCarry {     // uniform, carried across steps and chunks
    uint32_t cstart;  // last run start + 1 (0: none yet)
    uint32_t cpairs;  // pairs so far
    uint32_t lastb;   // the last stream byte so far
};
struct NarBig {           // a closed run of more than kNarLaneFull full pairs (at most one per step)
    uint32_t full, val;   // how many 255-count pairs, of which value
    uint32_t hs;          // pairs staged before them
};

// ---- the narrowing rule (psyne_tdt.h), u the fp32 bit pattern
__device__ __forceinline__ uint32_t nar_bf16(uint32_t u) {
    const uint32_t r = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;  // nearest even; overflow reaches infinity by the carry
    return (u & 0x7fffffffu) > 0x7f800000u ? ((u >> 16) | 0x0040u) : r;
}
__device__ __forceinline__ uint32_t nar_f16(uint32_t u) {
    // v_cvt_f16_f32: nearest even, subnormal results kept, infinity past the largest finite value;
    // its NaN is replaced by the rule's
    const uint32_t r = (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)__uint_as_float(u));
    const uint32_t nan = ((u >> 16) & 0x8000u) | 0x7e00u | ((u >> 13) & 0x3ffu);
    return (u & 0x7fffffffu) > 0x7f800000u ? nan : r;
}

// Elements e .. e + 3 of the source (4-byte aligned); those at or past ne read as 0 and are not touched.
__device__ __forceinline__ void nar_load4(const uint8_t *src, uint64_t e, uint64_t ne, uint32_t (&u)[4]) {
    const uint8_t *p = src + 4ull * e;
    if (e + 4 <= ne) {
        if (((uintptr_t)p & 15) == 0) {
            const psy_u32x4 v = gload<psy_u32x4>(p);
            u[0] = v.x, u[1] = v.y, u[2] = v.z, u[3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) u[i] = gload<uint32_t>(p + 4 * i);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = e + i < ne ? gload<uint32_t>(p + 4 * i) : 0u;
    }
}

// Four elements narrowed: h01 / h23 hold the halfwords of elements 0, 1 / 2, 3
__device__ __forceinline__ void nar_narrow4(const uint32_t (&u)[4], bool bf, uint32_t &h01, uint32_t &h23) {
    uint32_t h[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = bf ? nar_bf16(u[i]) : nar_f16(u[i]);
    h01 = h[0] | (h[1] << 16);
    h23 = h[2] | (h[3] << 16);
}

// Elements [eb, eb + cnt) of the source into the planes (cnt <= kNarResident; the planes' bytes past
// cnt are left as they are); HIST: counted into this lane's copy of the bins.
template <bool HIST>
__device__ __forceinline__ void nar_stage(const uint8_t *src, uint64_t eb, uint32_t cnt, bool bf, uint8_t *s_pl, uint32_t *s_hist) {
    uint32_t *p0 = reinterpret_cast<uint32_t *>(s_pl), *p1 = reinterpret_cast<uint32_t *>(s_pl + kNarResident);
    uint32_t *h = s_hist + (threadIdx.x & (kNarHistCopies - 1u)) * 512u;
#pragma unroll 2
    for (uint32_t k = threadIdx.x; 4u * k < cnt; k += kNarTeam) {
        uint32_t u[4], h01, h23;
        nar_load4(src, eb + 4ull * k, eb + cnt, u);
        nar_narrow4(u, bf, h01, h23);
        const uint32_t lo = perm(h23, h01, 0x06040200u), hi = perm(h23, h01, 0x07050301u);
        p0[k] = lo;
        p1[k] = hi;
        if constexpr (HIST) {
            const uint32_t valid = cnt - 4u * k >= 4u ? 4u : cnt - 4u * k;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                if (i < valid) atomicAdd(&h[(lo >> (8u * i)) & 0xffu], 1u);
            if (valid == 4u && hi == (hi & 0xffu) * 0x01010101u) {
                atomicAdd(&h[256u + (hi & 0xffu)], 4u);
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i)
                    if (i < valid) atomicAdd(&h[256u + ((hi >> (8u * i)) & 0xffu)], 1u);
            }
        }
    }
}

// nb bytes of the stage from byte sb on → the blob at A: byte stores up to A's next dword boundary
// and behind the last whole dword, dword stores between (the stage is read as two aligned dwords
// and shifted; it has a dword of slack behind it)
__device__ __forceinline__ void nar_flush(uint8_t *A, const uint32_t *s_stage, uint32_t sb, uint32_t nb) {
    const uint32_t tid = threadIdx.x;
    const uint8_t *sbytes = reinterpret_cast<const uint8_t *>(s_stage);
    uint32_t head = (4u - (uint32_t)((uintptr_t)A & 3u)) & 3u;
    if (head > nb) head = nb;
    if (tid < head) A[tid] = sbytes[sb + tid];
    const uint32_t body = (nb - head) / 4u;
    uint32_t *Aw = reinterpret_cast<uint32_t *>(A + head);
    for (uint32_t k = tid; k < body; k += kNarTeam) {
        const uint32_t b = sb + head + 4u * k;
        Aw[k] = __builtin_amdgcn_alignbyte(s_stage[(b >> 2) + 1u], s_stage[b >> 2], b & 3u);
    }
    const uint32_t done = head + 4u * body;
    if (tid < nb - done) A[done + tid] = sbytes[sb + done + tid];
}

// cnt pairs (255, val) at A by the whole workgroup, dword stores between the unaligned edges
__device__ __forceinline__ void nar_fill(uint8_t *A, uint32_t cnt, uint32_t val) {
    const uint32_t tid = threadIdx.x;
    const uint64_t nb = 2ull * cnt;
    uint64_t head = (4u - (uint32_t)((uintptr_t)A & 3u)) & 3u;
    if (head > nb) head = nb;
    if (tid < head) A[tid] = (uint8_t)(tid & 1u ? val : 255u);
    const uint32_t even = 0x00ff00ffu | (val << 8) | (val << 24), odd = 0xff00ff00u | val | (val << 16);
    const uint32_t pat = head & 1u ? odd : even;
    const uint64_t body = (nb - head) / 4u;
    uint32_t *Aw = reinterpret_cast<uint32_t *>(A + head);
    for (uint64_t k = tid; k < body; k += kNarTeam) Aw[k] = pat;
    const uint64_t done = head + 4u * body;
    if (tid < nb - done) A[done + tid] = (uint8_t)((done + tid) & 1u ? val : 255u);
}

// One step of one stream: the lane's 16 stream bytes from the planes, SWAR run starts, the two team
// scans; EMIT: the step's pairs staged at their rank and flushed to `pairs` (the stream's pairs in
// the blob).  inter: the one stream of mapping [0,0], byte i = plane i & 1, index i >> 1; else the
// stream is plane `plane`.  Q: the step's first stream index, lq: the same within the staged chunk,
// Lc: its bytes (1 .. kNarStep).
template <bool EMIT>
__device__ __forceinline__ void nar_step(const uint8_t *s_pl, bool inter, uint32_t plane, uint32_t Q, uint32_t lq, uint32_t Lc,
                                         NarCarry &c, uint8_t *pairs, uint32_t *s_stage, uint32_t (*s_slots)[kNW], NarBig *s_big) {
    const uint32_t tid = threadIdx.x;
    const uint32_t q0 = 16u * tid, l0 = lq + q0;
    const uint32_t m = q0 >= Lc ? 0u : (Lc - q0 >= 16u ? 16u : Lc - q0);
    uint32_t x[4], prev;
    if (inter) {
        const uint2 lo = *reinterpret_cast<const uint2 *>(s_pl + (l0 >> 1));
        const uint2 hi = *reinterpret_cast<const uint2 *>(s_pl + kNarResident + (l0 >> 1));
        x[0] = perm(hi.x, lo.x, 0x05010400u);
        x[1] = perm(hi.x, lo.x, 0x07030602u);
        x[2] = perm(hi.y, lo.y, 0x05010400u);
        x[3] = perm(hi.y, lo.y, 0x07030602u);
        prev = l0 ? s_pl[kNarResident + (l0 >> 1) - 1u] : c.lastb;  // (the byte before an even index is a high byte)
        const uint32_t le = lq + Lc - 1u;
        c.lastb = s_pl[(le & 1u) * kNarResident + (le >> 1)];
    } else {
        const uint4 v = *reinterpret_cast<const uint4 *>(s_pl + plane * kNarResident + l0);
        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
        prev = l0 ? s_pl[plane * kNarResident + l0 - 1u] : c.lastb;
        c.lastb = s_pl[plane * kNarResident + lq + Lc - 1u];
    }
    if constexpr (EMIT) {
        if (tid == 0) s_big->full = 0u;  // (every lane has read the step before's behind the flush's barriers)
    }
    // simple_rle_compress :557-582 as any_chunk (tdt_anyws.hip) has it: a stream byte that differs from
    // the one before it starts a run and closes the run before it
    uint32_t sm = neq_prev_mask4(x[0], prev << 24) | (neq_prev_mask4(x[1], x[0]) << 4) | (neq_prev_mask4(x[2], x[1]) << 8) |
                  (neq_prev_mask4(x[3], x[2]) << 12);
    if (Q + q0 == 0u) sm |= 1u;  // the stream's first byte
    sm &= (1u << m) - 1u;
    uint32_t vmax[1] = {sm ? Q + q0 + (31u - (uint32_t)__builtin_clz(sm)) + 1u : 0u}, tmax[1];
    team_excl_scan<kNW, 1, OpMax>(vmax, tmax, s_slots[0]);
    const uint32_t cur = vmax[0] > c.cstart ? vmax[0] : c.cstart;  // run start + 1 entering this lane
    // only a lane's first run start can close a run longer than its 16 bytes
    uint32_t first_full = 0u, first_rem = 0u, np = 0u;
    bool big = false;
    if (sm) {
        const uint32_t i0 = (uint32_t)__builtin_ctz(sm), qf = Q + q0 + i0;
        np = (uint32_t)__builtin_popcount(sm);
        if (qf == 0u) {
            --np;  // nothing before the stream's first byte
        } else {
            const uint32_t Lr = qf - (cur - 1u);
            first_full = (Lr - 1u) / 255u;
            first_rem = Lr - 255u * first_full;
            big = EMIT && first_full > kNarLaneFull;
            if (big) {  // its full pairs are the whole workgroup's
                s_big->full = first_full;
                const uint32_t d = (i0 - 1u) >> 2, xd = d == 0u ? x[0] : d == 1u ? x[1] : d == 2u ? x[2] : x[3];
                s_big->val = i0 ? (xd >> (8u * ((i0 - 1u) & 3u))) & 0xffu : prev;  // (the byte before the run start)
            } else {
                np += first_full;
            }
        }
    }
    uint32_t vadd[1] = {np}, tadd[1];
    team_excl_scan<kNW, 1, OpAdd>(vadd, tadd, s_slots[1]);
    uint32_t extra = 0u;
    if constexpr (EMIT) {
        uint16_t *st = reinterpret_cast<uint16_t *>(s_stage);
        if (sm) {
            uint32_t si = vadd[0];
            uint32_t rs = cur;  // start + 1 of the run being closed
            bool first = true;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (!((sm >> i) & 1u)) continue;
                const uint32_t q = Q + q0 + (uint32_t)i;
                const uint32_t val = i ? (x[(i - 1) >> 2] >> (8 * ((i - 1) & 3))) & 0xffu : prev;
                if (q != 0u) {
                    uint32_t cnt = q - (rs - 1u);
                    if (first) {
                        if (!big)
                            for (uint32_t f = 0; f < first_full; ++f) st[si++] = (uint16_t)(255u | (val << 8));
                        cnt = first_rem;
                    }
                    st[si++] = (uint16_t)(cnt | (val << 8));
                }
                first = false;
                rs = q + 1u;
            }
            if (big) s_big->hs = vadd[0];
        }
        __syncthreads();
        const uint32_t full = s_big->full;
        uint8_t *A = pairs + 2ull * c.cpairs;
        if (!full) {
            nar_flush(A, s_stage, 0u, 2u * tadd[0]);
        } else {  // (uniform) the pairs before the long run, its full pairs, the rest
            const uint32_t hs = s_big->hs;
            nar_flush(A, s_stage, 0u, 2u * hs);
            nar_fill(A + 2ull * hs, full, s_big->val);
            nar_flush(A + 2ull * hs + 2ull * full, s_stage, 2u * hs, 2u * (tadd[0] - hs));
            extra = full;
        }
        __syncthreads();  // (the next step restages)
    }
    c.cstart = tmax[0] > c.cstart ? tmax[0] : c.cstart;
    c.cpairs += tadd[0] + extra;
}

// The UNCP form: the marker and the w = 2 ne narrowed bytes, 16 per lane and store.  staged: the
// planes hold the whole message (ne <= kNarResident); else it is narrowed from the source again.
__device__ __forceinline__ void nar_uncp(uint8_t *dst, const uint8_t *src, uint64_t ne, bool bf, bool staged, const uint8_t *s_pl) {
    const uint32_t tid = threadIdx.x;
    const uint64_t w = 2ull * ne;
    if (tid < 4) dst[tid] = (uint8_t)(kMagicUNCP >> (8 * tid));
    for (uint64_t g = tid; 16ull * g < w; g += kNarTeam) {
        const int valid = w - 16ull * g >= 16 ? 16 : (int)(w - 16ull * g);
        uint4 v;
        if (staged) {
            const uint2 lo = *reinterpret_cast<const uint2 *>(s_pl + 8u * (uint32_t)g);
            const uint2 hi = *reinterpret_cast<const uint2 *>(s_pl + kNarResident + 8u * (uint32_t)g);
            v = make_uint4(perm(hi.x, lo.x, 0x05010400u), perm(hi.x, lo.x, 0x07030602u), perm(hi.y, lo.y, 0x05010400u),
                           perm(hi.y, lo.y, 0x07030602u));
        } else {
            uint32_t u[4];
            nar_load4(src, 8ull * g, ne, u);
            nar_narrow4(u, bf, v.x, v.y);
            nar_load4(src, 8ull * g + 4, ne, u);
            nar_narrow4(u, bf, v.z, v.w);
        }
        st16_any(dst + 4 + 16ull * g, v, valid);
    }
}

__global__ __launch_bounds__(kNarTeam) void tdt_encode_narrow_kernel(NarrowArgs a, uint32_t base) {
    __shared__ __attribute__((aligned(16))) uint8_t s_pl[2 * kNarResident];
    __shared__ __attribute__((aligned(16))) uint32_t s_un[kNarHistCopies * 512];  // the histogram copies, then the pair stage
    __shared__ double s_ent[2];
    __shared__ uint32_t s_slots[2][kNW];
    __shared__ NarBig s_big;

    const uint32_t tid = threadIdx.x, lane = (uint32_t)lane_id(), wv = tid >> 6;
    const uint32_t msg = base + blockIdx.x;
    if (msg >= a.n_msgs) return;
    const uint32_t code = a.elem_codes ? (uint32_t)a.elem_codes[msg] : a.elem;
    const uint64_t srca = a.msgs[msg], size = a.sizes[msg], cap = a.blob_cap[msg];
    const uint8_t *src = reinterpret_cast<const uint8_t *>(srca);
    uint8_t *dst = reinterpret_cast<uint8_t *>(a.blobs[msg]);
    auto report = [&](int32_t st, uint64_t len) __attribute__((always_inline)) {
        if (tid == 0) {
            if (a.status) a.status[msg] = st;
            if (a.out_len) a.out_len[msg] = len;
        }
    };
    // every refusal precedes the first store
    if (code != kNarBF16 && code != kNarF16) return report(ST_ARG, 0);
    if ((srca & 3u) || (size & 3u)) return report(kNarStElement, 0);
    const bool bf = code == kNarBF16;
    const uint64_t ne = size / 4, w = size / 2;  // elements, wire bytes
    // should_transform :186-201 and compress_tdt's size guard :364-367 on the wire size, at word size 2
    const bool compress = a.policy_on && w >= a.min_tensor && (w % 4 == 0) && w >= 64 && w < (1ull << 32);
    if (!compress) {
        const bool fits = w + 4 <= cap;
        report(fits ? ST_OK : ST_CAPACITY, fits ? w + 4 : 0);
        if (fits) nar_uncp(dst, src, ne, bf, false, s_pl);
        return;
    }
    const uint32_t ne32 = (uint32_t)ne, w32 = (uint32_t)w;
    const bool resident = ne32 <= kNarResident;

    // ---- H: planes and histograms (extract_features :441-446, every word)
    for (uint32_t i = tid; i < kNarHistCopies * 512u; i += kNarTeam) s_un[i] = 0u;
    __syncthreads();
    for (uint32_t eb = 0; eb < ne32; eb += kNarResident)
        nar_stage<true>(src, eb, ne32 - eb < kNarResident ? ne32 - eb : kNarResident, bf, s_pl, s_un);
    __syncthreads();
    // ---- M: entropies, then perform_clustering :507-525: entropy > in-order sum / 2
    if (wv < 2u) {
        uint32_t cb[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t r = 0; r < kNarHistCopies; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) cb[k] += s_un[r * 512u + wv * 256u + 64u * k + lane];
        const double e = any_entropy(cb, (double)ne32);
        if (lane == 0) s_ent[wv] = e;
    }
    __syncthreads();
    double sum = 0.0;
    sum += s_ent[0];
    sum += s_ent[1];
    const double thr = sum / 2.0;
    const uint32_t m0 = (uint32_t)__builtin_amdgcn_readfirstlane(s_ent[0] > thr ? 1 : 0);  // (uniform: every lane ran the same chain)
    const uint32_t m1 = (uint32_t)__builtin_amdgcn_readfirstlane(s_ent[1] > thr ? 1 : 0);
    const uint32_t ns = (m0 | m1) ? 2u : 1u;  // separate_byte_streams :527-549: max(mapping) + 1
    const bool inter = ns == 1u;              // [0,0]: the one stream is the message
    const uint32_t S = inter ? w32 : ne32;    // bytes of a stream

    // one pass over the chunks and both streams; EMIT: pairs[s] is where stream s's pairs go
    auto pass = [&](auto emit_tag, uint8_t *const (&pairs)[2], uint32_t (&total)[2]) __attribute__((always_inline)) {
        constexpr bool EMIT = decltype(emit_tag)::value;
        NarCarry c[2] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
        for (uint32_t eb = 0; eb < ne32; eb += kNarResident) {
            const uint32_t cnt = ne32 - eb < kNarResident ? ne32 - eb : kNarResident;
            if (!resident) {
                __syncthreads();  // (the chunk before is read)
                nar_stage<false>(src, eb, cnt, bf, s_pl, s_un);
                __syncthreads();
            }
#pragma unroll
            for (uint32_t s = 0; s < 2; ++s) {
                if (s >= ns) continue;
                const uint32_t plane = m0 ? 1u - s : s;  // stream 0 holds the positions mapped to 0
                const uint32_t Qb = inter ? 2u * eb : eb, Ls = inter ? 2u * cnt : cnt;
                for (uint32_t lq = 0; lq < Ls; lq += kNarStep)
                    nar_step<EMIT>(s_pl, inter, plane, Qb + lq, lq, Ls - lq < kNarStep ? Ls - lq : kNarStep, c[s], pairs[s], s_un,
                                   s_slots, &s_big);
            }
        }
        // the last run closes at the end of the stream
#pragma unroll
        for (uint32_t s = 0; s < 2; ++s) {
            if (s >= ns) continue;
            const uint32_t Lr = S - (c[s].cstart - 1u);
            const uint32_t full = (Lr - 1u) / 255u;
            if constexpr (EMIT) {
                uint8_t *A = pairs[s] + 2ull * c[s].cpairs;
                nar_fill(A, full, c[s].lastb);
                if (tid == 0) {
                    A[2ull * full] = (uint8_t)(Lr - 255u * full);
                    A[2ull * full + 1] = (uint8_t)c[s].lastb;
                }
            }
            total[s] = c[s].cpairs + full + 1u;
        }
    };

    // ---- C: both streams' pairs, and with them the blob's length and stream 1's place
    uint32_t P[2] = {0u, 0u}, Pe[2] = {0u, 0u};
    uint8_t *const none[2] = {nullptr, nullptr};
    pass(std::false_type{}, none, P);
    const uint64_t o1 = 32 + 2ull * P[0];                               // stream 1's length word
    const uint64_t Etdt = ns == 2u ? o1 + 4 + 2ull * P[1] : o1;         // header 28, length word(s), pairs
    const bool raw = a.raw_fallback && Etdt > w + 4;                    // TDT_OPT_RAW_FALLBACK
    const uint64_t E = raw ? w + 4 : Etdt;
    const bool fits = E <= cap;
    report(fits ? ST_OK : ST_CAPACITY, fits ? E : 0);
    if (!fits) return;
    if (raw) {
        nar_uncp(dst, src, ne, bf, resident, s_pl);
        return;
    }
    // ---- E: header (serialize :81-117): magic, original size, streams, word size, mapping; length words
    if (tid < 36u) {
        const uint32_t k = tid >> 2;
        const uint32_t hv = k == 0 ? kMagicTDT : k == 1 ? w32 : k == 2 ? ns : k == 3 ? 2u : k == 4 ? 2u : k == 5 ? m0 : k == 6 ? m1
                          : k == 7 ? 2u * P[0] : 2u * P[1];
        const uint64_t at = k < 8u ? tid : o1 + (tid & 3u);
        if (k < 8u || ns == 2u) dst[at] = (uint8_t)(hv >> (8u * (tid & 3u)));
    }
    uint8_t *const pairs[2] = {dst + 32, dst + o1 + 4};
    pass(std::true_type{}, pairs, Pe);
}

}  // namespace

int launch_encode_narrow(const NarrowArgs &a, hipStream_t s) {
    // one workgroup per message; a launch holds < 2^32 threads
    const uint32_t maxb = 0xffffffffu / kNarTeam;
    for (uint32_t b = 0; b < a.n_msgs; b += maxb)
        hipLaunchKernelGGL(tdt_encode_narrow_kernel, dim3(std::min(maxb, a.n_msgs - b)), dim3(kNarTeam), 0, s, a, b);
    return (int)hipGetLastError();
}

}  // namespace psy
