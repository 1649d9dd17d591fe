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
#include "tdt_enc_narrow_tiled.h"

#include <algorithm>

#include "tdt_anyws_tiles.h"
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

// ---- error feedback (psyne_tdt.h, tdt_encode_narrow_ef_v): the value narrowed is v = g + r
// Elements e .. e + 3 of v; EF and a residual: the source plus the residual, one v_add_f32 each (subnormals
// kept: the kernels' float mode); else the source as it is.
template <bool EF>
__device__ __forceinline__ void nar_value4(const uint8_t *src, const uint8_t *res, uint64_t e, uint64_t ne, uint32_t (&u)[4]) {
    nar_load4(src, e, ne, u);
    if constexpr (EF) {
        if (res) {  // (uniform)
            uint32_t r[4];
            nar_load4(res, e, ne, r);
#pragma unroll
            for (int i = 0; i < 4; ++i) u[i] = __float_as_uint(__uint_as_float(u[i]) + __uint_as_float(r[i]));
        }
    }
}
// r' = v - widen(h) of elements e .. e + 3 (u: v's bit patterns, h01 / h23: nar_narrow4's) to the residual,
// bit pattern 0 where h is an infinity or a NaN; those at or past ne are not touched.
__device__ __forceinline__ void nar_resid4(uint8_t *res, uint64_t e, uint64_t ne, const uint32_t (&u)[4], bool bf, uint32_t h01,
                                           uint32_t h23) {
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t h = ((i < 2 ? h01 : h23) >> (16 * (i & 1))) & 0xffffu;
        const uint32_t wide = bf ? h << 16 : __float_as_uint((float)__builtin_bit_cast(_Float16, (uint16_t)h));
        const uint32_t ex = bf ? 0x7f80u : 0x7c00u;
        o[i] = (h & ex) == ex ? 0u : __float_as_uint(__uint_as_float(u[i]) - __uint_as_float(wide));
    }
    uint8_t *p = res + 4ull * e;
    if (e + 4 <= ne && ((uintptr_t)p & 15) == 0) {
        psy_u32x4 t;
        t.x = o[0], t.y = o[1], t.z = o[2], t.w = o[3];
        *(__attribute__((address_space(1))) psy_u32x4 *)(p) = t;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (e + i < ne) *(__attribute__((address_space(1))) uint32_t *)(p + 4 * i) = o[i];
    }
}
// The resident form's last pass: v again from one more read of the source and the residual, r' stored.
__device__ __forceinline__ void nar_resid_pass(const uint8_t *src, uint8_t *res, uint32_t ne, bool bf) {
    for (uint32_t k = threadIdx.x; 4u * k < ne; k += kNarTeam) {
        uint32_t u[4], h01, h23;
        nar_value4<true>(src, res, 4ull * k, ne, u);
        nar_narrow4(u, bf, h01, h23);
        nar_resid4(res, 4ull * k, ne, u, bf, h01, h23);
    }
}

// Elements [eb, eb + cnt) of the source into the planes (cnt <= kNarResident; the planes' bytes past
// cnt are left as they are); HIST: counted into this lane's copy of the bins.  EF: of source + residual
// (nar_value4); WR: this is the last read of these elements, and r' is stored behind it.
template <bool HIST, bool EF = false, bool WR = false>
__device__ __forceinline__ void nar_stage(const uint8_t *src, uint8_t *res, uint64_t eb, uint32_t cnt, bool bf, uint8_t *s_pl,
                                          uint32_t *s_hist) {
    uint32_t *p0 = reinterpret_cast<uint32_t *>(s_pl), *p1 = reinterpret_cast<uint32_t *>(s_pl + kNarResident);
    uint32_t *h = s_hist + (threadIdx.x & (kNarHistCopies - 1u)) * 512u;
#pragma unroll 2
    for (uint32_t k = threadIdx.x; 4u * k < cnt; k += kNarTeam) {
        uint32_t u[4], h01, h23;
        nar_value4<EF>(src, res, eb + 4ull * k, eb + cnt, u);
        nar_narrow4(u, bf, h01, h23);
        if constexpr (EF && WR) {
            if (res) nar_resid4(res, eb + 4ull * k, eb + cnt, u, bf, h01, h23);
        }
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

// The 16-byte groups [g0, g1) of the w = 2 ne narrowed bytes behind the marker, one per lane and store.
// staged: the planes hold the whole message (ne <= kNarResident); else it is narrowed from the source again
// (EF: from source + residual, and r' of the groups' elements is stored: the last read of them).
template <bool EF = false>
__device__ __forceinline__ void nar_uncp_groups(uint8_t *dst, const uint8_t *src, uint8_t *res, uint64_t ne, bool bf, bool staged,
                                                const uint8_t *s_pl, uint64_t g0, uint64_t g1) {
    const uint64_t w = 2ull * ne;
    for (uint64_t g = g0 + threadIdx.x; g < g1; g += kNarTeam) {
        const int valid = w - 16ull * g >= 16 ? 16 : (int)(w - 16ull * g);
        uint4 v;
        if (staged) {
            const uint2 lo = *reinterpret_cast<const uint2 *>(s_pl + 8u * (uint32_t)g);
            const uint2 hi = *reinterpret_cast<const uint2 *>(s_pl + kNarResident + 8u * (uint32_t)g);
            v = make_uint4(perm(hi.x, lo.x, 0x05010400u), perm(hi.x, lo.x, 0x07030602u), perm(hi.y, lo.y, 0x05010400u),
                           perm(hi.y, lo.y, 0x07030602u));
        } else {
            uint32_t u[4];
            nar_value4<EF>(src, res, 8ull * g, ne, u);
            nar_narrow4(u, bf, v.x, v.y);
            if constexpr (EF) {
                if (res) nar_resid4(res, 8ull * g, ne, u, bf, v.x, v.y);
            }
            nar_value4<EF>(src, res, 8ull * g + 4, ne, u);
            nar_narrow4(u, bf, v.z, v.w);
            if constexpr (EF) {
                if (res) nar_resid4(res, 8ull * g + 4, ne, u, bf, v.z, v.w);
            }
        }
        st16_any(dst + 4 + 16ull * g, v, valid);
    }
}
// The UNCP form: the marker and every group.
template <bool EF = false>
__device__ __forceinline__ void nar_uncp(uint8_t *dst, const uint8_t *src, uint8_t *res, uint64_t ne, bool bf, bool staged,
                                         const uint8_t *s_pl) {
    if (threadIdx.x < 4) dst[threadIdx.x] = (uint8_t)(kMagicUNCP >> (8 * threadIdx.x));
    nar_uncp_groups<EF>(dst, src, res, ne, bf, staged, s_pl, 0, (2ull * ne + 15) / 16);
}

// EF: the instance of tdt_encode_narrow_ef_v (a.resid is set; an entry of 0: that message as without it)
template <bool EF>
__global__ __launch_bounds__(kNarTeam) void tdt_encode_narrow_kernel(NarrowArgs a, uint32_t base) {
    __shared__ __attribute__((aligned(16))) uint8_t s_pl[2 * kNarResident];
    __shared__ __attribute__((aligned(16))) uint32_t s_un[kNarHistCopies * 512];  // the histogram copies, then the pair stage
    __shared__ double s_ent[2];
    __shared__ uint32_t s_slots[2][kNW];
    __shared__ NarBig s_big;

    const uint32_t tid = threadIdx.x, lane = (uint32_t)lane_id(), wv = tid >> 6;
    const uint32_t msg = base + blockIdx.x;
    if (msg >= a.n_msgs) return;
    if (a.mark && a.mark[msg]) return;  // (uniform) the tile passes have it
    const uint32_t code = a.elem_codes ? (uint32_t)a.elem_codes[msg] : a.elem;
    const uint64_t srca = a.msgs[msg], size = a.sizes[msg], cap = a.blob_cap[msg];
    const uint8_t *src = reinterpret_cast<const uint8_t *>(srca);
    uint8_t *dst = reinterpret_cast<uint8_t *>(a.blobs[msg]);
    uint8_t *res = nullptr;
    if constexpr (EF) res = reinterpret_cast<uint8_t *>(a.resid[msg]);
    auto report = [&](int32_t st, uint64_t len) __attribute__((always_inline)) {
        if (tid == 0) {
            if (a.status) a.status[msg] = st;
            if (a.out_len) a.out_len[msg] = len;
        }
    };
    // every refusal precedes the first store, to the blob and to the residual
    if (code != kNarBF16 && code != kNarF16) return report(ST_ARG, 0);
    if ((srca & 3u) || (size & 3u) || ((uintptr_t)res & 3u)) return report(kNarStElement, 0);
    const bool bf = code == kNarBF16;
    const uint64_t ne = size / 4, w = size / 2;  // elements, wire bytes
    // should_transform :186-201 and compress_tdt's size guard :364-367 on the wire size, at word size 2
    const bool compress = a.policy_on && w >= a.min_tensor && (w % 4 == 0) && w >= 64 && w < (1ull << 32);
    if (!compress) {
        const bool fits = w + 4 <= cap;
        report(fits ? ST_OK : ST_CAPACITY, fits ? w + 4 : 0);
        if (fits) nar_uncp<EF>(dst, src, res, ne, bf, false, s_pl);
        return;
    }
    const uint32_t ne32 = (uint32_t)ne, w32 = (uint32_t)w;
    const bool resident = ne32 <= kNarResident;

    // ---- H: planes and histograms (extract_features :441-446, every word)
    for (uint32_t i = tid; i < kNarHistCopies * 512u; i += kNarTeam) s_un[i] = 0u;
    __syncthreads();
    for (uint32_t eb = 0; eb < ne32; eb += kNarResident)
        nar_stage<true, EF>(src, res, eb, ne32 - eb < kNarResident ? ne32 - eb : kNarResident, bf, s_pl, s_un);
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
                nar_stage<false, EF, EMIT>(src, res, eb, cnt, bf, s_pl, s_un);  // (the emit pass: the chunk's last read, r' behind it)
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
    if constexpr (EF) {
        if (resident && res) nar_resid_pass(src, res, ne32, bf);  // (neither route below reads the source again)
    }
    if (raw) {
        nar_uncp<EF>(dst, src, res, ne, bf, resident, s_pl);
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

// ---------------------------------------------------------------------------------------
// The tiled form (tdt_enc_narrow_tiled.h).  Every kernel below but the plan and the snapshot runs a
// fixed grid striding over the records the plan claimed; their counts stay in device memory.

// the records in use: what the plan claimed, within the budgets it ran with
__device__ __forceinline__ uint32_t nar_claimed(const NarTiledArgs &t, NarCount k, uint32_t cap) {
    const unsigned long long c = t.cnt[k];
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(c < cap ? (uint32_t)c : cap));
}
__device__ __forceinline__ uint32_t nar_uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
// the wire halfword of element e (EF and a residual: of source + residual, as nar_value4)
template <bool EF = false>
__device__ __forceinline__ uint32_t nar_halfword(const uint8_t *src, const uint8_t *res, uint64_t e, bool bf) {
    uint32_t u = gload<uint32_t>(src + 4ull * e);
    if constexpr (EF) {
        if (res) u = __float_as_uint(__uint_as_float(u) + __uint_as_float(gload<uint32_t>(res + 4ull * e)));
    }
    return bf ? nar_bf16(u) : nar_f16(u);
}
// the bytes of d that are not 0, as a 4-bit mask (the tail of neq_prev_mask4)
__device__ __forceinline__ uint32_t nar_nz_mask4(uint32_t d) {
    const uint32_t nz = (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;
    return (((nz >> 7) * 0x00204081u) >> 21) & 0xfu;
}
// bit i of a 16-bit mask to bit 2 i
__device__ __forceinline__ uint32_t nar_spread16(uint32_t x) {
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    return (x | (x << 1)) & 0x55555555u;
}

// ---- plan: one lane per tensor
__global__ __launch_bounds__(1024) void tdt_narrow_plan_kernel(NarTiledArgs t) {
    __shared__ uint64_t lds[2 * (16 + 1)];
    const NarrowArgs &a = t.a;
    const uint32_t msg = blockIdx.x * 1024u + threadIdx.x, lane = (uint32_t)lane_id();
    bool want = false;
    uint32_t code = 0u;
    uint64_t srca = 0, size = 0, resa = 0;
    if (msg < a.n_msgs) {
        code = a.elem_codes ? (uint32_t)a.elem_codes[msg] : a.elem;
        srca = a.msgs[msg];
        size = a.sizes[msg];
        if (a.resid) resa = a.resid[msg];
        // (everything else is the one-workgroup kernel's: the refusals, a wire size of 2^32 and more)
        want = (code == kNarBF16 || code == kNarF16) && !((srca | size | resa) & 3u) && size / 2 < (1ull << 32) && size > t.large_min;
    }
    const uint64_t ne = size / 4, w = size / 2;
    const uint32_t nt = want ? (uint32_t)((ne + kNarTile - 1) / kNarTile) : 0u;
    uint64_t A[2][1] = {{want ? 1u : 0u}, {nt}}, SA[2][1];
    {
        constexpr int ia[2] = {NC_LARGE, NC_TILES};
        wg_claim_n<2, 1>(A, SA, t.cnt, ia, lds);
    }
    const uint64_t L = SA[0][0], T = SA[1][0];
    const bool ok = want && L < t.lcap && T + nt <= t.tcap;
    uint64_t B[2][1] = {{ok ? 1u : 0u}, {ok ? nt : 0u}}, SB[2][1];
    {
        constexpr int ib[2] = {NC_TILED, NC_TILED_TILES};
        wg_claim_n<2, 1>(B, SB, t.cnt, ib, lds);
    }
    if (want && L < t.lcap) {
        NarLarge g{};  // (over the tile budget: ntiles 0, no pass's record)
        if (ok) {
            g.src = reinterpret_cast<const uint8_t *>(srca);
            g.dst = reinterpret_cast<uint8_t *>(a.blobs[msg]);
            g.res = reinterpret_cast<uint8_t *>(resa);
            g.cap = a.blob_cap[msg];
            g.msg = msg;
            g.ne = (uint32_t)ne;
            g.tile0 = (uint32_t)T;
            g.ntiles = nt;
            // should_transform :186-201 and compress_tdt's size guard :364-367, as the one-workgroup kernel
            const bool compress = a.policy_on && w >= a.min_tensor && (w % 4 == 0) && w >= 64 && w < (1ull << 32);
            g.flags = (compress ? 0u : kNarUncpRouted) | (code == kNarBF16 ? kNarIsBf16 : 0u);
        }
        t.large[L] = g;
    }
    // the owner of every tile record a claim reached, 64 records a step (one lane writing a long
    // tensor's thousands of entries would be the plan's whole time); over a budget: no owner
    const uint32_t tb = (uint32_t)(T < t.tcap ? T : t.tcap), te = (uint32_t)(T + nt < t.tcap ? T + nt : t.tcap);
    const uint32_t own = ok ? (uint32_t)L : kNarNoOwner;
    uint64_t m = __ballot(want && tb < te);
    while (m) {  // (uniform)
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        const uint32_t b = (uint32_t)__shfl((int)tb, l), e = (uint32_t)__shfl((int)te, l), o = (uint32_t)__shfl((int)own, l);
        for (uint32_t k = b + lane; k < e; k += 64u) t.tiles[k].owner = o;
    }
    if (msg < a.n_msgs) t.mark[msg] = ok ? 1u : 0u;
}

// ---- A: one tile staged once — its bins, and the run records of all three candidate streams
template <bool EF>
__global__ __launch_bounds__(kNarTeam) void tdt_narrow_analyse_kernel(NarTiledArgs t) {
    __shared__ __attribute__((aligned(16))) uint8_t s_pl[2 * kNarResident];
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[kNarHistCopies * 512];
    __shared__ uint32_t s_slots[2][kNarCand * kNW];
    __shared__ uint32_t s_first[kNarCand];
    const uint32_t tid = threadIdx.x;
    const uint32_t nt = nar_claimed(t, NC_TILES, t.tcap);
    for (uint32_t i = tid; i < kNarHistCopies * 512u; i += kNarTeam) s_hist[i] = 0u;
    for (uint32_t e = blockIdx.x; e < nt; e += gridDim.x) {  // (uniform)
        NarTileRec &r = t.tiles[e];
        const uint32_t L = nar_uniform(r.owner);
        if (L == kNarNoOwner) continue;
        const NarLarge &g = t.large[L];
        const uint32_t flags = nar_uniform(g.flags);
        if (flags & kNarUncpRouted) continue;  // (nothing to decide: its tiles copy)
        const uint8_t *src = g.src;
        uint8_t *res = EF ? g.res : nullptr;
        const bool bf = (flags & kNarIsBf16) != 0u;
        const uint32_t eb = (e - nar_uniform(g.tile0)) * kNarTile, ne = nar_uniform(g.ne);
        const uint32_t cnt = ne - eb < kNarTile ? ne - eb : kNarTile;
        __syncthreads();  // (the tile before is done with the planes and s_first; the copies are zero)
        if (tid < (uint32_t)kNarCand) s_first[tid] = 0u;
        nar_stage<true, EF>(src, res, eb, cnt, bf, s_pl, s_hist);
        // the bytes before the tile: element eb - 1 (EF: kept for the emit pass, which must not read it again)
        const uint32_t hb = eb ? nar_halfword<EF>(src, res, eb - 1u, bf) : 0u;
        if constexpr (EF) {
            if (tid == 0) r.prev = hb;
        }
        const uint32_t pl = hb & 0xffu, ph = hb >> 8;
        __syncthreads();
        // the copies → the tensor's bins (integer adds: any order gives the same counts)
        uint32_t *bins = t.bins + (size_t)L * kNarBins;
        for (uint32_t b = tid; b < kNarBins; b += kNarTeam) {
            uint32_t c = 0u;
#pragma unroll
            for (uint32_t q = 0; q < kNarHistCopies; ++q) {
                c += s_hist[q * 512u + b];
                s_hist[q * 512u + b] = 0u;
            }
            if (c) atomicAdd(bins + b, c);
        }
        // the sweep: 16 elements of both planes per lane and step; positions in each stream's own
        // coordinates, + 1; cst: the candidate's last run start so far in this tile (0: none yet)
        uint32_t cst[kNarCand] = {0u, 0u, 0u}, inner[kNarCand] = {0u, 0u, 0u};
        for (uint32_t sb = 0; sb < cnt; sb += kNarStep) {  // (uniform)
            const uint32_t l0 = sb + 16u * tid;
            const uint32_t mv = l0 >= cnt ? 0u : (cnt - l0 >= 16u ? 16u : cnt - l0);
            const uint4 lo = *reinterpret_cast<const uint4 *>(s_pl + l0);
            const uint4 hi = *reinterpret_cast<const uint4 *>(s_pl + kNarResident + l0);
            const uint32_t p0 = l0 ? s_pl[l0 - 1u] : pl, p1 = l0 ? s_pl[kNarResident + l0 - 1u] : ph;
            const uint32_t x0[4] = {lo.x, lo.y, lo.z, lo.w}, x1[4] = {hi.x, hi.y, hi.z, hi.w};
            uint32_t sm[kNarCand] = {0u, 0u, 0u}, ma = 0u, mb = 0u;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const uint32_t b0 = d ? x0[d ? d - 1 : 0] : p0 << 24, b1 = d ? x1[d ? d - 1 : 0] : p1 << 24;
                sm[0] |= neq_prev_mask4(x0[d], b0) << (4 * d);
                sm[1] |= neq_prev_mask4(x1[d], b1) << (4 * d);
                // the interleaved stream: its byte 2 i is lo[i] (after hi[i - 1]), byte 2 i + 1 is hi[i] (after lo[i])
                ma |= nar_nz_mask4(x0[d] ^ __builtin_amdgcn_alignbyte(x1[d], b1, 3)) << (4 * d);
                mb |= nar_nz_mask4(x0[d] ^ x1[d]) << (4 * d);
            }
            sm[2] = nar_spread16(ma) | (nar_spread16(mb) << 1);
            const uint32_t vm = (1u << mv) - 1u;
            const uint32_t q[kNarCand] = {eb + l0, eb + l0, 2u * (eb + l0)};  // the lane's first position in each stream
            uint32_t vmax[kNarCand], tmax[kNarCand], vadd[kNarCand], tadd[kNarCand];
#pragma unroll
            for (int s = 0; s < kNarCand; ++s) {
                if (eb + l0 == 0u) sm[s] |= 1u;  // the stream's first byte
                sm[s] &= s == 2 ? (mv == 16u ? ~0u : (1u << (2u * mv)) - 1u) : vm;
                vmax[s] = sm[s] ? q[s] + (31u - (uint32_t)__builtin_clz(sm[s])) + 1u : 0u;
            }
            team_excl_scan<kNW, kNarCand, OpMax>(vmax, tmax, s_slots[0]);
#pragma unroll
            for (int s = 0; s < kNarCand; ++s) {
                const uint32_t cur = vmax[s] > cst[s] ? vmax[s] : cst[s];  // run start + 1 entering this lane
                uint32_t np = 0u;
                if (sm[s]) {
                    const uint32_t qf = q[s] + (uint32_t)__builtin_ctz(sm[s]);
                    np = (uint32_t)__builtin_popcount(sm[s]);
                    if (cur == 0u) {  // the tile's first start: the run it closes is the scan's
                        --np;
                        s_first[s] = qf + 1u;
                    } else {
                        np += (qf - cur) / 255u;  // nar_step: (Lr - 1) / 255 full pairs, Lr = qf - (cur - 1)
                    }
                }
                vadd[s] = np;
            }
            team_excl_scan<kNW, kNarCand, OpAdd>(vadd, tadd, s_slots[1]);
#pragma unroll
            for (int s = 0; s < kNarCand; ++s) {
                cst[s] = tmax[s] > cst[s] ? tmax[s] : cst[s];
                inner[s] += tadd[s];
            }
        }
        __syncthreads();  // (s_first is written)
        if (tid < (uint32_t)kNarCand) {
            r.first[tid] = s_first[tid];
            r.last[tid] = tid == 0u ? cst[0] : tid == 1u ? cst[1] : cst[2];
            r.inner[tid] = tid == 0u ? inner[0] : tid == 1u ? inner[1] : inner[2];
        }
    }
}

// ---- M: the mapping of a large tensor, the scan over its tiles, its length, status and fixed words
__global__ __launch_bounds__(kNarTeam) void tdt_narrow_map_kernel(NarTiledArgs t) {
    __shared__ double s_ent[2];
    __shared__ uint32_t s_slots[2][2 * kNW];
    const NarrowArgs &a = t.a;
    const uint32_t tid = threadIdx.x, lane = (uint32_t)lane_id(), wv = tid >> 6;
    const uint32_t nl = nar_claimed(t, NC_LARGE, t.lcap);
    for (uint32_t L = blockIdx.x; L < nl; L += gridDim.x) {  // (uniform)
        NarLarge *g = t.large + L;
        const uint32_t nt = nar_uniform(g->ntiles);
        if (!nt) continue;
        const uint32_t msg = g->msg, ne32 = nar_uniform(g->ne), flags = nar_uniform(g->flags);
        const uint64_t w = 2ull * ne32, cap = g->cap;
        const uint32_t w32 = (uint32_t)w;
        uint8_t *dst = g->dst;
        auto report = [&](int32_t st, uint64_t len) __attribute__((always_inline)) {
            if (tid == 0) {
                if (a.status) a.status[msg] = st;
                if (a.out_len) a.out_len[msg] = len;
            }
        };
        if (flags & kNarUncpRouted) {
            const bool fits = w + 4 <= cap;
            report(fits ? ST_OK : ST_CAPACITY, fits ? w + 4 : 0);
            if (tid == 0) g->route = fits ? kNarRaw : kNarRefused;
            continue;
        }
        // entropies, then perform_clustering :507-525: entropy > in-order sum / 2
        uint32_t *bins = t.bins + (size_t)L * kNarBins;
        __syncthreads();  // (the tensor before is done with s_ent)
        if (wv < 2u) {
            uint32_t cb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                cb[k] = bins[wv * 256u + 64u * k + lane];
                bins[wv * 256u + 64u * k + lane] = 0u;  // (all zero again for the next call)
            }
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
        const bool inter = ns == 1u;
        const uint32_t S = inter ? w32 : ne32;  // bytes of a stream
        // stream s is candidate cand[s]: stream 0 holds the positions mapped to 0
        const uint32_t cand[2] = {inter ? 2u : m0, inter ? 2u : 1u - m0};
        NarTileRec *tiles = t.tiles + g->tile0;
        uint32_t carry[2] = {0u, 0u}, base[2] = {0u, 0u};  // (uniform) behind the tiles so far
        for (uint32_t i0 = 0; i0 < nt; i0 += kNarTeam) {
            const uint32_t i = i0 + tid;
            AnyTileRuns runs[2] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
            if (i < nt) {
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    if ((uint32_t)s < ns) runs[s] = AnyTileRuns{tiles[i].first[cand[s]], tiles[i].last[cand[s]], tiles[i].inner[cand[s]]};
            }
            uint32_t vmax[2] = {runs[0].last, runs[1].last}, tmax[2];
            team_excl_scan<kNW, 2, OpMax>(vmax, tmax, s_slots[0]);
            uint32_t vadd[2], tadd[2], cin[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                cin[s] = vmax[s] > carry[s] ? vmax[s] : carry[s];
                vadd[s] = any_tile_pairs(runs[s], cin[s]);
            }
            team_excl_scan<kNW, 2, OpAdd>(vadd, tadd, s_slots[1]);
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
        uint32_t P[2] = {0u, 0u};
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if ((uint32_t)s < ns) P[s] = base[s] + any_final_pairs(S, carry[s]);
        const uint64_t o1 = 32 + 2ull * P[0];                        // stream 1's length word
        const uint64_t Etdt = ns == 2u ? o1 + 4 + 2ull * P[1] : o1;  // header 28, length word(s), pairs
        const bool raw = a.raw_fallback && Etdt > w + 4;             // TDT_OPT_RAW_FALLBACK
        const uint64_t E = raw ? w + 4 : Etdt;
        const bool fits = E <= cap;
        report(fits ? ST_OK : ST_CAPACITY, fits ? E : 0);
        if (tid == 0) {
            g->route = !fits ? kNarRefused : raw ? kNarRaw : kNarTdt;
            g->m0 = m0;
            g->m1 = m1;
            g->pairs[0] = P[0];
            g->pairs[1] = P[1];
        }
        // header (serialize :81-117): magic, original size, streams, word size, mapping; length words
        if (fits && !raw && tid < 36u) {
            const uint32_t k = tid >> 2;
            const uint32_t hv = k == 0 ? kMagicTDT : k == 1 ? w32 : k == 2 ? ns : k == 3 ? 2u : k == 4 ? 2u : k == 5 ? m0 : k == 6 ? m1
                              : k == 7 ? 2u * P[0] : 2u * P[1];
            const uint64_t at = k < 8u ? tid : o1 + (tid & 3u);
            if (k < 8u || ns == 2u) dst[at] = (uint8_t)(hv >> (8u * (tid & 3u)));
        }
    }
}

// ---- E: one tile's pairs of the chosen stream(s), or its share of the UNCP form
template <bool EF>
__global__ __launch_bounds__(kNarTeam) void tdt_narrow_emit_kernel(NarTiledArgs t) {
    __shared__ __attribute__((aligned(16))) uint8_t s_pl[2 * kNarResident];
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[(2u * kNarStagePairs + 8u + 3u) / 4u];
    __shared__ uint32_t s_slots[2][kNW];
    __shared__ NarBig s_big;
    const uint32_t tid = threadIdx.x;
    const uint32_t nt = nar_claimed(t, NC_TILES, t.tcap);
    for (uint32_t e = blockIdx.x; e < nt; e += gridDim.x) {  // (uniform)
        const NarTileRec &r = t.tiles[e];
        const uint32_t L = nar_uniform(r.owner);
        if (L == kNarNoOwner) continue;
        const NarLarge &g = t.large[L];
        const uint32_t route = nar_uniform(g.route);
        if (route == kNarRefused) continue;  // (nothing is written)
        const uint8_t *src = g.src;
        uint8_t *dst = g.dst;
        uint8_t *res = EF ? g.res : nullptr;
        const bool bf = (nar_uniform(g.flags) & kNarIsBf16) != 0u;
        const uint32_t tt = e - nar_uniform(g.tile0), eb = tt * kNarTile, ne = nar_uniform(g.ne);
        const uint32_t cnt = ne - eb < kNarTile ? ne - eb : kNarTile;
        if (route == kNarRaw) {  // the tile's wire bytes behind the marker (a tile is whole 16-byte groups)
            if (tt == 0u && tid < 4u) dst[tid] = (uint8_t)(kMagicUNCP >> (8 * tid));
            nar_uncp_groups<EF>(dst, src, res, ne, bf, false, nullptr, eb / 8u, (2ull * (eb + cnt) + 15) / 16);
            continue;
        }
        const uint32_t m0 = nar_uniform(g.m0), m1 = nar_uniform(g.m1);
        const uint32_t ns = (m0 | m1) ? 2u : 1u;
        const bool inter = ns == 1u;
        const uint32_t S = inter ? 2u * ne : ne;
        __syncthreads();  // (the tile before is done with the planes)
        nar_stage<false, EF, true>(src, res, eb, cnt, bf, s_pl, nullptr);  // (EF: the tile's r' behind its last read)
        // the bytes before the tile (EF: as the analyse pass saw them; that element's residual may be rewritten by now)
        uint32_t hb;
        if constexpr (EF) hb = eb ? nar_uniform(r.prev) : 0u;
        else hb = eb ? nar_halfword(src, nullptr, eb - 1u, bf) : 0u;
        __syncthreads();
        uint8_t *const pairs[2] = {dst + 32, dst + 32 + 2ull * g.pairs[0] + 4};
#pragma unroll
        for (uint32_t s = 0; s < 2; ++s) {
            if (s >= ns) continue;
            const uint32_t plane = m0 ? 1u - s : s;  // stream 0 holds the positions mapped to 0
            NarCarry c{r.carry[s], r.base[s], inter || plane ? hb >> 8 : hb & 0xffu};
            const uint32_t Qb = inter ? 2u * eb : eb, Ls = inter ? 2u * cnt : cnt;
            for (uint32_t lq = 0; lq < Ls; lq += kNarStep)
                nar_step<true>(s_pl, inter, plane, Qb + lq, lq, Ls - lq < kNarStep ? Ls - lq : kNarStep, c, pairs[s], s_stage, s_slots,
                               &s_big);
            if (tt + 1u == nar_uniform(g.ntiles)) {  // the stream's last tile: the run that closes at the stream's end
                const uint32_t Lr = S - (c.cstart - 1u);
                const uint32_t full = (Lr - 1u) / 255u;
                uint8_t *A = pairs[s] + 2ull * c.cpairs;
                nar_fill(A, full, c.lastb);
                if (tid == 0) {
                    A[2ull * full] = (uint8_t)(Lr - 255u * full);
                    A[2ull * full + 1] = (uint8_t)c.lastb;
                }
            }
        }
    }
}

// ---- snap: the counters to the host's snapshot, and zero for the next call
__global__ __launch_bounds__(64) void tdt_narrow_snap_kernel(unsigned long long *cnt, uint32_t *pin) {
    uint32_t *c = reinterpret_cast<uint32_t *>(cnt);
    if (threadIdx.x < kPlanSnapBytes / 4) {
        if (pin) pin[threadIdx.x] = c[threadIdx.x];
        c[threadIdx.x] = 0u;
    }
}

}  // namespace

int launch_narrow_plan(const NarTiledArgs &t, hipStream_t s) {
    hipLaunchKernelGGL(tdt_narrow_plan_kernel, dim3((t.a.n_msgs + 1023u) / 1024u), dim3(1024), 0, s, t);
    return (int)hipGetLastError();
}

int launch_narrow_tiles(const NarTiledArgs &t, hipStream_t s) {
    const dim3 tg(std::max(1u, std::min(t.tcap, t.grid))), lg(std::max(1u, std::min(t.lcap, t.grid)));
    const bool ef = t.a.resid != nullptr;  // tdt_encode_narrow_ef_v
    hipLaunchKernelGGL(ef ? tdt_narrow_analyse_kernel<true> : tdt_narrow_analyse_kernel<false>, tg, dim3(kNarTeam), 0, s, t);
    hipLaunchKernelGGL(tdt_narrow_map_kernel, lg, dim3(kNarTeam), 0, s, t);
    hipLaunchKernelGGL(ef ? tdt_narrow_emit_kernel<true> : tdt_narrow_emit_kernel<false>, tg, dim3(kNarTeam), 0, s, t);
    return (int)hipGetLastError();
}

int launch_narrow_snap(const NarTiledArgs &t, uint32_t *pin, hipStream_t s) {
    hipLaunchKernelGGL(tdt_narrow_snap_kernel, dim3(1), dim3(64), 0, s, t.cnt, pin);
    return (int)hipGetLastError();
}

int launch_encode_narrow(const NarrowArgs &a, hipStream_t s) {
    // one workgroup per message; a launch holds < 2^32 threads
    const uint32_t maxb = 0xffffffffu / kNarTeam;
    for (uint32_t b = 0; b < a.n_msgs; b += maxb)
        hipLaunchKernelGGL(a.resid ? tdt_encode_narrow_kernel<true> : tdt_encode_narrow_kernel<false>,
                           dim3(std::min(maxb, a.n_msgs - b)), dim3(kNarTeam), 0, s, a, b);
    return (int)hipGetLastError();
}

}  // namespace psy
