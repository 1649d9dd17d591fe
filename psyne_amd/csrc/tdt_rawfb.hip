// tdt_rawfb.hip — the kernels of the raw fallback (tdt_rawfb.h) and their launchers: the slot clamp,
// the flag pass, the byte-balanced copy of the flagged messages into their own slots, and the small
// kernels of the size and slot routes.  A translation unit of its own, compiled beside tdt_api.hip
// (psyne_amd/build.py): no encode kernel is touched.
#include "tdt_rawfb.h"

#include "../../include/psyne_tdt.h"
#include "tdt_copy.h"
#include "tdt_device.h"

namespace psy {
namespace {

static_assert(kRawStOk == TDT_OK && kRawStCapacity == TDT_E_CAPACITY, "the rule reads the C ABI's statuses");

__device__ __forceinline__ uint64_t raw_shfl_u64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}
// *count += the threads of the workgroup with `hit`: one atomic per workgroup that has any (one per
// wave was 4,096 atomics on the one word for 262,144 messages, and the flag pass took 52 us:
// profiles/raw_fallback/kernel_stats_row5.csv)
__device__ __forceinline__ void raw_count(unsigned long long *count, bool hit) {
    const int c = __syncthreads_count(hit);
    if (c && threadIdx.x == 0) atomicAdd(count, (unsigned long long)c);
}

__global__ __launch_bounds__(256) void tdt_raw_clamp_kernel(const uint64_t *size, const uint64_t *cap, uint64_t *cap_out,
                                                            uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t raw = raw_blob_bytes(size[i]), c = cap[i];
    cap_out[i] = c < raw ? c : raw;
}

__global__ __launch_bounds__(256) void tdt_raw_contig_kernel(const uint8_t *in, const uint64_t *in_off, uint8_t *out,
                                                             const uint64_t *slot_off, uint64_t *ptr, uint64_t *size,
                                                             uint64_t *optr, uint64_t *cap, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t i0 = in_off[i], s0 = slot_off[i];
    ptr[i] = (uint64_t)(uintptr_t)in + i0;
    size[i] = in_off[i + 1] - i0;
    optr[i] = (uint64_t)(uintptr_t)out + s0;
    cap[i] = slot_off[i + 1] - s0;
}

constexpr uint32_t kRawFlagLanes = 1024;
__global__ __launch_bounds__(kRawFlagLanes) void tdt_raw_flag_kernel(const uint64_t *size, const uint64_t *cap, int32_t *status,
                                                           uint64_t *len, uint64_t *raw_len, unsigned long long *count,
                                                           uint32_t n) {
    const uint32_t i = blockIdx.x * kRawFlagLanes + threadIdx.x;
    bool flagged = false;
    if (i < n) {
        const uint64_t sz = size[i];
        flagged = raw_flagged(status[i], len[i], sz, cap[i]);
        if (flagged) {
            status[i] = TDT_OK;
            len[i] = raw_blob_bytes(sz);
        }
        raw_len[i] = flagged ? raw_blob_bytes(sz) : 0ull;
    }
    raw_count(count, flagged);
}

// One 512-lane workgroup per kPackPiece bytes of the flagged blobs (a fixed grid striding over the
// device-side total; it leaves at once when nothing is flagged).  The search and the walk are the
// pack kernel's (tdt_pack.hip); a segment goes to its blob's own slot.
template <int U>
__global__ __launch_bounds__(kPackLanes) void tdt_raw_copy_kernel(const uint64_t *__restrict__ msgs,
                                                                  const uint64_t *__restrict__ blobs,
                                                                  const uint64_t *__restrict__ off, uint32_t n,
                                                                  uint32_t cut) {
    const uint32_t lane = (uint32_t)lane_id(), wave = threadIdx.x >> 6;
    const uint64_t total = off[n];
    for (uint64_t piece = blockIdx.x;; piece += gridDim.x) {
        const PackPiece pc = pack_piece(piece, total, ~0ull);
        if (pc.p0 >= pc.p1) return;  // (at or past the end: every later piece too)
        PackRange r{0u, n};
        while (!pack_found(r)) {
            const uint32_t stride = pack_stride(r);
            const uint64_t j = pack_probe(r, stride, lane);
            const bool hit = j < r.hi && off[j] <= pc.p0;
            r = pack_narrow(r, stride, (uint32_t)__popcll(__ballot(hit)));
        }
        uint32_t seg = 0;
        for (uint64_t base = r.lo; base < n; base += 64) {
            const uint64_t j = base + lane;
            const uint64_t o0 = j < n ? off[j] : ~0ull, o1 = j < n ? off[j + 1] : ~0ull;
            const PackWalk wk = j < n ? pack_walk(o0, o1, pc, ~0ull) : PACK_END;
            uint64_t live = __ballot(wk == PACK_COPY);
            const bool last = __ballot(wk == PACK_END) != 0;
            while (live) {
                const int b = __ffsll((unsigned long long)live) - 1;
                live &= live - 1;
                const RawSeg s = raw_segment(raw_shfl_u64(o0, b), raw_shfl_u64(o1, b), pc);
                const bool wide = s.len > cut;
                const bool mine = wide || (seg++ & (kPackWaves - 1)) == wave;
                if (!mine) continue;
                uint8_t *dst = reinterpret_cast<uint8_t *>(blobs[base + b]);
                const uint8_t *src = reinterpret_cast<const uint8_t *>(msgs[base + b]);
                const uint32_t t = wide ? threadIdx.x : lane;
                if (t < s.marker_n) dst[s.marker_at + t] = raw_marker_byte(s.marker_at + t);
                if (s.len == 0) continue;
                if (wide) copy_shifted<U, true>(dst + s.dst_off, src + s.src_off, s.len, threadIdx.x, kPackLanes);
                else copy_shifted<U, true>(dst + s.dst_off, src + s.src_off, s.len, lane, 64);
            }
            if (last) break;
        }
    }
}

__global__ __launch_bounds__(256) void tdt_raw_min_kernel(const uint64_t *size, const uint64_t *in_off, uint64_t *enc,
                                                          uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t sz = in_off ? in_off[i + 1] - in_off[i] : size[i], e = enc[i], m = raw_min_size(e, sz);
    if (m != e) enc[i] = m;
}

__global__ __launch_bounds__(256) void tdt_raw_bounds_kernel(const uint64_t *size, const int32_t *ws, int32_t ws_all,
                                                             uint64_t mask, uint64_t *off, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int32_t w = ws ? ws[i] : ws_all;
    off[i] = w >= 1 && w <= 64 && ((mask >> (w - 1)) & 1) ? raw_blob_bytes(size[i]) : 0ull;
}

__global__ __launch_bounds__(256) void tdt_raw_slots_kernel(const uint64_t *in_off, uint64_t *off, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    off[i] = (uint64_t)kRawMarkerBytes * i + (in_off[i] - in_off[0]);
}

uint32_t blocks256(uint32_t n) { return (n + 255u) / 256u; }

}  // namespace

int launch_raw_clamp(const uint64_t *size, const uint64_t *cap, uint64_t *cap_out, uint32_t n, void *stream) {
    hipLaunchKernelGGL(tdt_raw_clamp_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, size, cap, cap_out, n);
    return (int)hipGetLastError();
}

int launch_raw_contig(const uint8_t *in, const uint64_t *in_off, uint8_t *out, const uint64_t *slot_off, uint64_t *ptr,
                      uint64_t *size, uint64_t *optr, uint64_t *cap, uint32_t n, void *stream) {
    hipLaunchKernelGGL(tdt_raw_contig_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, in, in_off, out,
                       slot_off, ptr, size, optr, cap, n);
    return (int)hipGetLastError();
}

int launch_raw_flag(const uint64_t *size, const uint64_t *cap, int32_t *status, uint64_t *len, uint64_t *raw_len,
                    unsigned long long *count, uint32_t n, void *stream) {
    hipLaunchKernelGGL(tdt_raw_flag_kernel, dim3((n + kRawFlagLanes - 1) / kRawFlagLanes), dim3(kRawFlagLanes), 0,
                       (hipStream_t)stream, size, cap, status, len, raw_len, count, n);
    return (int)hipGetLastError();
}

int launch_raw_copy(const uint64_t *msgs, const uint64_t *blobs, const uint64_t *off, uint32_t n, uint32_t cut,
                    uint32_t grid, void *stream) {
    hipLaunchKernelGGL(tdt_raw_copy_kernel<2>, dim3(grid ? grid : 1u), dim3(kPackLanes), 0, (hipStream_t)stream, msgs,
                       blobs, off, n, cut);
    return (int)hipGetLastError();
}

int launch_raw_min(const uint64_t *size, const uint64_t *in_off, uint64_t *enc, uint32_t n, void *stream) {
    hipLaunchKernelGGL(tdt_raw_min_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, size, in_off, enc, n);
    return (int)hipGetLastError();
}

int launch_raw_bounds(const uint64_t *size, const int32_t *ws, int32_t ws_all, uint64_t mask, uint64_t *off, uint32_t n,
                      void *stream) {
    hipLaunchKernelGGL(tdt_raw_bounds_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, size, ws, ws_all,
                       ws ? mask : ~0ull, off, n);
    return (int)hipGetLastError();
}

int launch_raw_slots(const uint64_t *in_off, uint64_t *off, uint32_t n, void *stream) {
    hipLaunchKernelGGL(tdt_raw_slots_kernel, dim3((n + 256u) / 256u), dim3(256), 0, (hipStream_t)stream, in_off, off, n);
    return (int)hipGetLastError();
}

}  // namespace psy
