// tdt_pack.hip — the byte-balanced pack kernel (tdt_pack.h), the two small kernels that lay out the
// scratch slots of tdt_encode_batch_vp, and their launchers.  A translation unit of its own,
// compiled beside tdt_api.hip and tdt_anyws.hip (psyne_amd/build.py).
#include "tdt_pack.h"

#include "../../include/psyne_tdt.h"
#include "tdt_copy.h"
#include "tdt_device.h"

// 16-byte chunks whose loads a lane issues before their stores (a build-time knob of the measurements)
#ifndef PSY_PACK_U
#define PSY_PACK_U 2
#endif

namespace psy {
namespace {

// Thread t of T copies its share of a segment: the shared copy (tdt_copy.h) with non-temporal
// 16-byte stores, the loads of U chunks issued before their stores.  src is a blob in device memory
// (tdt_pack_v's contract), out the packed device buffer.
template <uint32_t T, int U>
__device__ __forceinline__ void pack_copy(uint8_t *dst, const uint8_t *src, uint64_t len, uint32_t t) {
    static_assert(T >= kCopyMinT, "copy_shifted: one byte store per thread covers the head and the tail");
    copy_shifted<U, true>(dst, src, len, t, T);
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// One workgroup per piece of the packed output (grid-strided over the pieces out_cap allows).
__global__ __launch_bounds__(kPackLanes) void tdt_pack_kernel(const uint64_t *__restrict__ blobs,
                                                              const uint64_t *__restrict__ off, uint32_t n,
                                                              uint8_t *__restrict__ out, uint64_t out_cap,
                                                              int32_t *__restrict__ status, int keep_errors,
                                                              uint32_t cut, uint64_t pieces) {
    if (status) {
        for (uint64_t i = (uint64_t)blockIdx.x * kPackLanes + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kPackLanes) {
            const int32_t st = off[i + 1] > out_cap ? TDT_E_CAPACITY : TDT_OK;
            if (!keep_errors) status[i] = st;
            else if (st != TDT_OK && status[i] == TDT_OK) status[i] = st;
        }
    }
    const uint32_t lane = (uint32_t)lane_id(), wave = threadIdx.x >> 6;
    const uint64_t total = off[n];
    for (uint64_t piece = blockIdx.x; piece < pieces; piece += gridDim.x) {
        const PackPiece pc = pack_piece(piece, total, out_cap);
        if (pc.p0 >= pc.p1) return;  // (at or past the end: every later piece too)
        // the first blob of the piece (every wave for itself: the probes hit the caches)
        PackRange r{0u, n};
        while (!pack_found(r)) {
            const uint32_t stride = pack_stride(r);
            const uint64_t j = pack_probe(r, stride, lane);
            const bool hit = j < r.hi && off[j] <= pc.p0;
            r = pack_narrow(r, stride, (uint32_t)__popcll(__ballot(hit)));
        }
        // the segments, 64 blobs per load
        uint32_t seg = 0;
        for (uint64_t base = r.lo; base < n; base += 64) {
            const uint64_t j = base + lane;
            const uint64_t o0 = j < n ? off[j] : ~0ull, o1 = j < n ? off[j + 1] : ~0ull;
            const PackWalk wk = j < n ? pack_walk(o0, o1, pc, out_cap) : PACK_END;
            uint64_t live = __ballot(wk == PACK_COPY);
            const bool last = __ballot(wk == PACK_END) != 0;
            while (live) {
                const int b = __ffsll((unsigned long long)live) - 1;
                live &= live - 1;
                const PackSeg s = pack_segment(shfl_u64(o0, b), shfl_u64(o1, b), pc);
                const bool mine = s.len > cut || (seg++ & (kPackWaves - 1)) == wave;
                if (!mine) continue;
                const uint8_t *src = reinterpret_cast<const uint8_t *>(blobs[base + b]) + s.src_off;
                if (s.len > cut) pack_copy<kPackLanes, PSY_PACK_U>(out + s.dst_off, src, s.len, threadIdx.x);
                else pack_copy<64, PSY_PACK_U>(out + s.dst_off, src, s.len, lane);
            }
            if (last) break;
        }
    }
}

__global__ __launch_bounds__(256) void tdt_pack_bounds_kernel(const uint64_t *size, const int32_t *ws, int32_t ws_all,
                                                              uint64_t mask, uint64_t *off, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t w = ws ? ws[i] : ws_all;
    off[i] = w >= 1 && w <= 64 && ((mask >> (w - 1)) & 1) ? 28ull + 4ull * (uint32_t)w + 2ull * size[i] : 0ull;
}

__global__ __launch_bounds__(256) void tdt_pack_slots_kernel(const uint64_t *off, uint8_t *buf, uint64_t buf_bytes,
                                                             uint64_t *ptr, uint64_t *cap, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t o0 = off[i], o1 = off[i + 1];
    ptr[i] = (uint64_t)(uintptr_t)buf + o0;
    cap[i] = o1 <= buf_bytes ? o1 - o0 : 0;
}

__global__ __launch_bounds__(256) void tdt_pack_exact_slots_kernel(const uint64_t *off, uint8_t *out, uint64_t out_cap,
                                                                   uint64_t *ptr, uint64_t *cap, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const PackSlot sl = pack_exact_slot(off[i], off[i + 1], out_cap);
    ptr[i] = (uint64_t)(uintptr_t)out + sl.off;
    cap[i] = sl.cap;
}

}  // namespace

int launch_pack(const uint64_t *blobs, const uint64_t *off, uint32_t n, uint8_t *out, uint64_t out_cap, int32_t *status,
                bool keep_errors, uint32_t cut, uint32_t grid_cap, void *stream) {
    const uint64_t pieces = out_cap / kPackPiece + (out_cap % kPackPiece ? 1u : 0u);
    const uint64_t grid = pieces < grid_cap ? pieces : grid_cap;
    hipLaunchKernelGGL(tdt_pack_kernel, dim3(grid ? (uint32_t)grid : 1u), dim3(kPackLanes), 0, (hipStream_t)stream, blobs,
                       off, n, out, out_cap, status, keep_errors ? 1 : 0, cut, pieces);
    return (int)hipGetLastError();
}

int launch_pack_bounds(const uint64_t *size, const int32_t *ws, int32_t ws_all, uint64_t mask, uint64_t *off, uint32_t n,
                       void *stream) {
    hipLaunchKernelGGL(tdt_pack_bounds_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, size, ws, ws_all,
                       ws ? mask : ~0ull, off, n);
    return (int)hipGetLastError();
}

int launch_pack_slots(const uint64_t *off, uint8_t *buf, uint64_t buf_bytes, uint64_t *ptr, uint64_t *cap, uint32_t n,
                      void *stream) {
    hipLaunchKernelGGL(tdt_pack_slots_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, off, buf,
                       buf_bytes, ptr, cap, n);
    return (int)hipGetLastError();
}

int launch_pack_exact_slots(const uint64_t *off, uint8_t *out, uint64_t out_cap, uint64_t *ptr, uint64_t *cap, uint32_t n,
                            void *stream) {
    hipLaunchKernelGGL(tdt_pack_exact_slots_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, off, out,
                       out_cap, ptr, cap, n);
    return (int)hipGetLastError();
}

}  // namespace psy
