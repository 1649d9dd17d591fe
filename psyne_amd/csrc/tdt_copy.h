// tdt_copy.h — the one copy between a source and a destination of unrelated alignment: the UNCP
// passthrough lists, the compaction gathers, the host pipeline's output copies (tdt_api.hip) and
// the pack kernel (tdt_pack.hip) all run copy_shifted.
//
// Participant t of T copies its share of len bytes:
//   head    byte stores up to the destination's next 16-byte boundary (byte t by participant t);
//   chunks  16-byte stores, chunk k by participant k % T.  Chunk k is source bytes s0 + 16k ..
//           s0 + 16k + 15 (s0 = src + head); it is read as the aligned dwords from that address
//           rounded down to 4 and funnel-shifted by the source's misalignment sh, the fifth dword
//           only when sh != 0;
//   tail    the fewer than 16 bytes left, byte done + t by participant t.
//
// THE OVER-READ RULE.  Each of the four dwords of a chunk, and the fifth when sh != 0, holds at
// least one byte of that chunk.  So no aligned dword is read that holds no source byte: the copy
// reads at most 3 bytes before src and at most 3 bytes beyond src + len, inside the first and the
// last such dword, and never another 4-byte-aligned word.  A source needs no slack beyond its own
// aligned dwords; the head and tail bytes are read as bytes.  tests/cpp/test_copy_shifted.cpp
// checks the rule on every dword address the loop forms.
//
// The head, the chunks, the combine and the loop are plain host / device C++ here, so that a host program can
// drive them over a byte arena; the device copy below them supplies the loads and stores.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PSY_COPY_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define PSY_COPY_HD inline
#endif

namespace psy {

// The fewest participants of a copy: the head and the tail are one guarded byte store each, and
// both are shorter than 16 bytes.
constexpr uint32_t kCopyMinT = 16;

// The head: the bytes before the destination's first 16-byte boundary (all len when it ends before)
PSY_COPY_HD uint64_t copy_head(uintptr_t dst, uint64_t len) {
    const uint64_t head = (16 - (dst & 15)) & 15;
    return head > len ? len : head;
}
// The chunks of the `rest` bytes from s0 = src + head on; the tail starts at head + 16 * nb
struct CopyChunks {
    uint64_t nb;   // 16-byte chunks
    uint32_t sh;   // misalignment of s0 in bits: 0, 8, 16 or 24
    uintptr_t sw;  // s0 rounded down to 4: chunk k reads the aligned dwords at sw + 16k
};
PSY_COPY_HD CopyChunks copy_chunks(uintptr_t s0, uint64_t rest) {
    return CopyChunks{rest / 16, (uint32_t)(s0 & 3) * 8, s0 & ~(uintptr_t)3};
}

// Five aligned dwords shifted down by sh bits into the 16 bytes of a chunk (w4 is not looked at
// when sh == 0)
struct alignas(16) CopyWords {
    uint32_t x, y, z, w;
};
PSY_COPY_HD CopyWords copy_combine(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t sh) {
    return CopyWords{(uint32_t)((((uint64_t)w1 << 32) | w0) >> sh), (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh),
                     (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh), (uint32_t)((((uint64_t)w4 << 32) | w3) >> sh)};
}

// The copy itself over a caller's accesses, the only ones it makes: byte(i) copies byte i, load(q)
// reads the aligned dword q, store(p, words) writes the 16 bytes of a chunk at its 16-byte aligned
// place p.  The loads of U chunks are issued before their stores (U = 1: one chunk at a time).
// Precondition: T >= kCopyMinT, and every participant 0..T-1 calls it.
template <int U, class Byte, class Load, class Store>
PSY_COPY_HD void copy_shifted_with(uint8_t *dst, const uint8_t *src, uint64_t len, uint64_t t, uint64_t T, Byte byte,
                                   Load load, Store store) {
    const uint64_t head = copy_head((uintptr_t)dst, len);
    if (t < head) byte(t);
    const CopyChunks c = copy_chunks((uintptr_t)(src + head), len - head);
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(c.sw);
    CopyWords *dv = reinterpret_cast<CopyWords *>(dst + head);
    // the aligned dwords of chunk k, the fifth only when the source is misaligned (the over-read rule)
    const auto read = [&](uint64_t k, uint32_t *w) {
        const uint32_t *q = sw + 4 * k;
        w[0] = load(q), w[1] = load(q + 1), w[2] = load(q + 2), w[3] = load(q + 3);
        w[4] = c.sh ? load(q + 4) : 0u;
    };
    const auto write = [&](uint64_t k, const uint32_t *w) {
        store(dv + k, copy_combine(w[0], w[1], w[2], w[3], w[4], c.sh));
    };
    uint64_t k = t;
    for (; k + (uint64_t)(U - 1) * T < c.nb; k += (uint64_t)U * T) {
        uint32_t w[U][5];
#pragma unroll
        for (int g = 0; g < U; ++g) read(k + (uint64_t)g * T, w[g]);
#pragma unroll
        for (int g = 0; g < U; ++g) write(k + (uint64_t)g * T, w[g]);
    }
    if (U > 1)  // (U = 1: the loop above took every chunk; left in, this one cost the copy kernels VGPRs)
        for (; k < c.nb; k += T) {
            uint32_t w[5];
            read(k, w);
            write(k, w);
        }
    const uint64_t done = head + 16 * c.nb;
    if (t < len - done) byte(done + t);  // (fewer than 16 bytes, and T >= 16)
}

}  // namespace psy

#if defined(__HIPCC__)
#include "tdt_device.h"

namespace psy {

// Participant t of T copies its share of len bytes, src → dst (T >= kCopyMinT: copy_shifted_with).
// src is device memory (global loads); dst may be device memory or mapped host memory, so the
// 16-byte stores are generic ones unless NT asks for non-temporal global stores (device memory only).
template <int U, bool NT>
__device__ __forceinline__ void copy_shifted(uint8_t *dst, const uint8_t *src, uint64_t len, uint64_t t, uint64_t T) {
    copy_shifted_with<U>(
        dst, src, len, t, T, [=](uint64_t i) { dst[i] = src[i]; }, [](const uint32_t *q) { return gload<uint32_t>(q); },
        [](CopyWords *p, CopyWords w) {
            if (NT) st16_nt(p, make_uint4(w.x, w.y, w.z, w.w));
            else *reinterpret_cast<uint4 *>(p) = make_uint4(w.x, w.y, w.z, w.w);
        });
}

}  // namespace psy
#endif
