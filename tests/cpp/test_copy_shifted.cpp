// The funnel-shift copy of psyne_amd/csrc/tdt_copy.h (copy_head, copy_chunks, copy_combine and the
// loop copy_shifted_with), driven over a byte arena as the kernels drive it: participants t = 0..T-1
// one after the other, every access through this file's own byte, dword-load and chunk-store.
// Checked for every destination and source alignment, every length 0..96 and around 4096, T of
// 16, 64, 512 and 768, one and two chunks per step:
//   - the destination range equals the source range;
//   - the bytes before and after the destination range keep their sentinels;
//   - every dword the loop reads is aligned and holds a byte of [src, src + len) (the over-read
//     rule of tdt_copy.h), and every byte it reads singly lies inside that range;
//   - every destination byte is written exactly once across the participants, by stores that lie
//     inside the destination range (the 16-byte ones aligned).
// Host code only; built with -fsanitize=address,undefined and run directly
// (tests/test_copy_shifted.py).  The source lies inside a larger arena: the partial first and last
// dwords are legitimate reads that a redzone right at the source's ends would flag.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../psyne_amd/csrc/tdt_copy.h"

namespace {

long failures = 0;
#define CHECK(cond)                                                                                            \
    do {                                                                                                       \
        if (!(cond)) {                                                                                         \
            if (failures < 20)                                                                                 \
                std::printf("FAIL %s:%d: %s (da %u sa %u len %llu T %llu U %d)\n", __FILE__, __LINE__, #cond, \
                            cs.da, cs.sa, (unsigned long long)cs.len, (unsigned long long)cs.T, cs.U);        \
            ++failures;                                                                                        \
        }                                                                                                      \
    } while (0)

constexpr uint64_t kMaxLen = 4097, kPad = 64;
constexpr uint8_t kSentinel = 0xA5;

struct Case {
    uint32_t da, sa;  // the alignments of dst and src (mod 16)
    uint64_t len, T;
    int U;
};

uint8_t source_byte(uint64_t i) {
    const uint8_t b = (uint8_t)(i * 7u + (i >> 8) * 13u + 1u);
    return b == kSentinel ? 0x5A : b;  // (a copied byte never looks like an untouched one)
}

// 16-byte aligned arenas; the ranges start kPad + alignment into them
alignas(16) uint8_t src_arena[2 * kPad + 16 + kMaxLen];
alignas(16) uint8_t dst_arena[2 * kPad + 16 + kMaxLen];
uint8_t writes[sizeof dst_arena];

template <int U>
void run_case(const Case &cs) {
    const uint8_t *src = src_arena + kPad + cs.sa;
    uint8_t *dst = dst_arena + kPad + cs.da;
    const uint64_t len = cs.len;
    const size_t lo = kPad + cs.da - 32, span = (size_t)len + 64;  // what a stray store could plausibly hit
    std::memset(dst_arena + lo, kSentinel, span);
    std::memset(writes + lo, 0, span);
    uint64_t dwords = 0;

    const auto byte = [&](uint64_t i) {
        CHECK(i < len);
        if (i >= len) return;
        dst[i] = src[i];
        ++writes[dst - dst_arena + i];
    };
    const auto load = [&](const uint32_t *q) -> uint32_t {
        const uintptr_t a = (uintptr_t)q, s = (uintptr_t)src;
        const bool ok = (a & 3) == 0 && a + 4 > s && a < s + len;  // aligned, and holds a source byte
        CHECK(ok);
        ++dwords;
        if (!ok) return 0;
        uint32_t v;
        std::memcpy(&v, q, 4);
        return v;
    };
    const auto store = [&](psy::CopyWords *at, psy::CopyWords w) {
        uint8_t *p = reinterpret_cast<uint8_t *>(at);
        const bool ok = ((uintptr_t)p & 15) == 0 && p >= dst && p + 16 <= dst + len;
        CHECK(ok);
        if (!ok) return;
        const uint32_t v[4] = {w.x, w.y, w.z, w.w};
        std::memcpy(p, v, 16);  // (little-endian, as the device)
        for (int i = 0; i < 16; ++i) ++writes[p - dst_arena + i];
    };
    for (uint64_t t = 0; t < cs.T; ++t) psy::copy_shifted_with<U>(dst, src, len, t, cs.T, byte, load, store);

    CHECK(std::memcmp(dst, src, len) == 0);
    bool once = true, clean = true;
    for (size_t i = 0; i < span; ++i) {
        const size_t a = lo + i;
        const bool inside = a >= (size_t)(dst - dst_arena) && a < (size_t)(dst - dst_arena) + len;
        if (inside) once = once && writes[a] == 1;
        else clean = clean && writes[a] == 0 && dst_arena[a] == kSentinel;
    }
    CHECK(once);
    CHECK(clean);
    // the split itself: a head short of 16 that ends on the boundary, whole chunks, a tail short of 16
    const uint64_t head = psy::copy_head((uintptr_t)dst, len);
    CHECK(head <= len && head < 16 && (head == len || (((uintptr_t)dst + head) & 15) == 0));
    const psy::CopyChunks c = psy::copy_chunks((uintptr_t)(src + head), len - head);
    CHECK(head + 16 * c.nb <= len && len - (head + 16 * c.nb) < 16);
    CHECK(c.sw + c.sh / 8 == (uintptr_t)src + head && c.sh <= 24 && c.sh % 8 == 0);
    CHECK(dwords == c.nb * (c.sh ? 5u : 4u));
}

}  // namespace

int main() {
    for (size_t i = 0; i < sizeof src_arena; ++i) src_arena[i] = source_byte(i);
    std::vector<uint64_t> lens;
    for (uint64_t l = 0; l <= 96; ++l) lens.push_back(l);
    for (uint64_t l : {4095ull, 4096ull, 4097ull}) lens.push_back(l);
    long cases = 0;
    for (uint32_t da = 0; da < 16; ++da)
        for (uint32_t sa = 0; sa < 16; ++sa)
            for (uint64_t len : lens)
                for (uint64_t T : {16ull, 64ull, 512ull, 768ull})
                    for (int U : {1, 2}) {
                        const Case cs{da, sa, len, T, U};
                        if (U == 1) run_case<1>(cs);
                        else run_case<2>(cs);
                        ++cases;
                    }
    // the combine by itself: 20 known bytes at every shift
    {
        const Case cs{0, 0, 0, 0, 0};
        uint8_t b[20];
        for (int i = 0; i < 20; ++i) b[i] = (uint8_t)(i + 1);
        uint32_t w[5];
        std::memcpy(w, b, 20);
        for (uint32_t m = 0; m < 4; ++m) {
            const psy::CopyWords r = psy::copy_combine(w[0], w[1], w[2], w[3], m ? w[4] : 0u, 8 * m);
            const uint32_t v[4] = {r.x, r.y, r.z, r.w};
            CHECK(std::memcmp(v, b + m, 16) == 0);
        }
    }
    std::printf("copy shifted: %ld cases, %ld failures\n", cases, failures);
    std::printf("copy shifted: %ld failures\n", failures);
    return failures ? 1 : 0;
}
