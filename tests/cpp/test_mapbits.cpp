// The mapping bits of the known-mapping calls (psyne_amd/csrc/tdt_mapbits.h): which words are a
// usable mapping at a width (psy::mapbits_ok: what the kernels turn into TDT_E_BAD_MAPPING), the
// stream of a position, and the complement within the width.  Host code only; built with
// -fsanitize=address,undefined and run directly (tests/test_mapbits.py).  The shifts by the width
// are the point: a shift by 64 is undefined, and width 64 is a legal word size.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../psyne_amd/csrc/tdt_mapbits.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// the definition, restated bit by bit: no position at or above the width is mapped to stream 1
bool ok_ref(uint64_t bits, int ws) {
    if (ws < 1 || ws > 64) return false;
    for (int p = ws; p < 64; ++p)
        if ((bits >> p) & 1u) return false;
    return true;
}

uint64_t rnd(uint64_t &s) {  // splitmix64
    s += 0x9e3779b97f4a7c15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

}  // namespace

int main() {
    // compile-time use, as the kernels' callers may
    static_assert(psy::mapbits_ok(0x7u, 4) && !psy::mapbits_ok(0x10u, 4), "constexpr");
    static_assert(psy::mapbits_ok(~0ull, 64) && !psy::mapbits_ok(0, 0) && !psy::mapbits_ok(0, 65), "constexpr widths");

    // the widths outside 1..64 accept nothing
    for (int ws : {-64, -1, 0, 65, 66, 128, 1 << 20}) {
        CHECK(!psy::mapbits_ok(0, ws));
        CHECK(!psy::mapbits_ok(1, ws));
        CHECK(!psy::mapbits_ok(~0ull, ws));
    }
    uint64_t seed = 20240611;
    for (int ws = 1; ws <= 64; ++ws) {
        const uint64_t all = ws == 64 ? ~0ull : (1ull << ws) - 1ull;
        CHECK(psy::mapbits_ok(0, ws));
        CHECK(psy::mapbits_ok(all, ws));
        CHECK(psy::mapbits_ok(1ull << (ws - 1), ws));
        // every single bit: usable exactly when it lies below the width; and on top of a full mapping
        for (int p = 0; p < 64; ++p) {
            CHECK(psy::mapbits_ok(1ull << p, ws) == (p < ws));
            CHECK(psy::mapbits_ok(all | (1ull << p), ws) == (p < ws));
        }
        // random words, and random words cut to the width
        for (int k = 0; k < 2000; ++k) {
            const uint64_t r = rnd(seed);
            CHECK(psy::mapbits_ok(r, ws) == ok_ref(r, ws));
            CHECK(psy::mapbits_ok(r & all, ws));
            // the complement stays inside the width, differs in every position, and flips back
            const uint64_t f = psy::mapbits_flip(r & all, ws);
            CHECK(psy::mapbits_ok(f, ws));
            CHECK((f ^ (r & all)) == all);
            CHECK(psy::mapbits_flip(f, ws) == (r & all));
        }
        // a mapping written position by position reads back position by position
        std::vector<uint32_t> m((size_t)ws);
        uint64_t bits = 0;
        for (int p = 0; p < ws; ++p) {
            m[(size_t)p] = (uint32_t)(rnd(seed) & 1u);
            bits |= (uint64_t)m[(size_t)p] << p;
        }
        CHECK(psy::mapbits_ok(bits, ws));
        for (int p = 0; p < ws; ++p) CHECK(psy::mapbits_at(bits, p) == m[(size_t)p]);
    }
    CHECK(psy::mapbits_at(1ull << 63, 63) == 1u);
    CHECK(psy::mapbits_flip(0, 64) == ~0ull);
    CHECK(psy::mapbits_flip(0, 1) == 1ull);
    std::printf("mapbits: %d failures\n", failures);
    return failures ? 1 : 0;
}
