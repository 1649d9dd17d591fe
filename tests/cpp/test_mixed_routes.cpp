// The mask-to-routes mapping of the mixed-width scattered encode (psy::mixed_routes,
// psyne_amd/csrc/tdt_plan.h): which widths a mask launches, tuned or generic, and where each
// width's pair tables lie in the call's table workspace.  Host code only; built with
// -fsanitize=address,undefined and run directly (tests/test_mixed_ws_routes.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../psyne_amd/csrc/tdt_plan.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

uint64_t mask_of(std::initializer_list<int> widths) {
    uint64_t m = 0;
    for (int w : widths) m |= 1ull << (w - 1);
    return m;
}

bool tuned(int w) { return w == 1 || w == 2 || w == 4 || w == 8 || w == 16; }

// the widths in ascending order, the split into tuned and generic, and the tables: 16-byte aligned,
// 16 * n bytes each, inside the workspace, no two overlapping (checked by painting every byte)
void check_routes(std::initializer_list<int> widths, uint32_t n) {
    psy::MixedRoutes r;
    std::memset(&r, 0xff, sizeof(r));
    CHECK(psy::mixed_routes(mask_of(widths), n, r));
    CHECK(r.n_routes == (int)widths.size());
    int k = 0, nt = 0, ng = 0;
    for (int w : widths) {  // (the lists here are ascending)
        CHECK(r.route[k].ws == w);
        CHECK(r.route[k].tuned == tuned(w));
        CHECK(psy::mixed_route_of(r, w) == k);
        (tuned(w) ? nt : ng)++;
        ++k;
    }
    CHECK(r.n_tuned == nt && r.n_generic == ng);
    CHECK(psy::mixed_route_of(r, 63) == -1 || mask_of(widths) >> 62 & 1);
    CHECK(r.bytes == 32ull * n * widths.size());
    std::vector<uint8_t> paint(r.bytes, 0);
    for (int i = 0; i < r.n_routes; ++i)
        for (int t = 0; t < psy::kPlanPairs; ++t) {
            const size_t off = r.route[i].pair[t];
            CHECK(off % 16 == 0);
            CHECK(off + 16ull * n <= r.bytes);
            if (off + 16ull * n > r.bytes) continue;
            for (size_t b = 0; b < 16ull * n; ++b) CHECK(paint[off + b]++ == 0);
        }
    for (uint8_t p : paint) CHECK(p == 1);
}

}  // namespace

int main() {
    psy::MixedRoutes r;
    // the empty mask
    CHECK(!psy::mixed_routes(0, 16, r));
    CHECK(r.n_routes == 0 && r.bytes == 0);
    // every single width
    for (int w = 1; w <= 64; ++w) {
        CHECK(psy::mixed_routes(1ull << (w - 1), 100, r));
        CHECK(r.n_routes == 1 && r.route[0].ws == w && r.route[0].tuned == tuned(w));
        CHECK(r.n_tuned == (tuned(w) ? 1 : 0) && r.n_generic == (tuned(w) ? 0 : 1));
        CHECK(r.route[0].pair[psy::PT_IN] == 0 && r.route[0].pair[psy::PT_OUT] == 1600 && r.bytes == 3200);
    }
    for (uint32_t n : {1u, 255u, 256u, 257u}) {
        check_routes({2, 4}, n);
        check_routes({1, 2, 4, 8, 16}, n);
        check_routes({3, 12}, n);
        check_routes({1, 2, 3, 4, 8, 12, 16, 64}, n);  // 8 widths: the limit
    }
    // 8 bits against 9
    static_assert(psy::kMixedMaxWidths == 8, "the ABI's limit");
    CHECK(psy::mixed_routes(0xffull, 4, r) && r.n_routes == 8);
    CHECK(psy::mixed_routes(0xff00000000000000ull, 4, r) && r.n_routes == 8 && r.route[7].ws == 64);
    CHECK(!psy::mixed_routes(0x1ffull, 4, r));
    CHECK(r.n_routes == 0 && r.bytes == 0);
    CHECK(!psy::mixed_routes(~0ull, 4, r));
    // the absent entry is no message: begin <= end for every real one
    CHECK(psy::pair_absent(psy::kAbsentBegin, psy::kAbsentEnd));
    CHECK(psy::kAbsentBegin > psy::kAbsentEnd);
    CHECK(!psy::pair_absent(0, 0) && !psy::pair_absent(~0ull, ~0ull));
    std::printf("mixed routes: %d failures\n", failures);
    return failures ? 1 : 0;
}
