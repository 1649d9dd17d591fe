// The scan arithmetic of the tiled decode-reduce (psyne_amd/csrc/tdt_red_tiles.h) against a walk over
// pair lists: for random streams, the tiles each block's range covers (red_block_tiles, as the scan
// kernel applies it) and where each tile's decode starts (red_tile_carry) must name the block that
// holds the pair covering position t * TS - 1 and that block's first start, or "the stream ended".
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../psyne_amd/csrc/tdt_red_tiles.h"

using namespace psy;

static int failures = 0;
#define CHECK(c, ...)                      \
    do {                                   \
        if (!(c)) {                        \
            if (++failures <= 10) {        \
                std::printf("FAIL " #c ": "); \
                std::printf(__VA_ARGS__);  \
                std::printf("\n");         \
            }                              \
        }                                  \
    } while (0)

int main() {
    std::mt19937 rng(2711);
    int streams = 0;
    for (int it = 0; it < 400; ++it) {
        const uint32_t seg = 4u * (1u + rng() % 4u);
        const uint64_t TS = (uint64_t)kRedTileGroups * seg;
        const uint32_t np = it < 4 ? (uint32_t)it : 1u + rng() % 6000u;
        const int shape = it % 4;  // counts: any, long runs, many zeros, all zeros in whole blocks
        std::vector<uint8_t> cnt(np);
        for (uint32_t i = 0; i < np; ++i) {
            const uint32_t x = rng();
            cnt[i] = shape == 1 ? (uint8_t)(200 + x % 56) : shape == 2 ? (uint8_t)((x & 3) ? 0 : x >> 24)
                   : shape == 3 && (i / 700) % 2 ? 0 : (uint8_t)(x >> 24);
        }
        uint64_t total = 0;
        for (uint8_t c : cnt) total += c;
        // a destination a little shorter, equal or longer than the stream decodes to
        const uint64_t want = total + (it % 3 == 0 ? 0 : it % 3 == 1 ? 3 * TS / 2 : 0) - (it % 3 == 2 ? total / 3 : 0);
        const uint64_t osize = (want / seg + 1) * 16;
        const uint32_t gc = (uint32_t)((osize + 15) / 16), nt = red_ntiles(osize);
        CHECK(nt == (gc + kRedTileGroups - 1) / kRedTileGroups, "ntiles %u gc %u", nt, gc);
        uint32_t cover = 0;
        for (uint32_t t = 0; t < nt; ++t) {
            const RedGroups G = red_tile_groups(t, gc);
            CHECK(G.g_lo == cover && G.g_hi > G.g_lo && G.g_lo % (64 * kRedWinRounds) == 0, "tile %u groups", t);
            cover = G.g_hi;
        }
        CHECK(cover == gc && red_tile_groups(nt, gc).g_lo == red_tile_groups(nt, gc).g_hi, "cover %u of %u", cover, gc);
        // the block pass and the scan
        const uint32_t nb = red_nblocks(np);
        CHECK((uint64_t)nb <= red_block_claim(2ull * np), "block claim");
        std::vector<uint32_t> bsum(nb, 0), tblk(nt, 0xdeadbeefu);
        for (uint32_t i = 0; i < np; ++i) bsum[i / kRedBlockPairs] += cnt[i];
        uint64_t run = 0;
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t v = bsum[b];
            bsum[b] = (uint32_t)run;
            const RedTileSpan s = red_block_tiles(run, v, TS, nt);
            for (uint64_t t = s.t0; t < s.t1; ++t) {
                CHECK(t >= 1 && t < nt && tblk[t] == 0xdeadbeefu, "tile %llu claimed twice", (unsigned long long)t);
                if (t < nt) tblk[t] = b;
            }
            run += v;
        }
        CHECK(run == total, "scan total");
        const uint32_t slen = (uint32_t)run;
        // brute force: the pair covering position P - 1
        for (uint32_t t = 1; t < nt; ++t) {
            const uint32_t P = (uint32_t)(t * TS);
            const RedCarry c = red_tile_carry(P, slen, tblk[t], [&](uint32_t b) { return bsum[b]; });
            uint64_t start = 0;
            uint32_t wb = kRedNoBlock;
            for (uint32_t i = 0; i < np; ++i) {
                if (start <= P - 1u && P - 1u < start + cnt[i]) wb = i / kRedBlockPairs;
                start += cnt[i];
            }
            if (wb == kRedNoBlock) {
                CHECK(c.b0 == kRedNoBlock && c.s0 == slen && total <= P - 1u, "tile %u: ended stream", t);
            } else {
                uint64_t s0 = 0;
                for (uint32_t i = 0; i < wb * kRedBlockPairs; ++i) s0 += cnt[i];
                CHECK(c.b0 == wb && c.s0 == s0, "tile %u: block %u start %u, want %u %llu", t, c.b0, c.s0, wb,
                      (unsigned long long)s0);
            }
        }
        ++streams;
    }
    std::printf("red tiles: %d streams, %d failures\n", streams, failures);
    return failures != 0;
}
