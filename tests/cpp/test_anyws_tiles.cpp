// The tile arithmetic of the tiled generic-width encode (psyne_amd/csrc/tdt_anyws_tiles.h): a
// tile's stream range, its predecessor byte, the pairs of a run and the scan's combine, driven as
// the count, scan and emit kernels drive them over messages built from random and adversarial
// run-start sets.  Checked, per stream: the tiles' stream ranges partition the stream in order; the
// predecessor byte is the stream byte before the tile's first; every tile's pair base plus the
// pairs it writes is the serial encoder's pair count at the tile's end; and the pairs the tiles
// write, each at its base, are the serial encoder's pairs.  Host code only; built with
// -fsanitize=address,undefined and run directly (tests/test_anyws_tiles.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

#include "../../psyne_amd/csrc/tdt_anyws_tiles.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

using Pairs = std::vector<std::pair<uint8_t, uint8_t>>;  // (count, value)

// simple_rle_compress, serially
Pairs serial_rle(const std::vector<uint8_t> &x) {
    Pairs out;
    size_t i = 0;
    while (i < x.size()) {
        size_t L = 1;
        while (i + L < x.size() && x[i + L] == x[i] && L < 255) ++L;
        out.push_back({(uint8_t)L, x[i]});
        i += L;
    }
    return out;
}

// a stream of S bytes whose run starts are `starts` (ascending, starts[0] == 0): neighbouring runs differ
std::vector<uint8_t> stream_of(uint32_t S, const std::vector<uint32_t> &starts) {
    std::vector<uint8_t> x(S);
    uint8_t v = 7;
    size_t k = 0;
    for (uint32_t q = 0; q < S; ++q) {
        if (k < starts.size() && starts[k] == q) {
            v = (uint8_t)(v * 5u + 3u);  // (odd multiplier + odd step: never the same value twice in a row)
            ++k;
        }
        x[q] = v;
    }
    return x;
}

void emit_run(Pairs &out, uint32_t at, uint32_t L, uint8_t val, uint32_t &written) {
    for (; L > 255u; L -= 255u) out[at + written++] = {255, val};
    out[at + written++] = {(uint8_t)L, val};
}

// One message at width ws, mapping `bits`, tile size T, with the given run starts per stream.
void check_message(uint32_t ws, uint64_t bits, uint32_t wc, uint32_t T, const std::vector<uint32_t> (&starts)[2]) {
    const uint32_t n = ws * wc;
    const uint32_t k[2] = {psy::any_before(bits, 0, ws), psy::any_before(bits, 1, ws)};
    CHECK(k[0] + k[1] == ws);
    std::vector<uint8_t> stream[2], msg(n);
    for (uint32_t s = 0; s < 2; ++s) stream[s] = stream_of(wc * k[s], starts[s]);
    {
        uint32_t at[2] = {0, 0};
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t s = (uint32_t)((bits >> (j % ws)) & 1u);
            CHECK(psy::any_stream_pos(j, ws, bits, s) == at[s]);
            msg[j] = stream[s][at[s]++];
        }
    }
    const uint32_t nt = (n + T - 1) / T;
    for (uint32_t s = 0; s < 2; ++s) {
        const uint32_t S = wc * k[s];
        if (!S) continue;
        const std::vector<uint8_t> &x = stream[s];
        const Pairs want = serial_rle(x);
        // serial pair count of x[0, q) closed by a start at q (or the end): pairs before position q
        std::vector<uint32_t> pairs_before(S + 1, 0);
        {
            uint32_t run0 = 0, acc = 0;
            for (uint32_t q = 1; q <= S; ++q)
                if (q == S || x[q] != x[q - 1]) {
                    acc += psy::any_run_pairs(q - run0);
                    pairs_before[q] = acc;
                    run0 = q;
                }
            CHECK(acc == want.size());
        }
        // count: every tile alone
        std::vector<psy::AnyTileRuns> rec(nt);
        uint32_t cursor = 0;
        for (uint32_t t = 0; t < nt; ++t) {
            const uint32_t jb = t * T, je = std::min(n, jb + T);
            const psy::AnyRange r = psy::any_tile_range(jb, je, ws, bits, s);
            CHECK(r.b == cursor && r.e >= r.b && r.e <= S);
            cursor = r.e;
            uint8_t prev = 0;
            if (r.b) {
                const uint32_t pj = psy::any_pred_pos(jb, ws, bits, s);
                CHECK(pj < jb && jb - pj <= ws && ((bits >> (pj % ws)) & 1u) == s);
                CHECK(psy::any_stream_pos(pj, ws, bits, s) == r.b - 1);
                if (pj < jb) prev = msg[pj];
            }
            psy::AnyTileRuns a{0, 0, 0};
            for (uint32_t q = r.b; q < r.e; ++q) {
                if (q == 0 || x[q] != prev) {
                    if (a.first == 0) a.first = q + 1;
                    else a.inner += psy::any_run_pairs(q - (a.last - 1));
                    a.last = q + 1;
                }
                prev = x[q];
            }
            rec[t] = a;
        }
        CHECK(cursor == S);
        // scan: carries and pair bases
        std::vector<psy::AnyCarry> carry(nt + 1);
        carry[0] = psy::AnyCarry{0, 0};
        for (uint32_t t = 0; t < nt; ++t) carry[t + 1] = psy::any_scan_step(carry[t], rec[t]);
        const uint32_t total = carry[nt].pairs + psy::any_final_pairs(S, carry[nt].start);
        CHECK(total == want.size());
        if (total != want.size()) continue;
        // emit: every tile alone, from its carry and base
        Pairs got(total, {0, 0});
        uint32_t next_base = 0;
        for (uint32_t t = 0; t < nt; ++t) {
            const uint32_t jb = t * T, je = std::min(n, jb + T);
            const psy::AnyRange r = psy::any_tile_range(jb, je, ws, bits, s);
            CHECK(carry[t].pairs == next_base);  // the tiles' pair ranges partition the stream's in order
            uint32_t rs = carry[t].start, written = 0;
            for (uint32_t q = r.b; q < r.e; ++q) {
                if (q != 0 && x[q] == x[q - 1]) continue;
                if (q != 0) emit_run(got, carry[t].pairs, q - (rs - 1), x[q - 1], written);
                rs = q + 1;
            }
            CHECK(written == psy::any_tile_pairs(rec[t], carry[t].start));
            // pair base + pairs written = the serial encoder's pairs up to the tile's last start
            const uint32_t upto = rs ? rs - 1 : 0;
            CHECK(carry[t].pairs + written == pairs_before[upto]);
            next_base = carry[t].pairs + written;
            if (t == nt - 1) {
                CHECK(rs == carry[nt].start);
                emit_run(got, carry[t].pairs, S - (rs - 1), x[S - 1], written);
                CHECK(carry[t].pairs + written == total);
            }
        }
        CHECK(got == want);
    }
}

uint64_t mapping(uint32_t ws, int kind, std::mt19937 &rng) {
    const uint64_t all = ws >= 64 ? ~0ull : (1ull << ws) - 1;
    uint64_t bits = 0;
    switch (kind) {
        case 0: bits = (1ull << (ws / 2)) - 1; break;        // stream 1 low
        case 1: bits = all & ~((1ull << (ws / 2)) - 1); break;  // stream 1 high
        case 2: bits = 0x5555555555555555ull; break;          // interleaved
        case 3: bits = 0x9249249249249249ull; break;          // every third
        case 4: bits = 0; break;                              // one stream
        case 5: bits = all; break;                            // stream 0 empty
        case 6: bits = 1; break;
        case 7: bits = 1ull << (ws - 1); break;
        default: bits = ((uint64_t)rng() << 32) | rng(); break;
    }
    return bits & all;
}

// run starts of a stream of S bytes: 0, then `kind` picks the set
std::vector<uint32_t> start_set(uint32_t S, int kind, const std::vector<uint32_t> &edges, std::mt19937 &rng) {
    std::vector<uint32_t> st{0};
    auto add = [&](uint64_t q) {
        if (q > 0 && q < S) st.push_back((uint32_t)q);
    };
    switch (kind) {
        case 0: break;  // constant: one run, which is also the final one
        case 1:         // every byte
            for (uint32_t q = 1; q < S; ++q) add(q);
            break;
        case 2:  // runs ending at, starting at, and 255-caps landing on every tile edge and beside it
            for (uint32_t e : edges)
                for (int d = -1; d <= 1; ++d) {
                    add((uint64_t)e + d);
                    add((uint64_t)e + d - 255);
                    add((uint64_t)e + d - 510);
                    add((uint64_t)e + d + 255);
                }
            break;
        case 3:  // crossing runs of the cap's neighbours
            for (size_t i = 0; i < edges.size(); ++i) {
                static const uint32_t len[] = {254, 255, 256, 510, 511, 765};
                const uint32_t L = len[i % 6], e = edges[i];
                add((uint64_t)e - L / 2);
                add((uint64_t)e - L / 2 + L);
            }
            break;
        case 4:  // one start far in: the runs before and behind it span whole tiles
            add(S - S / 7);
            break;
        case 5:
            add(1);
            add(S - 1);
            break;
        default: {
            std::geometric_distribution<uint32_t> g(kind == 6 ? 0.5 : 0.002);
            for (uint64_t q = g(rng) + 1; q < S; q += g(rng) + 1) add(q);
        }
    }
    std::sort(st.begin(), st.end());
    st.erase(std::unique(st.begin(), st.end()), st.end());
    return st;
}

}  // namespace

int main() {
    std::mt19937 rng(20250607);
    static const uint32_t widths[] = {3, 5, 12, 40, 64};
    long messages = 0;
    for (uint32_t ws : widths)
        for (int mk = 0; mk < 11; ++mk) {
            const uint64_t bits = mapping(ws, mk, rng);
            for (uint32_t T : {64u, 1024u, 65536u}) {
                // two to five tiles and a partial last one (also one holding less than a word)
                const uint32_t tiles = 2 + (uint32_t)(rng() % 4);
                const uint32_t extra = mk % 3 == 0 ? 1 : 1 + (uint32_t)(rng() % (T / ws + 1));
                const uint32_t wc = (tiles * T) / ws + extra;
                const uint32_t n = wc * ws;
                for (int kind = 0; kind < 9; ++kind) {
                    std::vector<uint32_t> starts[2];
                    for (uint32_t s = 0; s < 2; ++s) {
                        const uint32_t S = wc * psy::any_before(bits, s, ws);
                        std::vector<uint32_t> edges;  // the tile boundaries' stream bytes
                        for (uint32_t jb = T; jb < n; jb += T) edges.push_back(psy::any_stream_pos(jb, ws, bits, s));
                        if (S) starts[s] = start_set(S, (kind + (int)s * (kind > 6)) % 9, edges, rng);
                    }
                    check_message(ws, bits, wc, T, starts);
                    ++messages;
                }
            }
        }
    // the pairs of a run at the cap's edges
    CHECK(psy::any_run_pairs(1) == 1 && psy::any_run_pairs(255) == 1 && psy::any_run_pairs(256) == 2);
    CHECK(psy::any_run_pairs(510) == 2 && psy::any_run_pairs(511) == 3 && psy::any_run_pairs(0xffffffffu - 254u) == 16843009u);
    std::printf("anyws tiles: %ld messages, %d failures\n", messages, failures);
    return failures ? 1 : 0;
}
