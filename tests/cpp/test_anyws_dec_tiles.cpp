// Host test of the tiled generic-width decode's arithmetic (psyne_amd/csrc/tdt_anyws_dec_tiles.h): a
// tile-by-tile decode built from the header alone — block sums, the clamped prefix, the search for a
// tile's first block, the chunk walk with every pair cut to the tile, the planes and the recombine
// through the rank table — against a serial decode, over random blobs and the edge families of the
// GPU tests.  Every output byte must be written exactly once.  A program of its own (built with
// AddressSanitizer and UBSan by tests/test_anyws_dec_tiles.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../psyne_amd/csrc/tdt_anyws_dec_tiles.h"

using namespace psy;

namespace {

struct Blob {
    uint32_t ws = 0, orig = 0;
    std::vector<int> map;                  // position -> referenced stream (0 or 1)
    std::vector<uint8_t> stream[2];        // (count, value) pairs, maybe an odd trailing byte
};

int g_fail = 0, g_blobs = 0;
void fail(const std::string &what) {
    if (++g_fail <= 20) std::printf("FAIL %s\n", what.c_str());
}

// the serial decode: lazily, never past a stream's share
std::vector<uint8_t> serial(const Blob &b) {
    std::vector<uint8_t> out(b.orig, 0);
    const uint32_t wc = b.orig / b.ws;
    for (int r = 0; r < 2; ++r) {
        std::vector<uint8_t> P;
        for (uint32_t p = 0; p < b.ws; ++p)
            if (b.map[p] == r) P.push_back((uint8_t)p);
        const uint32_t k = (uint32_t)P.size();
        if (!k) continue;
        const uint64_t S = (uint64_t)wc * k;
        uint64_t q = 0;
        const size_t np = b.stream[r].size() / 2;
        for (size_t i = 0; i < np && q < S; ++i) {
            const uint32_t c = b.stream[r][2 * i];
            for (uint32_t j = 0; j < c && q < S; ++j, ++q) out[any_dec_out_byte((uint32_t)q, k, b.ws, P.data())] = b.stream[r][2 * i + 1];
        }
    }
    return out;
}

// the tile-by-tile decode, as the kernels do it
std::vector<uint8_t> tiled(const Blob &b, uint32_t tile, std::vector<uint8_t> &writes) {
    std::vector<uint8_t> out(b.orig, 0xEE);
    writes.assign(b.orig, 0);
    const uint32_t ws = b.ws, wc = b.orig / ws, wbytes = wc * ws;
    const uint32_t tw = any_dec_tile_words(ws, tile), ntiles = any_dec_ntiles(wc, tw);
    uint32_t k[2] = {0, 0};
    std::vector<uint8_t> rank(ws);
    for (uint32_t p = 0; p < ws; ++p) rank[p] = (uint8_t)(k[b.map[p]]++ | (b.map[p] ? 0x80u : 0u));
    // block sums, then the clamped exclusive prefix
    std::vector<uint32_t> E[2];
    uint32_t np[2];
    for (int r = 0; r < 2; ++r) {
        np[r] = (uint32_t)(b.stream[r].size() / 2);
        const uint32_t nb = any_dec_nblocks(np[r]);
        E[r].assign(nb, 0);
        for (uint32_t i = 0; i < np[r]; ++i) E[r][i / kAnyDecBlockPairs] += b.stream[r][2 * (size_t)i];
        const uint32_t S = wc * k[r];
        uint32_t carry = 0;
        for (uint32_t i = 0; i < nb; ++i) {
            const uint32_t sum = E[r][i];
            if (sum > kAnyDecBlockMax) fail("block sum above its bound");
            E[r][i] = carry;
            carry = any_dec_scan_step(carry, sum, S);
        }
    }
    std::vector<uint8_t> plane(tile + 16);
    for (uint32_t t = 0; t < ntiles; ++t) {
        const AnyDecWords W = any_dec_tile_words_of(t, wc, tw);
        const AnyDecBytes J = any_dec_tile_bytes(t, ntiles, W, ws, b.orig);
        if (W.w0 != t * tw || W.w1 > wc || W.w1 <= W.w0 || (t + 1 == ntiles) != (W.w1 == wc)) fail("tile words");
        const uint32_t nw = W.w1 - W.w0, off1 = (nw * k[0] + 15u) & ~15u;
        if (off1 + nw * k[1] > plane.size()) fail("planes larger than a tile");
        std::fill(plane.begin(), plane.end(), 0);
        for (int r = 0; r < 2; ++r) {
            if (!k[r] || !np[r]) continue;
            const AnyDecRange R = any_dec_stream_range(W, k[r]);
            const uint32_t nb = (uint32_t)E[r].size();
            const uint32_t blk = any_dec_first_block([&](uint32_t i) { return E[r].at(i); }, nb, R.q0);
            if (E[r][blk] > R.q0 || (blk + 1 < nb && E[r][blk + 1] <= R.q0)) fail("first block is not the largest one at or below q0");
            uint64_t q = E[r][blk];
            uint8_t *pl = plane.data() + (r ? off1 : 0);
            for (uint32_t pc = blk * kAnyDecBlockPairs; pc < np[r] && q < R.q1; pc += kAnyDecBlockPairs) {
                const uint32_t pe = np[r] - pc < kAnyDecBlockPairs ? np[r] : pc + kAnyDecBlockPairs;
                for (uint32_t i = pc; i < pe; ++i) {
                    const uint32_t c = b.stream[r][2 * (size_t)i];
                    const AnyDecClip cl = any_dec_clip(q, c, R.q0, R.q1);
                    if (cl.n && cl.off + cl.n > R.q1 - R.q0) fail("clip past the plane");
                    for (uint32_t j = 0; j < cl.n; ++j) pl[cl.off + j] = b.stream[r][2 * (size_t)i + 1];
                    q += c;
                }
            }
        }
        for (uint32_t j = J.jb; j < J.je; ++j) {
            uint8_t v = 0;
            if (j < wbytes) {
                const uint32_t w = j / ws, p = j - w * ws, rk = rank[p];
                v = plane.at(((rk & 0x80u) ? off1 + (w - W.w0) * k[1] : (w - W.w0) * k[0]) + (rk & 63u));
            }
            out[j] = v;
            ++writes[j];
        }
    }
    return out;
}

void check(const Blob &b, const char *name) {
    ++g_blobs;
    const std::vector<uint8_t> want = serial(b);
    for (uint32_t tile : {kAnyDecTile, 4096u, 1024u}) {
        if (tile < b.ws) continue;
        std::vector<uint8_t> writes;
        const std::vector<uint8_t> got = tiled(b, tile, writes);
        if (got != want) fail(std::string(name) + ": bytes differ at tile " + std::to_string(tile));
        for (uint8_t w : writes)
            if (w != 1) {
                fail(std::string(name) + ": a byte not written exactly once");
                break;
            }
    }
}

void push_pairs(std::vector<uint8_t> &s, uint32_t count, uint32_t n, uint8_t &val) {
    for (uint32_t i = 0; i < n; ++i) {
        s.push_back((uint8_t)count);
        s.push_back(val = (uint8_t)(val * 5 + 3));
    }
}
// pairs whose counts sum to `total`: counts in 1..maxrun, count-0 pairs with probability zf
void random_pairs(std::mt19937 &g, std::vector<uint8_t> &s, uint64_t total, uint32_t maxrun, double zf) {
    uint8_t val = (uint8_t)g();
    std::uniform_real_distribution<double> u(0, 1);
    while (total) {
        uint32_t c = u(g) < zf ? 0u : 1u + g() % maxrun;
        if (c > total) c = (uint32_t)total;
        push_pairs(s, c, 1, val);
        total -= c;
    }
}
std::vector<int> mapping_of(std::mt19937 &g, uint32_t ws, int kind) {
    std::vector<int> m(ws);
    for (uint32_t p = 0; p < ws; ++p)
        m[p] = kind == 0 ? (p < ws / 2 ? 1 : 0) : kind == 1 ? (p < ws / 2 ? 0 : 1) : kind == 2 ? (int)(p & 1) : kind == 3 ? 0 : (int)(g() & 1);
    return m;
}
uint32_t share(const Blob &b, int r) {
    uint32_t k = 0;
    for (int m : b.map) k += m == r;
    return (b.orig / b.ws) * k;
}

// a stream that reaches position `at` exactly with a pair boundary d bytes from it, runs of count-0
// pairs around it, and one pair straddling `at2` with `near` bytes before it
void edge_stream(std::mt19937 &g, std::vector<uint8_t> &s, uint64_t total, uint64_t at, int d, uint32_t near, uint32_t zeros) {
    uint8_t val = (uint8_t)g();
    uint64_t have = 0;
    auto fill_to = [&](uint64_t goal, uint32_t maxrun) {
        while (have < goal) {
            uint32_t c = 1u + g() % maxrun;
            if (c > goal - have) c = (uint32_t)(goal - have);
            push_pairs(s, c, 1, val);
            have += c;
        }
    };
    const uint64_t b0 = at + (uint64_t)(int64_t)d;
    if (b0 > 300 && b0 < total) {
        fill_to(b0 - near, 3);
        push_pairs(s, 0, zeros, val);
        if (near) {  // a pair straddling b0: `near` bytes before it
            const uint32_t c = near + (uint32_t)std::min<uint64_t>(255 - near, total - b0);
            push_pairs(s, c, 1, val);
            have += c;
        }
        push_pairs(s, 0, zeros, val);
    }
    fill_to(total, 255);
}

}  // namespace

int main() {
    std::mt19937 g(0xDEC7113);
    const uint32_t widths[] = {3, 5, 12, 40, 64, 7, 33};
    // ---- random blobs: every width and mapping shape, short, exact and long streams
    for (uint32_t ws : widths)
        for (int kind = 0; kind < 5; ++kind)
            for (int fam = 0; fam < 6; ++fam) {
                Blob b;
                b.ws = ws;
                b.map = mapping_of(g, ws, kind);
                const uint32_t tw = kAnyDecTile / ws;
                const uint32_t wc = fam == 0 ? tw : fam == 1 ? tw + 1 : fam == 2 ? 2 * tw : tw * (1 + g() % 3) + g() % tw;
                b.orig = wc * ws + (fam % 3 == 0 ? 0 : fam % 3 == 1 ? 1 : ws - 1);
                for (int r = 0; r < 2; ++r) {
                    const uint64_t S = share(b, r);
                    const uint64_t total = fam == 3 ? S / 2 : fam == 4 ? S + 1 + g() % 70000 : fam == 5 ? (S ? S - 1 : 0) : S;
                    random_pairs(g, b.stream[r], total, kind % 2 ? 3 : 255, fam == 2 ? 0.3 : 0.0);
                    if (fam == 4) b.stream[r].push_back(7);  // an odd trailing byte
                }
                check(b, "random");
            }
    // ---- pair boundaries, straddling pairs and count-0 runs at every tile boundary
    for (uint32_t ws : {3u, 12u, 64u})
        for (int kind = 0; kind < 3; ++kind) {
            const uint32_t tw = kAnyDecTile / ws;
            for (int d : {-1, 0, 1})
                for (uint32_t near : {0u, 1u, 127u, 254u})
                    for (uint32_t zeros : {0u, 3u}) {
                        Blob b;
                        b.ws = ws;
                        b.map = mapping_of(g, ws, kind);
                        b.orig = (2 * tw + 17) * ws + 1;
                        for (int r = 0; r < 2; ++r) {
                            uint32_t k = 0;
                            for (int m : b.map) k += m == r;
                            edge_stream(g, b.stream[r], share(b, r), (uint64_t)tw * k, d, near, zeros);
                        }
                        check(b, "edges");
                    }
        }
    // ---- whole blocks of count-0 pairs: at a tile's first byte and mid-tile, one and two in a row
    for (uint32_t ws : {5u, 40u})
        for (uint32_t nzero : {1u, 2u})
            for (int where = 0; where < 2; ++where)
                for (uint32_t tail : {1u, 7u, 8u, 9u, 2047u, 2048u, 2049u}) {
                    Blob b;
                    b.ws = ws;
                    b.map = mapping_of(g, ws, 2);
                    const uint32_t tw = kAnyDecTile / ws;
                    b.orig = 3 * tw * ws;
                    for (int r = 0; r < 2; ++r) {
                        uint32_t k = 0;
                        for (int m : b.map) k += m == r;
                        const uint64_t S = share(b, r), at = where ? (uint64_t)tw * k + tw * k / 2 : (uint64_t)tw * k;
                        uint8_t val = 1;
                        uint64_t have = 0;
                        auto &s = b.stream[r];
                        // whole blocks of maxrun-1..3 pairs up to `at`: the last of them cut so that a block boundary is on it
                        while (have < at) {
                            const uint32_t inblock = (uint32_t)(s.size() / 2 % kAnyDecBlockPairs);
                            uint32_t c = 1u + g() % 3;
                            if (c > at - have) c = (uint32_t)(at - have);
                            if (have + c == at && inblock != kAnyDecBlockPairs - 1) {  // pad the block with count-0 pairs first
                                push_pairs(s, 0, kAnyDecBlockPairs - 1 - inblock, val);
                            }
                            push_pairs(s, c, 1, val);
                            have += c;
                        }
                        push_pairs(s, 0, nzero * kAnyDecBlockPairs, val);
                        while (have < S) {
                            uint32_t c = 1u + g() % 200;
                            if (c > S - have) c = (uint32_t)(S - have);
                            push_pairs(s, c, 1, val);
                            have += c;
                        }
                        push_pairs(s, 0, tail, val);  // np modulo the block size
                    }
                    check(b, "zero blocks");
                }
    // ---- streams of length 0, of count-0 pairs only, of one odd byte; one referenced stream only
    for (uint32_t ws : {3u, 12u, 64u})
        for (int fam = 0; fam < 4; ++fam) {
            Blob b;
            b.ws = ws;
            b.map = mapping_of(g, ws, fam == 3 ? 3 : 0);
            b.orig = (2 * (kAnyDecTile / ws) + 5) * ws + ws - 1;
            random_pairs(g, b.stream[0], share(b, 0), 3, 0.1);
            uint8_t val = 9;
            if (fam == 1) push_pairs(b.stream[1], 0, 5000, val);
            if (fam == 2) b.stream[1].push_back(200);
            check(b, "degenerate");
        }
    // ---- the search on prefixes with duplicates
    {
        const uint32_t E[] = {0, 0, 0, 5, 5, 9, 9, 9, 20};
        const uint32_t want_at[][2] = {{0, 2}, {4, 2}, {5, 4}, {8, 4}, {9, 7}, {19, 7}, {20, 8}, {4000000000u, 8}};
        for (auto &w : want_at)
            if (any_dec_first_block([&](uint32_t i) { return E[i]; }, 9, w[0]) != w[1]) fail("search with duplicates");
        if (any_dec_first_block([&](uint32_t i) { return E[i]; }, 1, 77) != 0) fail("search over one block");
        ++g_blobs;
    }
    // ---- counts that sum past 2^32: 16,843,010 pairs of 255, three tiles of output
    {
        Blob b;
        b.ws = 12;
        b.map = mapping_of(g, 12, 0);
        b.orig = 3 * kAnyDecTile / 12 * 12;
        uint8_t val = 3;
        b.stream[0].reserve(2ull * 16843010);
        for (uint32_t i = 0; i < 16843010u; ++i) {
            b.stream[0].push_back(255);
            b.stream[0].push_back((uint8_t)(i / 3));
        }
        random_pairs(g, b.stream[1], share(b, 1), 255, 0.0);
        (void)val;
        uint64_t sum = 0;
        for (size_t i = 0; i < b.stream[0].size(); i += 2) sum += b.stream[0][i];
        if (sum <= 0xffffffffull) fail("the long stream does not pass 2^32");
        // the clamp: the prefix never passes the share, and stays exact below it
        const uint32_t S = share(b, 0);
        uint32_t carry = 0;
        uint64_t exact = 0;
        for (uint32_t i = 0; i < any_dec_nblocks(16843010u); ++i) {
            if (exact < S ? carry != exact : carry != S) fail("clamped prefix");
            carry = any_dec_scan_step(carry, kAnyDecBlockMax, S);
            exact += kAnyDecBlockMax;
        }
        if (any_dec_scan_step(0xfffffff0u, kAnyDecBlockMax, 0xffffffffu) != 0xffffffffu) fail("clamp near 2^32");
        check(b, "past 2^32");
    }
    std::printf("anyws dec tiles: %d blobs, %d failures\n", g_blobs, g_fail);
    return g_fail ? 1 : 0;
}
