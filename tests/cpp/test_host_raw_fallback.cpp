// tests/cpp/test_host_raw_fallback.cpp — the raw fallback of the host path (TDT_OPT_HOST_RAW_FALLBACK)
// through the C++ layers (GPU codec):
//   * HipTDTCompressionProtocol::set_raw_fallback(true): a dense 64 KiB message encodes to n + 4 bytes,
//     "UNCP" + the message, and decodes back; transformation_ratio() is unchanged by it; a 70 %-zero
//     gradient encodes to the same bytes as a protocol without the option;
//   * TdtSubstrate<PosixTcpSubstrate> with Defaults::raw_fallback over 127.0.0.1: send_batch of
//     {dense, gradient, uniform, 60-byte} delivers the payloads intact, and its wire bytes are
//     Σ min(E_i, n_i + 4) plus the 4-byte frame headers, E_i being the frames of a second decorator pair
//     with the option off.
// Prints "cpp host raw fallback OK" on success.
#include <psyne_amd/tdt_substrate.hpp>

#include <cstdio>
#include <random>

using namespace psyne_amd;

static std::vector<uint8_t> floats_of(const std::vector<float> &g) {
    const uint8_t *p = reinterpret_cast<const uint8_t *>(g.data());
    return std::vector<uint8_t>(p, p + g.size() * 4);
}
static std::vector<uint8_t> grad(std::mt19937 &rng, size_t floats) {  // 70 % zeros: compresses
    std::normal_distribution<float> nd(0.f, 0.01f);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    std::vector<float> g(floats);
    for (auto &x : g) x = u(rng) < 0.7f ? 0.f : nd(rng);
    return floats_of(g);
}
static std::vector<uint8_t> dense(std::mt19937 &rng, size_t floats) {  // no zeros: expands at width 4
    std::normal_distribution<float> nd(0.f, 1e-3f);
    std::vector<float> g(floats);
    for (auto &x : g) {
        x = nd(rng);
        if (x == 0.f) x = 1e-3f;
    }
    return floats_of(g);
}
static std::vector<uint8_t> uniform(std::mt19937 &rng, size_t n) {
    std::vector<uint8_t> v(n);
    for (auto &x : v) x = (uint8_t)rng();
    return v;
}

#define CHECK(c, msg)                                   \
    do {                                                \
        if (!(c)) {                                     \
            std::printf("FAILED: %s\n", msg);           \
            return 1;                                   \
        }                                               \
    } while (0)

using Sub = TdtSubstrate<PosixTcpSubstrate>;

int main() {
    std::mt19937 rng(2027);
    TDTConfig cfg;
    cfg.sample_fraction = 1.0f;
    const uint8_t uncp[4] = {0x50, 0x43, 0x4E, 0x55};

    // ---- the protocol class
    {
        HipTDTCompressionProtocol on(cfg), off(cfg);
        on.update_network_metrics(10.0, 1.0);  // compression on
        off.update_network_metrics(10.0, 1.0);
        CHECK(!on.raw_fallback(), "default off");
        on.set_raw_fallback(true);
        CHECK(on.raw_fallback() && !off.raw_fallback(), "set_raw_fallback");
        std::vector<uint8_t> g = grad(rng, 16384), d = dense(rng, 16384);
        const std::vector<uint8_t> bg_on = on.encode(g.data(), g.size()), bg_off = off.encode(g.data(), g.size());
        CHECK(bg_on.size() < g.size() && bg_on == bg_off, "a compressing message keeps its TDT blob");
        const double ratio = on.transformation_ratio();
        const std::vector<uint8_t> bd_off = off.encode(d.data(), d.size());
        CHECK(bd_off.size() > d.size() + 4, "the dense message expands without the option");
        const std::vector<uint8_t> bd = on.encode(d.data(), d.size());
        CHECK(bd.size() == d.size() + 4, "dense: n + 4 bytes");
        CHECK(std::memcmp(bd.data(), uncp, 4) == 0 && std::memcmp(bd.data() + 4, d.data(), d.size()) == 0, "dense: UNCP + x");
        CHECK(on.transformation_ratio() == ratio, "a fallen-back message leaves the ratio");
        CHECK(on.decode(bd) == d && on.decode(bg_on) == g && off.decode(bd) == d, "decode back");
        uint64_t v = 99;
        CHECK(tdt_ctx_get_stat(on.context(), TDT_STAT_HOST_RAW_FALLBACKS, &v) == TDT_OK, "stat readable");
    }

    // ---- the decorator: one pair with Defaults::raw_fallback, one without
    std::vector<std::vector<uint8_t>> msgs = {dense(rng, 16384), grad(rng, 16384), uniform(rng, 65536), uniform(rng, 60)};
    std::vector<const void *> ptr;
    std::vector<size_t> sz;
    for (auto &m : msgs) ptr.push_back(m.data()), sz.push_back(m.size());
    const size_t n = msgs.size();
    Sub::defaults().bandwidth_mbps = 10.0;
    auto run = [&](uint16_t port, bool raw, std::vector<uint64_t> &blob_len, size_t &wire, size_t &framed) -> int {
        Sub::defaults().raw_fallback = raw;
        Sub rx(cfg, "127.0.0.1", port, true);
        Sub tx(cfg, "127.0.0.1", port, false);
        CHECK(rx.inner().wait_for_connection() && tx.inner().wait_for_connection(), "connect");
        CHECK(tx.codec().raw_fallback() == raw, "Defaults::raw_fallback applied");
        tx.record_last_batch(true);
        wire = tx.send_batch(ptr.data(), sz.data(), n);
        std::vector<uint8_t> out;
        std::vector<uint64_t> off;
        const std::vector<int32_t> st = rx.receive_batch(n, 1 << 18, out, off);
        tx.flush();
        for (size_t i = 0; i < n; ++i) {
            CHECK(st[i] == TDT_OK && off[i + 1] - off[i] == msgs[i].size(), "delivered size");
            CHECK(std::memcmp(out.data() + off[i], msgs[i].data(), msgs[i].size()) == 0, "delivered payload");
        }
        blob_len.clear();
        for (size_t i = 0; i < n; ++i) blob_len.push_back(tx.last_batch_offsets()[i + 1] - tx.last_batch_offsets()[i]);
        framed = tx.inner().get_bytes_sent();
        return 0;
    };
    std::vector<uint64_t> e_plain, e_raw;
    size_t wire_plain = 0, wire_raw = 0, framed_plain = 0, framed_raw = 0;
    if (run((uint16_t)18211, false, e_plain, wire_plain, framed_plain)) return 1;
    if (run((uint16_t)18212, true, e_raw, wire_raw, framed_raw)) return 1;
    Sub::defaults().raw_fallback = false;
    uint64_t want = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t m = std::min<uint64_t>(e_plain[i], msgs[i].size() + 4);
        CHECK(e_raw[i] == m, "frame i is min(E_i, n_i + 4) bytes");
        want += m;
    }
    CHECK(e_plain[0] > msgs[0].size() + 4 && e_plain[2] > msgs[2].size() + 4, "dense and uniform expand without the option");
    CHECK(e_plain[1] < msgs[1].size() && e_plain[3] == 64, "the gradient compresses; 60 bytes are routed to UNCP");
    CHECK(wire_raw == want && framed_raw == want + 4 * n, "wire bytes with the option");
    CHECK(framed_plain == wire_plain + 4 * n && wire_plain > want, "wire bytes without it");
    std::printf("cpp host raw fallback OK wire %zu -> %zu\n", wire_plain, wire_raw);
    return 0;
}
