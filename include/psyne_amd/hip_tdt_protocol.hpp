// hip_tdt_protocol.hpp — psyne Protocol plugin backed by the MI355X TDT codec.
//
// Drop-in for psyne::protocol::TDTCompressionProtocol
// (reference: include/psyne/protocol/tdt_compression.hpp:176-638).  Same member names,
// signatures, defaults, metric semantics and exception texts; encode/decode run on the GPU
// through the C ABI (include/psyne_tdt.h).  The class satisfies psyne's Protocol concept
// (include/psyne/concepts/protocol_concepts.hpp:22-47), restated below from its
// requirements so that this header stands alone; a psyne build can equally
// static_assert(psyne::concepts::Protocol<psyne_amd::HipTDTCompressionProtocol>).
//
// Batch extensions (encode_batch / decode_batch on device buffers, encode_batch_v / decode_batch_v
// on one device buffer per message) expose the batched
// kernels directly for callers that hold many messages (the hot path bench.py measures).
#pragma once

#include <psyne_tdt.h>

#include <atomic>
#include <chrono>
#include <concepts>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace psyne_amd {

namespace concepts {
// Restatement of psyne::concepts::Protocol (protocol_concepts.hpp:22-47).
template <typename P>
concept Protocol = requires(P protocol, void *data, size_t size) {
    { protocol.should_transform(data, size) } -> std::same_as<bool>;
    { protocol.analyze_data(data, size) } -> std::same_as<void>;
    { protocol.encode(data, size) } -> std::convertible_to<std::vector<uint8_t>>;
    { protocol.decode(std::declval<const std::vector<uint8_t> &>()) } -> std::convertible_to<std::vector<uint8_t>>;
    { protocol.update_network_metrics(0.0, 0.0) } -> std::same_as<void>;
    { protocol.update_system_metrics(0.0) } -> std::same_as<void>;
    { protocol.protocol_name() } -> std::convertible_to<const char *>;
    { protocol.is_lossless() } -> std::same_as<bool>;
    { protocol.transformation_ratio() } -> std::same_as<double>;
    { protocol.processing_overhead_ms() } -> std::same_as<double>;
};
}  // namespace concepts

// TDTConfig (tdt_compression.hpp:31-43).
struct TDTConfig {
    float sample_fraction = 0.3f;  // accepted; the GPU analyses every word (sample 1.0)
    int word_size = 4;
    bool auto_detect_clusters = true;  // declared but unused by the reference
    int max_clusters = 4;              // declared but unused by the reference
    bool enable_simd = true;           // declared but unused by the reference
    double bandwidth_threshold_mbps = 100.0;
    double cpu_usage_threshold = 0.8;
    size_t min_tensor_size = 1024;
};

class HipTDTCompressionProtocol {
public:
    explicit HipTDTCompressionProtocol(const TDTConfig &config = {}, int device = 0) : config_(config) {
        tdt_config c;
        tdt_default_config(&c);
        c.sample_fraction = config.sample_fraction;
        c.word_size = config.word_size;
        c.bandwidth_threshold_mbps = config.bandwidth_threshold_mbps;
        c.cpu_usage_threshold = config.cpu_usage_threshold;
        c.min_tensor_size = config.min_tensor_size;
        if (tdt_ctx_create(device, &c, &ctx_) != TDT_OK) throw std::runtime_error(tdt_last_error());
        push_metrics();
    }
    ~HipTDTCompressionProtocol() { tdt_ctx_destroy(ctx_); }
    HipTDTCompressionProtocol(const HipTDTCompressionProtocol &) = delete;
    HipTDTCompressionProtocol &operator=(const HipTDTCompressionProtocol &) = delete;

    // Raw fallback on the host path (TDT_OPT_HOST_RAW_FALLBACK, psyne_tdt.h; not in the reference, default
    // off): encode returns "UNCP" + the message where the TDT blob would be longer than size + 4 bytes.
    // Such a message leaves transformation_ratio() and the times as a message the policy routes to UNCP does.
    void set_raw_fallback(bool on) {
        if (tdt_ctx_set_option(ctx_, TDT_OPT_HOST_RAW_FALLBACK, on ? 1 : 0) != TDT_OK)
            throw std::runtime_error(tdt_last_error());
    }
    bool raw_fallback() const { return tdt_ctx_host_encode_bound(ctx_, 0) == 4; }

    // PROTOCOL CONCEPT IMPLEMENTATION -------------------------------------------------
    bool should_transform(void *, size_t size) { return tdt_should_transform(ctx_, size) != 0; }

    // analyze_data :206-222 — average full-sample entropy of the byte positions.
    void analyze_data(void *data, size_t size) {
        if (!(size % 4 == 0 && size >= 64)) return;  // is_tensor_data :409-413
        const size_t ws = (size_t)config_.word_size;
        const size_t words = size / ws;
        if (words == 0) {
            avg_entropy_ = 0.0;
            return;
        }
        std::vector<double> ent = analyze_host(static_cast<const uint8_t *>(data), words * ws);
        double total = 0.0;
        for (double e : ent) total += e;
        avg_entropy_ = total / (double)config_.word_size;
    }

    std::vector<uint8_t> encode(void *data, size_t size) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint64_t off[2] = {0, size};
        std::vector<uint8_t> out(tdt_ctx_host_encode_bound(ctx_, size));  // (n + 4 under set_raw_fallback)
        uint64_t ooff[2] = {0, 0};
        int32_t st = 0;
        if (tdt_encode_host(ctx_, static_cast<const uint8_t *>(data), off, 1, out.data(), out.size(), ooff, &st) !=
                TDT_OK ||
            st != TDT_OK)
            throw std::runtime_error(std::string("TDT: GPU encode failed: ") + tdt_last_error());
        out.resize(ooff[1]);
        uint32_t magic;
        std::memcpy(&magic, out.data(), 4);
        if (magic == 0x54445444u) {  // compressed: update metrics like :243-248
            uint32_t ns;
            std::memcpy(&ns, out.data() + 8, 4);
            // encoded_size() = stream bytes + mapping ints + sizeof(TDTEncodedData)=72 (:71-78)
            const double enc = double(out.size() - 20 - 4 * config_.word_size - 4 * ns) +
                               4.0 * config_.word_size + 72.0;
            last_compression_ratio_ = double(size) / enc;
            last_encode_time_ms_ =
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return out;
    }

    std::vector<uint8_t> decode(const std::vector<uint8_t> &encoded) {
        const auto t0 = std::chrono::steady_clock::now();
        if (encoded.size() < 4) throw std::runtime_error("TDT: Invalid encoded data size");
        uint32_t magic;
        std::memcpy(&magic, encoded.data(), 4);
        uint64_t cap = 0;
        if (magic == 0x554E4350u) cap = encoded.size() - 4;
        else if (magic == 0x54445444u && encoded.size() >= 8) {
            uint32_t o;
            std::memcpy(&o, encoded.data() + 4, 4);
            cap = o;
        }
        std::vector<uint8_t> out(cap ? cap : 1);
        const uint64_t off[2] = {0, encoded.size()};
        uint64_t ooff[2] = {0, 0};
        int32_t st = 0;
        if (tdt_decode_host(ctx_, encoded.data(), off, 1, out.data(), cap, ooff, &st) != TDT_OK)
            throw std::runtime_error(std::string("TDT: GPU decode failed: ") + tdt_last_error());
        if (st != TDT_OK) throw std::runtime_error(tdt_status_string(st));
        out.resize(ooff[1]);
        if (magic != 0x554E4350u)
            last_decode_time_ms_ =
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return out;
    }

    void update_network_metrics(double bandwidth_mbps, double latency_ms) {
        bandwidth_mbps_.store(bandwidth_mbps);
        latency_ms_.store(latency_ms);
        push_metrics();
    }
    void update_system_metrics(double cpu_usage) {
        cpu_usage_.store(cpu_usage);
        push_metrics();
    }

    // IDENTITY BEHAVIORS ----------------------------------------------------------------
    const char *protocol_name() const { return "TDT-Compression"; }
    bool is_lossless() const { return true; }
    double transformation_ratio() const { return last_compression_ratio_; }
    double processing_overhead_ms() const { return (last_encode_time_ms_ + last_decode_time_ms_) / 2.0; }
    double get_average_entropy() const { return avg_entropy_; }
    double get_bandwidth_mbps() const { return bandwidth_mbps_.load(); }
    double get_cpu_usage() const { return cpu_usage_.load(); }

    // BATCH EXTENSIONS (device-resident, asynchronous on `stream`) ----------------------
    int encode_batch(const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n, uint8_t *d_out, uint64_t cap,
                     uint64_t *d_out_off, int32_t *d_status, void *stream = nullptr) {
        return tdt_encode_batch(ctx_, d_in, d_in_off, n, d_out, cap, d_out_off, d_status, stream);
    }
    int decode_batch(const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n, uint8_t *d_out, uint64_t cap,
                     uint64_t *d_out_off, int32_t *d_status, void *stream = nullptr) {
        return tdt_decode_batch(ctx_, d_in, d_in_off, n, d_out, cap, d_out_off, d_status, stream);
    }
    // scattered batches: message i at d_msgs[i] (d_sizes[i] bytes), blob i at d_blobs[i] — one buffer
    // per message, as a loop of encode / decode calls holds them (tdt_encode_batch_v)
    int encode_batch_v(const uint8_t *const *d_msgs, const uint64_t *d_sizes, uint32_t n, uint8_t *const *d_blobs,
                       const uint64_t *d_blob_cap, uint64_t *d_out_len, int32_t *d_status, void *stream = nullptr) {
        return tdt_encode_batch_v(ctx_, d_msgs, d_sizes, n, d_blobs, d_blob_cap, d_out_len, d_status, stream);
    }
    // the same with one record width per message (d_word_size[i]; width_mask: bit w - 1 set for
    // every width that may occur, at most TDT_MIXED_MAX_WIDTHS of them) — a mixed-precision
    // gradient list in one call, whatever this protocol's own word_size (tdt_encode_batch_vw)
    int encode_batch_vw(const uint8_t *const *d_msgs, const uint64_t *d_sizes, const int32_t *d_word_size,
                        uint64_t width_mask, uint32_t n, uint8_t *const *d_blobs, const uint64_t *d_blob_cap,
                        uint64_t *d_out_len, int32_t *d_status, void *stream = nullptr) {
        return tdt_encode_batch_vw(ctx_, d_msgs, d_sizes, d_word_size, width_mask, n, d_blobs, d_blob_cap, d_out_len,
                                   d_status, stream);
    }
    // the packed wire buffer: blobs back to back in d_out with n + 1 offsets in d_out_off, one send per
    // batch.  encode_batch_vp: the scattered encode (d_word_size null: this protocol's width; else
    // one width per message) into such a buffer, total_bytes a host bound of the sum of d_sizes
    // (tdt_encode_batch_vp); pack_v: blobs that exist already (tdt_pack_v)
    int encode_batch_vp(const uint8_t *const *d_msgs, const uint64_t *d_sizes, const int32_t *d_word_size,
                        uint64_t width_mask, uint32_t n, uint64_t total_bytes, uint8_t *d_out, uint64_t out_cap,
                        uint64_t *d_out_off, int32_t *d_status, void *stream = nullptr) {
        return tdt_encode_batch_vp(ctx_, d_msgs, d_sizes, d_word_size, width_mask, n, total_bytes, d_out, out_cap,
                                   d_out_off, d_status, stream);
    }
    int pack_v(const uint8_t *const *d_blobs, const uint64_t *d_blob_len, uint32_t n, uint8_t *d_out, uint64_t out_cap,
               uint64_t *d_out_off, int32_t *d_status, void *stream = nullptr) {
        return tdt_pack_v(ctx_, d_blobs, d_blob_len, n, d_out, out_cap, d_out_off, d_status, stream);
    }
    int decode_batch_v(const uint8_t *const *d_blobs, const uint64_t *d_blob_len, uint32_t n, uint8_t *const *d_outs,
                       const uint64_t *d_out_cap, uint64_t *d_out_len, int32_t *d_status, void *stream = nullptr) {
        return tdt_decode_batch_v(ctx_, d_blobs, d_blob_len, n, d_outs, d_out_cap, d_out_len, d_status, stream);
    }
    tdt_ctx *context() { return ctx_; }
    int word_size() const { return config_.word_size; }

private:
    void push_metrics() { tdt_ctx_set_metrics(ctx_, bandwidth_mbps_.load(), latency_ms_.load(), cpu_usage_.load()); }

    std::vector<double> analyze_host(const uint8_t *data, size_t n) {
        std::vector<double> ent((size_t)config_.word_size, 0.0);
        const uint64_t off[2] = {0, n};
        int32_t st = 0;
        if (tdt_analyze_host(ctx_, data, off, 1, ent.data(), nullptr, &st) != TDT_OK || st != TDT_OK)
            throw std::runtime_error(std::string("TDT: GPU analyze failed: ") + tdt_last_error());
        return ent;
    }

    TDTConfig config_;
    tdt_ctx *ctx_ = nullptr;
    std::atomic<double> bandwidth_mbps_{100.0};  // :352-354
    std::atomic<double> latency_ms_{1.0};
    std::atomic<double> cpu_usage_{0.5};
    double last_compression_ratio_ = 1.0;
    double last_encode_time_ms_ = 0.0;
    double last_decode_time_ms_ = 0.0;
    double avg_entropy_ = 0.0;
};

static_assert(concepts::Protocol<HipTDTCompressionProtocol>);

}  // namespace psyne_amd

