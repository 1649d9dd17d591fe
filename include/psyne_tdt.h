/* psyne_tdt.h — C ABI of the MI355X TDT payload codec (libpsyne_tdt.so).
 *
 * Drop-in boundary for psyne's TDT protocol (include/psyne/protocol/tdt_compression.hpp
 * in the reference).  The reference exposes the codec through the C++ `Protocol` concept
 * (include/psyne/concepts/protocol_concepts.hpp:22-47), one message per call, host
 * vectors in and out.  This ABI is what a binding of that concept for the GPU binds:
 * plain pointers and sizes, batches of independent messages, device-resident buffers,
 * asynchronous on a caller-supplied hipStream_t (passed as void*).  The header-only C++
 * class psyne_amd::HipTDTCompressionProtocol (include/psyne_amd/hip_tdt_protocol.hpp)
 * layers the reference's exact Protocol surface on top of it.
 *
 * Which reference interface each entry point replaces:
 *   tdt_ctx_create / tdt_ctx_destroy  TDTCompressionProtocol(const TDTConfig&)   :178-179
 *   tdt_ctx_set_metrics               update_network_metrics / update_system_metrics :309-319
 *   tdt_should_transform              should_transform                            :186-201
 *   tdt_encode_batch                  encode                                      :227-266
 *   tdt_encode_with_mapping_batch     encode with a given cluster mapping (parity hook for
 *                                     blobs made in the reference's random-sample mode)
 *   tdt_decode_batch                  decode                                      :271-304
 *   tdt_decoded_sizes_batch           the output size decode would produce (header parse)
 *   tdt_encode_batch_into /           encode / decode into caller slots (one vector per
 *   tdt_decode_batch_into             message, as the reference returns them)
 *   tdt_encode_batch_v /              a loop of encode :227-266 / decode :271-304 over messages
 *   tdt_decode_batch_v                that lie in separate device buffers (one tensor, one
 *                                     transport_send(void*, size_t) buffer per message)
 *   tdt_decoded_sizes_v               tdt_decoded_sizes_batch over such blobs
 *   tdt_encode_batch_vp /             a loop of encode :227-266 followed by a framed send of each
 *   tdt_pack_v                        vector: the blobs back to back in one wire buffer, one send
 *   tdt_analyze_batch                 analyze_data / extract_features / perform_clustering
 *                                     :206-222, :434-525 (full-sample histograms, entropies,
 *                                     mapping per message)
 *   tdt_encode_bound /                worst-case blob size (sizing out buffers), and the same under the
 *   tdt_ctx_encode_bound /            context's options (n + 4 with TDT_OPT_RAW_FALLBACK; for the host calls
 *   tdt_ctx_host_encode_bound         n + 4 with TDT_OPT_HOST_RAW_FALLBACK)
 *   tdt_encoded_sizes_batch /         transformation_ratio (encoded size / original size) of each
 *   tdt_encoded_sizes_v               message BEFORE it is encoded: the exact blob length, no blob written
 *   tdt_mappings_v /                  analyze_data's clustering kept between encodes: the mapping of each
 *   tdt_encode_mapped_v / _vp         message as one word, and the scattered encodes with such mappings given
 *   tdt_last_error                    the reference's exception text (:128, :275)
 *
 * Wire format: identical bytes to the reference: UNCP marker
 * 0x554E4350 + payload, or TDT header | mapping | (u32 len, RLE pairs) per stream.
 *
 * Batch layout: message i occupies in[in_off[i] .. in_off[i+1]) (in_off has n+1
 * entries, device memory).  Outputs are either SLOTTED (the *_into entry points, below) or
 * COMPACTED (tdt_encode_batch / tdt_decode_batch): message i's result is written at
 * out[out_off[i] .. out_off[i+1]) and the kernel fills out_off (n+1 entries, device
 * memory) itself with a single-pass decoupled look-back, so the caller never needs the
 * sizes up front.  Per-message status codes go to status[i] if status != NULL.
 *
 * Determinism: the reference chooses the byte-plane mapping from a random 30% sample
 * (mt19937 seeded by random_device).  This codec always analyses every word — the
 * reference's sample_fraction = 1.0 behaviour — so its output is deterministic and
 * byte-identical to the reference configured that way; tdt_encode_with_mapping_batch
 * reproduces default-mode blobs given their mapping.
 */
#ifndef PSYNE_TDT_H
#define PSYNE_TDT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSYNE_TDT_ABI_VERSION 1

/* Status codes (per call and per message). */
#define TDT_OK 0
#define TDT_E_SHORT 1         /* blob < 4 bytes: "TDT: Invalid encoded data size" (:274-276) */
#define TDT_E_MAGIC 2         /* neither UNCP nor TDT magic: "Invalid TDT magic number" (:127-129) */
#define TDT_E_TRUNCATED 3     /* header or stream runs past the blob (reference: UB) */
#define TDT_E_BAD_MAPPING 4   /* mapping shorter than word_size or value >= num_streams (reference: UB) */
#define TDT_E_CAPACITY 5      /* output buffer too small for this message */
#define TDT_E_UNSUPPORTED 6   /* word_size above 64 (tdt_ctx_create, or a blob's header); a compacted
                                 encode at a word size other than 1, 2, 4, 8, 16, or with
                                 TDT_OPT_RAW_FALLBACK set, under stream capture or TDT_OPT_NO_TWO_PHASE
                                 (tdt_last_error has the text) */
#define TDT_E_BAD_HEADER 7    /* word_size == 0 in a blob (reference: division by zero) */
#define TDT_E_CONFIG 8        /* invalid tdt_config */
#define TDT_E_HIP 10          /* HIP runtime error (tdt_last_error has the text) */
#define TDT_E_ARG 11          /* invalid argument */
#define TDT_E_CAPTURE 12      /* a workspace must grow while the stream is captured: make one eager
                                 call of the batch on this context before capturing it */

/* TDTConfig (:31-43).  Fields the reference declares but never reads
 * (auto_detect_clusters, max_clusters, enable_simd) are omitted. */
typedef struct tdt_config {
    float sample_fraction;           /* accepted; the GPU always uses the full sample (1.0) */
    int32_t word_size;               /* 1..64 (the record stride: 3 RGB8, 12 float3, ...); 1, 2, 4, 8
                                        and 16 run the tuned kernels, every other width the generic
                                        ones; <= 0: TDT_E_CONFIG, > 64: TDT_E_UNSUPPORTED */
    double bandwidth_threshold_mbps; /* default 100.0 */
    double cpu_usage_threshold;      /* default 0.8 */
    uint64_t min_tensor_size;        /* default 1024 */
} tdt_config;

typedef struct tdt_ctx tdt_ctx;

void tdt_default_config(tdt_config *cfg);

/* Create a codec context bound to HIP device `device`.
 *
 * Streams: a context owns one device workspace (look-back words, error flags, slot-scan
 * sums), so its *_batch / *_slots calls must be issued on ONE stream at a time (stream order
 * keeps consecutive batches apart); use one context per stream for concurrent batches.  The
 * host calls (tdt_*_host) run on the context's own two pipeline streams and are serialised by
 * the context; they do not touch the caller's streams. */
int tdt_ctx_create(int device, const tdt_config *cfg, tdt_ctx **out);
void tdt_ctx_destroy(tdt_ctx *ctx);

/* update_network_metrics(bandwidth, latency) + update_system_metrics(cpu) (:309-319).
 * Defaults match the reference: bandwidth 100 Mbps (compression OFF), cpu 0.5. */
void tdt_ctx_set_metrics(tdt_ctx *ctx, double bandwidth_mbps, double latency_ms, double cpu_usage);
void tdt_ctx_get_metrics(const tdt_ctx *ctx, double *bandwidth_mbps, double *latency_ms, double *cpu_usage);

/* Seed for the team shape of one-pass launches whose message sizes the host does not know
 * (tdt_encode_with_mapping_batch, tdt_analyze_batch, and tdt_encode_batch under stream
 * capture): one 64-lane wave per message up to 4 KiB, a 512-lane workgroup otherwise.  Once a
 * slotted plan of this context has completed, its class counts decide instead; the slotted
 * calls, tdt_encode_batch outside capture and the host pipeline never use it.  Optional; any
 * size encodes correctly with either shape. */
void tdt_ctx_set_size_hint(tdt_ctx *ctx, uint64_t typical_message_bytes);

/* should_transform (:186-201) for a message of n bytes under the current metrics. */
int tdt_should_transform(const tdt_ctx *ctx, uint64_t n);

/* Worst-case encoded size of one n-byte message: max(n + 4, 28 + 4*ws + 2n). */
uint64_t tdt_encode_bound(uint64_t n, int32_t word_size);
/* The same for this context: n + 4 with TDT_OPT_RAW_FALLBACK set (below), else
 * tdt_encode_bound(n, the context's word_size).  What tdt_encode_slots sums and what a slot of the
 * device-batch encodes needs at most. */
uint64_t tdt_ctx_encode_bound(const tdt_ctx *ctx, uint64_t n);
/* The same for the host calls (tdt_encode_host / tdt_encode_host_v): n + 4 with TDT_OPT_HOST_RAW_FALLBACK
 * set (below), else tdt_encode_bound(n, the context's word_size).  What h_out must hold per message. */
uint64_t tdt_ctx_host_encode_bound(const tdt_ctx *ctx, uint64_t n);

/* Encode a batch.  out_cap: bytes available at d_out (use the sum of tdt_encode_bound).
 * Messages whose compressed blob would overflow out_cap get TDT_E_CAPACITY.
 * Returns TDT_OK or an argument/HIP error; per-message results go to d_status.
 * At a word size other than 1, 2, 4, 8, 16 this call and tdt_encode_with_mapping_batch always
 * encode into slots and gather (they read the batch's byte count back), so under stream capture
 * or with TDT_OPT_NO_TWO_PHASE they return TDT_E_UNSUPPORTED: capture the slotted entry points
 * (tdt_encode_slots + tdt_encode_batch_into), which read nothing back at any word size.  The same holds
 * at every word size with TDT_OPT_RAW_FALLBACK set (below); use the context's bound for out_cap then. */
int tdt_encode_batch(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs,
                     uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status,
                     void *hip_stream);

/* Encode with a caller-chosen mapping: d_mapping holds n_msgs * word_size int32 values in
 * {0, 1} (e.g. read from reference blobs at bytes 20 .. 20 + 4*ws). */
int tdt_encode_with_mapping_batch(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off,
                                  uint32_t n_msgs, const int32_t *d_mapping, uint8_t *d_out,
                                  uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status,
                                  void *hip_stream);

/* Decode a batch of blobs (any mix of UNCP and TDT, of any word sizes up to 64 whatever the
 * context's own; a blob with a larger one gets TDT_E_UNSUPPORTED).  Output compacted by decoded size. */
int tdt_decode_batch(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs,
                     uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status,
                     void *hip_stream);

/* SLOTTED batches — the hot path.  No dependency between messages: blob i goes to
 * out[slot_off[i] ..) with capacity slot_off[i+1] - slot_off[i] (slot_off: n+1 entries,
 * device memory, chosen by the caller — tdt_encode_slots gives the prefix sum of the encode
 * bounds, tdt_decode_slots the prefix sum of the decoded sizes); its length goes to
 * out_len[i] (0 with status TDT_E_CAPACITY if the slot is too small).  This is the layout of
 * the reference's API — one independent vector per message (:227-266, :271-304) — and of
 * batched GPU codecs generally: each blob is sent as its own frame. */
int tdt_encode_batch_into(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs,
                          uint8_t *d_out, const uint64_t *d_slot_off, uint64_t *d_out_len, int32_t *d_status,
                          void *hip_stream);
/* Decode input: blob i = in[in_off[i] .. in_off[i] + in_len[i]) when d_in_len != NULL (e.g. the
 * slots and lengths tdt_encode_batch_into produced), else in[in_off[i] .. in_off[i+1]). */
int tdt_decode_batch_into(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, const uint64_t *d_in_len,
                          uint32_t n_msgs, uint8_t *d_out, const uint64_t *d_slot_off, uint64_t *d_out_len,
                          int32_t *d_status, void *hip_stream);
/* SCATTERED batches — the slotted calls for messages that do not lie in one buffer: message i is
 * d_msgs[i][0 .. d_sizes[i]) and blob i is written at d_blobs[i] with capacity d_blob_cap[i] (encode);
 * blob i is d_blobs[i][0 .. d_blob_len[i]) and message i is written at d_outs[i] with capacity
 * d_out_cap[i] (decode).  Every array holds n_msgs entries in device memory; the calls are
 * asynchronous on hip_stream and the host reads nothing back.
 *   Same bytes: per message, the result, its length (d_out_len[i]) and its status are exactly what
 *     tdt_encode_batch_into / tdt_decode_batch_into give for the same message bytes and the same
 *     capacity, in every message class.
 *   Statuses: an output whose capacity is too small gets TDT_E_CAPACITY and length 0; an error blob
 *     gets its usual status and length 0; a blob of a generic word size (1..64 other than 1, 2, 4,
 *     8, 16) is decoded and may be mixed into any batch; a context of a generic word size encodes
 *     through the generic kernels.
 *   Addressing: the pointers may have any alignment and stand in any order (ascending, descending,
 *     shuffled).  Inputs may alias each other (the same buffer may be listed twice); outputs must
 *     not overlap each other or any input.  The pointer of a message or blob of size 0 is never
 *     dereferenced and may be null.  No byte is written outside [ptr, ptr + cap) of any output,
 *     whatever the status.
 *   Context rules: those of the slotted calls — one stream at a time per context, the side stream
 *     as there; capturable at every word size once one eager scattered call of the batch size has
 *     grown the workspace (TDT_E_CAPTURE otherwise); n_msgs == 0 returns TDT_OK and touches nothing.
 *   Mixed layouts: for gathered input into ONE slotted output buffer fill d_blobs[i] = out +
 *     slot_off[i] and d_blob_cap[i] = slot_off[i+1] - slot_off[i].
 * A batch's tiled-path threshold (1/4096 of its bytes) comes from the sum of the sizes, taken on
 * the device.  Replaces a loop of TDTCompressionProtocol::encode / decode over per-message buffers. */
int tdt_encode_batch_v(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes, uint32_t n_msgs,
                       uint8_t *const *d_blobs, const uint64_t *d_blob_cap, uint64_t *d_out_len, int32_t *d_status,
                       void *hip_stream);
int tdt_decode_batch_v(tdt_ctx *ctx, const uint8_t *const *d_blobs, const uint64_t *d_blob_len, uint32_t n_msgs,
                       uint8_t *const *d_outs, const uint64_t *d_out_cap, uint64_t *d_out_len, int32_t *d_status,
                       void *hip_stream);
/* MIXED WORD SIZES — tdt_encode_batch_v with one record width per message (a mixed-precision
 * gradient list: bf16 / fp16 tensors at width 2 beside fp32 ones at 4 and fp64 / int64 ones at 8).
 * d_word_size[i] (device memory, n_msgs entries) is message i's width; the context's own word_size
 * plays no part.  width_mask is the host's statement of the widths that may occur: bit w - 1 set
 * means "width w may occur" (the host reads no device array, so the mask is how it learns which
 * pipelines to launch).  At most TDT_MIXED_MAX_WIDTHS bits may be set: the call keeps one pair of
 * tables (32 bytes) per message and width, and launches one pipeline per width.  A zero mask (with
 * n_msgs > 0) or one with more bits returns TDT_E_ARG.
 *   Same bytes: blob i, d_out_len[i] and d_status[i] are exactly what tdt_encode_batch_v gives on a
 *     context created with word_size = d_word_size[i] and the same metrics, min_tensor_size and
 *     capacity — the UNCP routing (n % 4, n >= 64, n % word_size, the policy) and TDT_E_CAPACITY
 *     included.
 *   Rejected widths: d_word_size[i] <= 0 gives TDT_E_CONFIG, > 64 TDT_E_UNSUPPORTED, and a width in
 *     1..64 whose mask bit is clear TDT_E_ARG; each with length 0 and no byte of the output written.
 *   Everything else — addressing, aliasing, size-0 messages, one stream per context, asynchronous,
 *     nothing read back — is as for tdt_encode_batch_v.  Capturable once one eager call of the same
 *     n_msgs and mask has grown the workspaces (TDT_E_CAPTURE otherwise); n_msgs == 0 returns TDT_OK
 *     and touches nothing.  Blobs carry their width, so tdt_decode_batch_v decodes the result as it is. */
#define TDT_MIXED_MAX_WIDTHS 8
int tdt_encode_batch_vw(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes,
                        const int32_t *d_word_size, uint64_t width_mask, uint32_t n_msgs,
                        uint8_t *const *d_blobs, const uint64_t *d_blob_cap,
                        uint64_t *d_out_len, int32_t *d_status, void *hip_stream);
/* PACKED WIRE BUFFER — blobs back to back in message order with an offset table, so that one copy
 * of d_out_off[n] bytes (or one send) ships the batch; tdt_decode_batch_v reads blobs at any
 * offsets, so the receiving side needs nothing new.
 *
 * tdt_pack_v: blob i = d_blobs[i][0 .. d_blob_len[i]) -> d_out[d_out_off[i] .. d_out_off[i+1]), for
 * anyone who holds slotted or scattered blobs (the output of tdt_encode_batch_into / _v / _vw).
 * d_out_off (n_msgs + 1 entries, device memory) receives the exclusive prefix sum of the lengths,
 * the total at [n_msgs]; it is complete whatever out_cap.  The copy is split by output bytes, one
 * workgroup per 64 KiB of d_out, so one very long blob beside short ones costs what its bytes cost.
 *   Capacity: a blob with d_out_off[i+1] > out_cap gets TDT_E_CAPACITY and not one of its bytes is
 *     copied; every other blob gets TDT_OK (d_status may be NULL).  No byte is written outside
 *     d_out[0 .. min(total, out_cap)).
 *   Addressing: the sources may have any alignment and stand in any order, and may alias each
 *     other; they must not overlap d_out.  The pointer of a zero-length blob is never dereferenced.
 *   Context rules: asynchronous on hip_stream, nothing is read back, one stream at a time per
 *     context; capturable once an eager call of the same n_msgs has grown the scan's workspace
 *     (TDT_E_CAPTURE otherwise); n_msgs == 0 returns TDT_OK and touches nothing. */
int tdt_pack_v(tdt_ctx *ctx, const uint8_t *const *d_blobs, const uint64_t *d_blob_len, uint32_t n_msgs,
               uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status, void *hip_stream);
/* tdt_encode_batch_vp: tdt_encode_batch_v (d_word_size == NULL: every message at the context's
 * width, width_mask ignored) or tdt_encode_batch_vw (one width per message, width_mask as there)
 * into a packed buffer.  Two phases on the device: every message is encoded into a slot of its
 * encode bound in the context's scratch, then the blobs are packed into d_out as by tdt_pack_v.
 * total_bytes is the host's upper bound of the sum of d_sizes: it sizes the scratch, 2 * total_bytes
 * + n_msgs * (28 + 4 * wmax) bytes, wmax being the context's width or the highest mask bit (the host
 * reads no device array).  A message whose slot would end past a scratch sized by an understated
 * total_bytes gets TDT_E_CAPACITY; nothing is ever written outside the scratch.
 *   Same bytes: blob i at d_out[d_out_off[i] .. d_out_off[i+1]) and d_status[i] are exactly what
 *     tdt_encode_batch_v / _vw give for message i with a capacity of its encode bound.  A message
 *     with an error status (a rejected width, ...) has length 0 and occupies no bytes.
 *   Capacity: a blob with d_out_off[i+1] > out_cap gets TDT_E_CAPACITY (only if its status was
 *     TDT_OK) and is not copied; d_out_off[n_msgs] is the number of bytes the whole batch needs,
 *     whether or not it fit.
 *   Context rules: addressing, aliasing and size-0 messages as for tdt_encode_batch_v, mask errors
 *     at call level as for _vw; the messages must not overlap d_out.  Asynchronous, nothing read back,
 *     one stream at a time per context, n_msgs == 0 touches nothing.  Capturable at every word size
 *     once one eager call with the same n_msgs, the same mask and a total_bytes at least as large
 *     has run (TDT_E_CAPTURE otherwise) — tdt_encode_batch, the compacted call for contiguous
 *     input, is not at generic widths.
 *   Sizes first: with TDT_OPT_PACK_SIZES_FIRST set, the call instead sizes every blob (the pass of
 *     tdt_encoded_sizes_v) into d_out_off, scans it in place, and encodes every blob once, straight
 *     into d_out[d_out_off[i] .. d_out_off[i+1]) — a blob that would end past out_cap gets a slot of
 *     capacity 0.  The scratch is not used and total_bytes is ignored; every line of the contract
 *     above holds unchanged (the same bytes, the same d_out_off with the full need at [n_msgs], the
 *     same statuses, nothing written outside d_out[0 .. min(total, out_cap)), capturable once warm).
 *     With the option at 2 the size pass also keeps every message's mapping (n more words of the
 *     context's tables) and the second pass runs as the known-mapping encode (below) with them: the
 *     analysis runs once per message instead of twice.  Bytes, offsets, statuses and the capture
 *     rules are exactly those of value 1.
 * Replaces a loop of TDTCompressionProtocol::encode (:227-266) followed by a framed send of each
 * vector. */
int tdt_encode_batch_vp(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes,
                        const int32_t *d_word_size, uint64_t width_mask, uint32_t n_msgs, uint64_t total_bytes,
                        uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status,
                        void *hip_stream);
/* EXACT ENCODED SIZES — how long blob i will be, before a byte of it is written.  The size pass runs
 * the encode pipeline (the UNCP routing, the histograms, the mapping decision with its exact chains
 * on near ties, the run and 255-cap counts) and stops at the pair counts: it reads what the encode
 * reads and writes 8 bytes per message.  A caller sizes its output exactly (scan d_enc_sizes into
 * offsets) instead of by tdt_encode_bound, or decides from d_enc_sizes[i] / size[i] — the message's
 * transformation ratio — whether compressing it pays.
 *   tdt_encoded_sizes_batch: message i = d_in[d_in_off[i] .. d_in_off[i+1]), at the context's width.
 *   tdt_encoded_sizes_v: message i = d_msgs[i][0 .. d_sizes[i]).  d_word_size == NULL: every message
 *     at the context's width, width_mask ignored.  Otherwise d_word_size[i] is message i's width and
 *     width_mask, the rejected widths and the call-level mask errors are those of tdt_encode_batch_vw.
 *   Contract: d_enc_sizes[i] and d_status[i] are exactly the d_out_len[i] and d_status[i] that
 *     tdt_encode_batch_v / _vw give for the same bytes, context and metrics with a capacity of the
 *     encode bound: TDT_OK for every accepted message, a rejected width's status with size 0.
 *   Context rules: those of the scattered calls — asynchronous, nothing read back, pointers of any
 *     alignment and order, the pointer of a size-0 message never dereferenced, one stream at a time
 *     per context, n_msgs == 0 touches nothing; capturable once one eager call of the same n_msgs
 *     (and mask) has grown the workspaces (TDT_E_CAPTURE otherwise).  The calls share the encode's
 *     plan workspace, so an eager size call also warms the context for a captured encode of that
 *     batch size, and the other way round. */
int tdt_encoded_sizes_batch(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs,
                            uint64_t *d_enc_sizes, int32_t *d_status, void *hip_stream);
int tdt_encoded_sizes_v(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes,
                        const int32_t *d_word_size, uint64_t width_mask, uint32_t n_msgs,
                        uint64_t *d_enc_sizes, int32_t *d_status, void *hip_stream);
/* KNOWN MAPPINGS — the scattered encodes without the analysis.  A training process encodes the same
 * tensors step after step, and the byte-plane mapping of an fp32 or bf16 gradient does not change
 * between steps: tdt_mappings_v decides every message's mapping once (every K steps), and the mapped
 * encodes between run neither histograms nor entropies nor the decision.
 *   Mapping bits: one uint64_t per message; bit p is the stream (0 or 1) of byte position p, for
 *     p < word_size — the int32 mapping of tdt_encode_with_mapping_batch (which stays as it is) with
 *     mapping[p] at bit p.  One word per message, so a mixed-width list needs no layout of its own.
 *
 * tdt_mappings_v: tdt_encoded_sizes_v plus d_mapbits (n_msgs entries, device memory).  d_enc_sizes and
 * d_status are exactly tdt_encoded_sizes_v's; d_mapbits[i] is the mapping the encode of message i
 * decides (the margin-checked fast decision and the exact chains on near ties are the encode's own
 * lines), and 0 for a message that takes the UNCP route or whose width is rejected.  Context rules,
 * capture and the shared plan workspace as for tdt_encoded_sizes_v.
 *
 * tdt_encode_mapped_v: tdt_encode_batch_v (d_word_size == NULL: every message at the context's
 * width, width_mask ignored) or tdt_encode_batch_vw with the caller's mapping d_mapbits[i] per message.
 *   UNCP first: the UNCP routing (the policy, min_tensor_size, n % 4, n >= 64, n % word_size) is
 *     evaluated first and is unchanged; the mapping of a message that takes it is ignored.
 *   Same bytes: otherwise blob i, d_out_len[i] and d_status[i] are byte for byte what the reference
 *     gives for that message at that width with mapping[p] = (d_mapbits[i] >> p) & 1 — what
 *     tdt_encode_with_mapping_batch gives for the same bytes on a context of that width.  With
 *     d_mapbits from tdt_mappings_v over the same bytes, context and metrics the result equals
 *     tdt_encode_batch_v / _vw's in every byte, length and status.
 *   Any mapping is valid: every mapping gives a blob that decodes to the message; a stale one costs
 *     compression ratio, never correctness.
 *   Statuses: a mapping with a bit at or above word_size set gives TDT_E_BAD_MAPPING, length 0 and
 *     no byte of the output written.  TDT_E_CAPACITY, the rejected widths (TDT_E_CONFIG /
 *     TDT_E_UNSUPPORTED / TDT_E_ARG) and the call-level mask errors are those of _v / _vw; a null
 *     d_mapbits with n_msgs > 0 returns TDT_E_ARG.
 *   Everything else — addressing, aliasing, size-0 messages, one stream per context, asynchronous,
 *     nothing read back — is as for tdt_encode_batch_v.  The call plans into the encode's plan
 *     workspace, classes, side stream and count history, so an ordinary encode warms the context for
 *     a captured mapped call of that n_msgs (and mask), and the other way round (TDT_E_CAPTURE
 *     otherwise).  d_mapbits is read on the device at run time: a replayed graph encodes with
 *     whatever the array holds then.
 *
 * tdt_encode_mapped_vp: the packed contract of tdt_encode_batch_vp over those blobs; a
 * TDT_E_BAD_MAPPING message occupies no bytes.  It always takes the two phases, whatever
 * TDT_OPT_PACK_SIZES_FIRST says: the sizes-first form would need the sizes under the caller's mapping,
 * and the size pass decides its mapping itself. */
int tdt_mappings_v(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes,
                   const int32_t *d_word_size, uint64_t width_mask, uint32_t n_msgs,
                   uint64_t *d_enc_sizes, uint64_t *d_mapbits, int32_t *d_status, void *hip_stream);
int tdt_encode_mapped_v(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes,
                        const int32_t *d_word_size, uint64_t width_mask, uint32_t n_msgs,
                        const uint64_t *d_mapbits, uint8_t *const *d_blobs, const uint64_t *d_blob_cap,
                        uint64_t *d_out_len, int32_t *d_status, void *hip_stream);
int tdt_encode_mapped_vp(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes,
                         const int32_t *d_word_size, uint64_t width_mask, uint32_t n_msgs,
                         uint64_t total_bytes, const uint64_t *d_mapbits, uint8_t *d_out, uint64_t out_cap,
                         uint64_t *d_out_off, int32_t *d_status, void *hip_stream);
/* Decoded size of each scattered blob (0 with an error status), as tdt_decoded_sizes_batch. */
int tdt_decoded_sizes_v(tdt_ctx *ctx, const uint8_t *const *d_blobs, const uint64_t *d_blob_len, uint32_t n_msgs,
                        uint64_t *d_sizes, int32_t *d_status, void *hip_stream);
/* d_slot_off (n+1 entries) = exclusive prefix sum of tdt_ctx_encode_bound(size_i): of
 * tdt_encode_bound(size_i, word_size), or of size_i + 4 with TDT_OPT_RAW_FALLBACK. */
int tdt_encode_slots(tdt_ctx *ctx, const uint64_t *d_in_off, uint32_t n_msgs, uint64_t *d_slot_off,
                     void *hip_stream);
/* d_slot_off (n+1 entries) = exclusive prefix sum of the decoded sizes (header parse). */
int tdt_decode_slots(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, const uint64_t *d_in_len,
                     uint32_t n_msgs, uint64_t *d_slot_off, int32_t *d_status, void *hip_stream);

/* Decoded size of each blob (0 for blobs with an error status). */
int tdt_decoded_sizes_batch(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off,
                            uint32_t n_msgs, uint64_t *d_sizes, int32_t *d_status, void *hip_stream);

/* Full-sample analysis of each message (n must be a non-zero multiple of word_size):
 * d_hist n*ws*256 uint32, d_entropy n*ws double, d_mapping n*ws int32 (any may be NULL). */
int tdt_analyze_batch(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs,
                      uint32_t *d_hist, double *d_entropy, int32_t *d_mapping, int32_t *d_status,
                      void *hip_stream);

/* Host-memory path (the TCP socket-buffer case).  The batch runs as chunks (an eighth of the
 * call's input, 2-64 MiB) through four pipeline slots (device buffers) on two streams, one for
 * the input DMAs and one for the kernels and the output: H2D, kernel and D2H of neighbouring
 * chunks overlap.  Pinned caller buffers are DMA'd
 * directly; pageable ones (std::vector, numpy) are staged through the context's pinned buffers
 * by a pool of host threads (TDT_OPT_COPY_THREADS).  h_out must hold the sum of
 * tdt_encode_bound (encode) or of the decoded sizes (decode); h_out_off receives n+1 offsets.
 * Blocks the calling thread until the results are in h_out. */
int tdt_encode_host(tdt_ctx *ctx, const uint8_t *h_in, const uint64_t *h_in_off, uint32_t n_msgs,
                    uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_off, int32_t *h_status);
int tdt_decode_host(tdt_ctx *ctx, const uint8_t *h_in, const uint64_t *h_in_off, uint32_t n_msgs,
                    uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_off, int32_t *h_status);
/* tdt_encode_host over n messages that are NOT contiguous (message i = msgs[i][0 .. sizes[i])),
 * as a substrate's send path holds them (one buffer per message, transport_send(void*, size_t),
 * tcp_simple.hpp:68-91): the pool copies them straight into the pinned staging, no packing
 * copy.  Replaces a loop of TDTCompressionProtocol::encode (tdt_compression.hpp:227-266). */
int tdt_encode_host_v(tdt_ctx *ctx, const uint8_t *const *msgs, const uint64_t *sizes, uint32_t n_msgs,
                      uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_off, int32_t *h_status);
/* Pinned (page-locked, device-mapped) host memory for callers that keep their socket buffers in
 * it: the host paths DMA such buffers directly instead of staging them.  Returns TDT_OK. */
int tdt_host_alloc(uint64_t bytes, void **ptr);
void tdt_host_free(void *ptr);
/* dst[0, bytes) = src[0, bytes) on the context's staging-copy threads (a parallel memcpy: one
 * thread's copy is below what a socket pipeline needs).  Host memory only. */
int tdt_host_copy(tdt_ctx *ctx, void *dst, const void *src, uint64_t bytes);
/* d_dst[0, bytes) = d_src[0, bytes) between device buffers, asynchronously on hip_stream (NULL:
 * the null stream), by the codec's hand-written HBM copy: one 512-lane workgroup per 64 KiB piece,
 * every load of the piece in flight before its non-temporal stores — the access shape of the
 * resident encode / decode, and the best hand-written copy measured on MI355X (tools/ubench_hbm.hip:
 * 5.6-5.8 TB/s read + write).  bench.py times it as roofline.copy_ceiling.  Any sizes and
 * alignments; the buffers must not overlap. */
int tdt_copy_device(void *d_dst, const void *d_src, uint64_t bytes, void *hip_stream);

/* Device-side invariant flags: bit0 look-back timeout, bit1 staging-index guard, bit2
 * flush-bound guard.  Always 0 for a correct build; the guards turn a logic error into a flag
 * instead of a wild write.  Reads the flag word in stream order on `hip_stream` (the stream
 * the context's batches were issued on) and synchronises that stream only.  Scope: the most
 * recent compacted (look-back) batch on the context's workspace, OR-ed with every slotted
 * batch since then (slotted calls do not clear the word) and with every host-pipeline chunk
 * since the context was created (sticky). */
int tdt_ctx_error_flags(tdt_ctx *ctx, void *hip_stream, uint32_t *flags);

/* Tuning / diagnostic options (tdt_ctx_create reads the same from the environment once:
 * PSYNE_TDT_LARGE_MIN, PSYNE_TDT_TILE_CAP, PSYNE_TDT_NO_SIDE, PSYNE_TDT_SMALL_MAIN,
 * PSYNE_TDT_NO_TWO_PHASE, PSYNE_TDT_COPY_THREADS, PSYNE_TDT_ANY_TILED, PSYNE_TDT_ANY_DEC_TILED,
 * PSYNE_TDT_RAW_FALLBACK, PSYNE_TDT_HOST_RAW_FALLBACK).  Not needed for correct results: every setting
 * encodes and decodes the same bytes — except TDT_OPT_RAW_FALLBACK and TDT_OPT_HOST_RAW_FALLBACK, which
 * change which blob an expanding message gets. */
#define TDT_OPT_LARGE_MIN 1               /* messages above this many bytes take the tiled path (every word size:
                                             the tuned widths' tiles and the generic widths' alike) */
#define TDT_OPT_TILE_CAP 2                /* lower tile budget per batch (tests of the fallback; every word size) */
#define TDT_OPT_NO_SIDE_STREAM 3          /* 1: the tile pipeline runs on the caller's stream */
#define TDT_OPT_SMALL_ON_CALLER_STREAM 4  /* 1: small-message lists stay on the caller's stream */
#define TDT_OPT_NO_TWO_PHASE 5            /* 1: compacted calls always take the one-pass kernels */
#define TDT_OPT_COPY_THREADS 6            /* host threads staging pageable buffers (default <= 16) */
#define TDT_OPT_PACK_SIZES_FIRST 7        /* 1: tdt_encode_batch_vp sizes the blobs first and encodes them in
                                             place, without the scratch (default 0: the two phases);
                                             2: as 1, and the second pass reuses the mappings the size
                                             pass decided (the known-mapping encode) */
#define TDT_OPT_ANY_TILED 8               /* word sizes other than 1, 2, 4, 8, 16: messages above the tiled-path
                                             threshold (max(TDT_OPT_LARGE_MIN, 1/4096 of the batch's bytes))
                                             are encoded as 64 KiB tiles over the whole device (default 1);
                                             0: every such message on one workgroup.  The A/B switch: the
                                             same bytes, lengths and statuses either way */
#define TDT_OPT_ANY_DEC_TILED 9           /* word sizes other than 1, 2, 4, 8, 16: blobs that decode to more than
                                             the tiled-path threshold (max(TDT_OPT_LARGE_MIN, 1/4096 of the
                                             batch's blob bytes)), with one or two referenced streams, are
                                             decoded as 32 KiB output tiles over the whole device (default 1);
                                             0: every such blob on one workgroup.  The A/B switch: the same
                                             bytes, lengths and statuses either way */
/* RAW FALLBACK.  TDT never falls back to the raw bytes by itself: a message that does not compress
 * (a dense fp32 gradient, random bytes) leaves as a TDT blob of up to 28 + 4*ws + 2n bytes.  With this
 * option at 1 (default 0: every call launches and writes exactly what it does without the option) the
 * device-batch encodes store such a message as its UNCP blob, which every decoder reads already.
 *   Rule: take a message that goes down the TDT route — the UNCP routing (the policy, min_tensor_size,
 *     n % 4, n >= 64, n % word_size) did not take it, and its status would be TDT_OK given enough room —
 *     and let E be its TDT blob length (under the caller's mapping in the mapped calls).  If E > n + 4
 *     the output is exactly the UNCP blob: the marker, then the n message bytes; length n + 4, status
 *     TDT_OK.  If E <= n + 4 (the tie included) the blob stays TDT, byte for byte as without the option.
 *   Capacity: a message is written, as TDT or as UNCP, if and only if min(E, n + 4) <= capacity;
 *     otherwise TDT_E_CAPACITY and length 0.  A slot of n + 4 bytes always suffices.  No byte outside
 *     [ptr, ptr + cap) is written whatever the status; bytes of a slot beyond the final blob may hold
 *     anything, as without the option.
 *   Other statuses: rejected widths, TDT_E_BAD_MAPPING, size-0 messages and messages that took UNCP
 *     by the routing are untouched.
 *   Where: tdt_encode_batch_into, tdt_encode_batch_v / _vw, tdt_encode_batch_vp (two phases and
 *     TDT_OPT_PACK_SIZES_FIRST 1 and 2), tdt_encode_mapped_v / _vp; tdt_encoded_sizes_batch / _v and
 *     tdt_mappings_v report min(E, n + 4) — d_mapbits[i] stays the mapping the analysis decided, also
 *     for a message that falls back, so mappings of the same bytes still give the same blobs.
 *     tdt_encode_batch takes its two-phase form (slots of n + 4, scan, gather), and so returns
 *     TDT_E_UNSUPPORTED under stream capture or TDT_OPT_NO_TWO_PHASE, as it does at generic widths.
 *     Every word size, every message class, TDT_OPT_ANY_TILED 0 and 1.
 *   Bounds: tdt_ctx_encode_bound gives n + 4, tdt_encode_slots sums it, and the packed two-phase
 *     scratch of tdt_encode_batch_vp is total_bytes + 4 * n_msgs.  tdt_encode_bound does not change.
 *   Device rules: nothing is read back, calls are asynchronous on the caller's stream and capturable
 *     once one eager call of the same n_msgs (and mask) has grown the workspaces (TDT_E_CAPTURE
 *     otherwise); n_msgs == 0 touches nothing.  d_out_len and d_status may be NULL as before.
 *   Calls that ignore the option: tdt_encode_with_mapping_batch (the parity hook, which no option
 *     changes), and the host calls tdt_encode_host / tdt_encode_host_v with the one-message path behind
 *     HipTDTCompressionProtocol and TdtSubstrate — those have an option of their own, next. */
#define TDT_OPT_RAW_FALLBACK 10
/* RAW FALLBACK ON THE HOST PATH.  The same rule for tdt_encode_host and tdt_encode_host_v (pageable and
 * pinned buffers, every word size, one message or many), and through them HipTDTCompressionProtocol::
 * encode and TdtSubstrate::send / send_batch.  Default 0: every host call launches and writes exactly what
 * it does without the option; independent of TDT_OPT_RAW_FALLBACK (PSYNE_TDT_HOST_RAW_FALLBACK).
 *   Rule: as above — a message that goes down the TDT route and whose TDT blob length E exceeds n + 4
 *     comes out as the marker and the n message bytes, length n + 4, status TDT_OK; E <= n + 4 (the tie
 *     included) stays TDT byte for byte; messages the UNCP routing takes and size-0 messages are untouched.
 *   Bound: tdt_ctx_host_encode_bound(ctx, n) is n + 4; h_out_off stays the exclusive prefix of the final
 *     lengths, and the call returns TDT_E_CAPACITY only if their sum exceeds out_cap.  Nothing is
 *     written past h_out + out_cap.
 *   How: every chunk of the pipeline takes the slotted route with slots of n + 4 bytes; behind the
 *     chunk's encode a flag pass decides, and the chunk's gather to host memory takes a flagged blob
 *     straight from the chunk's input — a fallen-back message is never written on the device.  A
 *     one-message call stores the raw bytes on the host, with no second launch.
 *   TDT_STAT_HOST_RAW_FALLBACKS counts the messages of the most recent host encode call. */
#define TDT_OPT_HOST_RAW_FALLBACK 11
int tdt_ctx_set_option(tdt_ctx *ctx, int option, uint64_t value);

/* Read-only counters of the context (tests and tools: which path a call took).  The claims are those
 * of the most recent call that ran the generic-width decode's plan and whose snapshot has landed — valid
 * after the device (or the call's stream) has been synchronised; claims are counted beyond the budgets
 * too, so a claim above its budget means that some blob fell back to one workgroup.  Until a call of
 * the context has met a blob of such a width no plan runs (the call after the first such one is the
 * first to be tiled); those calls leave the claims unchanged, as do the host pipeline's.  Returns TDT_E_ARG for an unknown `stat`. */
#define TDT_STAT_ANY_DEC_LARGE 1          /* long generic-width blobs the decode plan claimed records for */
#define TDT_STAT_ANY_DEC_BLOCKS 2         /* 2,048-pair block sums it claimed */
#define TDT_STAT_ANY_DEC_TILES 3          /* 32 KiB output tiles it claimed */
#define TDT_STAT_ANY_DEC_BUDGET_LARGE 4   /* the current budgets: long-blob records ... */
#define TDT_STAT_ANY_DEC_BUDGET_TILES 5   /* ... and tiles (before TDT_OPT_TILE_CAP) */
#define TDT_STAT_RAW_FALLBACKS 6          /* messages the most recent device-batch encode whose snapshot has landed
                                             stored raw by TDT_OPT_RAW_FALLBACK's rule (0 after an encode with the
                                             option off; the size calls and captured replays leave it as it is) */
#define TDT_STAT_PACK_SCRATCH_BYTES 7     /* bytes of the context's scratch (the slots of the two-phase
                                             tdt_encode_batch_vp and of the two-phase compacted encode): sized
                                             exactly by the largest such call so far, 2 * total_bytes + n_msgs *
                                             (28 + 4 * wmax) — total_bytes + 4 * n_msgs with TDT_OPT_RAW_FALLBACK */
#define TDT_STAT_HOST_RAW_FALLBACKS 8     /* messages the most recent host encode call of the context (tdt_encode_host
                                             / _v) stored raw by TDT_OPT_HOST_RAW_FALLBACK's rule.  Host calls block, so
                                             the value is final when the call returns; 0 after a call with the option off */
int tdt_ctx_get_stat(tdt_ctx *ctx, int stat, uint64_t *value);

/* Host-memory analyze (analyze_data :206-222): h_entropy n*ws doubles, h_mapping n*ws int32
 * (either may be NULL).  Blocks the calling thread. */
int tdt_analyze_host(tdt_ctx *ctx, const uint8_t *h_in, const uint64_t *h_in_off, uint32_t n_msgs,
                     double *h_entropy, int32_t *h_mapping, int32_t *h_status);

/* Text of the last error on this thread ("" if none). */
const char *tdt_last_error(void);
/* Human-readable status name; for TDT_E_SHORT / TDT_E_MAGIC the reference's exception text. */
const char *tdt_status_string(int status);

#ifdef __cplusplus
}
#endif
#endif
