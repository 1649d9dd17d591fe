// tdt_api.hip — C ABI (include/psyne_tdt.h) over the gfx950 TDT kernels.
//
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC (psyne_amd/build.py).
// The library never falls back to a CPU path: every entry point launches a HIP kernel or
// fails with TDT_E_HIP.
#include "../../include/psyne_tdt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <sched.h>
#include <string>
#include <type_traits>
#include <vector>

#include "tdt_anyws.h"
#include "tdt_copy.h"
#include "tdt_copypool.h"
#include "tdt_decode.h"
#include "tdt_encode.h"
#include "tdt_enc_lmap.h"
#include "tdt_grow.h"
#include "tdt_pack.h"
#include "tdt_plan.h"
#include "tdt_rawfb.h"
#include "tdt_slots.h"

// The encode kernels live in tdt_enc_ws.hip (one translation unit per word size); diagnostic
// builds (word size 4 only, phase profiling) instantiate them here instead.
#if !defined(PSY_FAST_BUILD) && !(defined(PSY_PROF) && PSY_PROF) && !defined(PSY_SINGLE_TU)
#define PSY_ENC_EXT(WS, T, G, M, L, TL, PS, PA) \
    extern template __global__ void psy::tdt_encode_kernel<WS, T, G, psy::M, L, TL, PS, PA>(psy::EncodeArgs);
#define PSY_ENC_PAIR_EXT(WS, T, G, TL, PS, PA) \
    extern template __global__ void psy::tdt_encode_kernel<WS, T, G, psy::MODE_ENCODE, 0, TL, PS, PA, true>(psy::EncodeArgs);
#define PSY_ENC_EXT_WS(WS)                                                                                          \
    PSY_ENC_INSTANCES(PSY_ENC_EXT, WS)                                                                              \
    extern template __global__ void psy::tdt_encode_lscan_kernel<WS>(psy::EncodeArgs, const uint32_t *, uint32_t);  \
    PSY_ENC_PAIR_INSTANCES(PSY_ENC_PAIR_EXT, WS)                                                                    \
    extern template __global__ void psy::tdt_encode_lscan_kernel<WS, true>(psy::EncodeArgs, const uint32_t *, uint32_t); \
    PSY_ENC_SIZES_INSTANCES(PSY_ENC_SIZES_EXT, WS)                                                                   \
    extern template __global__ void psy::tdt_encode_lscan_sizes_kernel<WS>(psy::EncodeArgs, const uint32_t *, uint32_t); \
    PSY_ENC_MAPPED_INSTANCES(PSY_ENC_MAPPED_EXT, WS)
// (the known-mapping scattered encode, MODE_MAPPED with PAIR: tdt_enc_mapped_ws.hip)
#define PSY_ENC_MAPPED_EXT(WS, T, G, TL, PS, PA) \
    extern template __global__ void psy::tdt_encode_kernel<WS, T, G, psy::MODE_MAPPED, 0, TL, PS, PA, true>(psy::EncodeArgs);
// (the size pass, MODE_SIZES: tdt_enc_sizes_ws.hip)
#define PSY_ENC_SIZES_EXT(WS, T, G, TL, PS, PA) \
    extern template __global__ void psy::tdt_encode_kernel<WS, T, G, psy::MODE_SIZES, 0, TL, PS, PA, true>(psy::EncodeArgs);
PSY_ENC_EXT_WS(1)
PSY_ENC_EXT_WS(2)
PSY_ENC_EXT_WS(4)
PSY_ENC_EXT_WS(8)
PSY_ENC_EXT_WS(16)
#endif

// The generic-word-size kernels live in tdt_anyws.hip; the diagnostic single-file builds leave
// them out (word sizes other than 1, 2, 4, 8, 16 are then unsupported, as blobs carrying one).
#if !defined(PSY_FAST_BUILD) && !(defined(PSY_PROF) && PSY_PROF) && !defined(PSY_SINGLE_TU)
#define PSY_HAVE_ANYWS 1
#else
#define PSY_HAVE_ANYWS 0
#endif

namespace {

thread_local std::string g_err;

int set_err(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return set_err(TDT_E_HIP, std::string(#expr ": ") + hipGetErrorString(e_));    \
    } while (0)

bool capturing(hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}
// A workspace must grow: not possible while the stream is being captured (the allocator and
// the implicit synchronisation of a free are not capturable) — warm the context with one eager
// call of the batch first.
int no_growth_in_capture(hipStream_t s) {
    if (!capturing(s)) return TDT_OK;
    return set_err(TDT_E_CAPTURE, "workspace too small for this batch under stream capture: issue one eager call "
                                  "of the same batch size on this context before capturing");
}

// The grower's callables (psy::grow, tdt_grow.h).  Allocation: `unit` bytes per counted element.
int hip_status(hipError_t e, const char *what) {
    return e == hipSuccess ? TDT_OK : set_err(TDT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
struct DevAlloc {
    size_t unit = 1;
    template <class T>
    int operator()(T **p, size_t cap) const { return hip_status(hipMalloc(p, unit * cap), "hipMalloc"); }
};
struct PinAlloc {
    size_t unit = 1;
    unsigned flags = hipHostMallocDefault;
    template <class T>
    int operator()(T **p, size_t cap) const { return hip_status(hipHostMalloc(p, unit * cap, flags), "hipHostMalloc"); }
};
// Dropping the old buffer: freed (the device waits for everything queued), or retired to a list its
// owner frees with itself — a graph captured earlier, or calls still queued, may point at it.
int dev_free(void *p) { return hip_status(hipFree(p), "hipFree"); }
int pin_free(void *p) { return hip_status(hipHostFree(p), "hipHostFree"); }
auto retire_to(std::vector<void *> &list) {
    return [&list](void *p) { return list.push_back(p), TDT_OK; };
}
// A device buffer that a graph captured on the context may point at: it does not grow under
// capture (no_growth_in_capture), and the buffer it replaces is retired
template <class T, class S>
int grow_retiring(T *&p, S &have, size_t need, size_t cap, std::vector<void *> &retired, hipStream_t s, size_t unit = 1) {
    if (need <= have) return TDT_OK;
    if (int st = no_growth_in_capture(s)) return st;
    return psy::grow(p, have, need, cap, retire_to(retired), DevAlloc{unit});
}

}  // namespace

// Counts of an earlier plan (the slotted calls size their main grids from them; no call ever
// waits for them).  Each call's plan counters are copied into pinned memory behind the plan
// kernel; a later call takes them once that copy has completed.  K: the direction's counter names.
template <class K>
struct CountHist {
    uint32_t *pin = nullptr;  // pinned: the snapshotted part of the plan's counter block
    hipEvent_t ev = nullptr;
    bool pending = false, valid = false;
    uint32_t v[psy::kPlanSnapBytes / 4] = {};
    uint32_t n = 0, n_pending = 0;  // messages in the snapshot's batch
    uint32_t operator[](K k) const { return v[psy::lo32(k)]; }
    // fold the newest completed snapshot in (never waits)
    void refresh() {
        if (pending && hipEventQuery(ev) == hipSuccess) {
            std::memcpy(v, pin, sizeof(v));
            n = n_pending;
            valid = true;
            pending = false;
        }
    }
    void release() {
        if (ev) (void)hipEventDestroy(ev);
        if (pin) (void)hipHostFree(pin);
        ev = nullptr;
        pin = nullptr;
        pending = valid = false;
    }
};

// Workspace of the slotted calls' plan (message classes / large-message state).  One per
// stream user: the context's own, and one per host-pipeline slot (those run concurrently).
struct PlanWS {
    uint8_t *buf = nullptr;  // counters | lists (grows with the batch)
    size_t bytes = 0;
    // large-message state, allocated at a small budget and grown (to the counts a plan reported)
    // when a batch had more large messages than the budget held
    uint8_t *elarge = nullptr;  // encode: LMeta | tile entries | tile records | span entries | span bins
    uint32_t e_lcap = 0, e_tcap = 0;
    uint8_t *dlarge = nullptr;  // decode: DMeta | block entries | block sums | tile entries | tile blocks
    uint32_t d_lcap = 0, d_bcap = 0, d_tcap = 0;
    CountHist<psy::EncCount> eh;  // encode / decode plan counts
    CountHist<psy::DecCount> dh;
    // buffers replaced by a larger one: a graph captured on the context before the growth may
    // still point at them, so they are freed only with the workspace
    std::vector<void *> retired;
    // the large-message pipeline runs on `side` beside the medium/small lists (fork/join events)
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    // host-pipeline slots run without the side stream: their chunks already overlap one another,
    // and every extra stream shares HIP's few hardware queues with the other slots (and with the
    // other end's context in a one-process loopback: C1's encode 6.2 -> 4.0 ms per 50 MiB call)
    bool no_side = false;
    void release() {
        if (join) (void)hipEventDestroy(join);
        if (fork) (void)hipEventDestroy(fork);
        if (side) (void)hipStreamDestroy(side);
        side = nullptr;
        fork = join = nullptr;
        if (buf) (void)hipFree(buf);
        if (elarge) (void)hipFree(elarge);
        if (dlarge) (void)hipFree(dlarge);
        for (void *p : retired) (void)hipFree(p);
        retired.clear();
        buf = elarge = dlarge = nullptr;
        e_lcap = e_tcap = d_lcap = d_bcap = d_tcap = 0;
        eh.release();
        dh.release();
        bytes = 0;
    }
};

// Workspace of the tiled generic-width encode (tdt_anyws.h), one per context: the calls that use it
// hold the context's lock.  Budgets as the slotted plan's: a starting budget, the claimed counts in
// the counter block, the pinned snapshot, growth on a later call with the old buffer retired.
struct AnyTiledWS {
    uint8_t *buf = nullptr;  // counters (kPlanCounterBytes) | one mark word per message
    size_t bytes = 0;
    uint8_t *rec = nullptr;  // AnyLarge records | AnyTile records | histograms
    size_t rec_bytes = 0;
    uint32_t lcap = 0, tcap = 0;
    CountHist<psy::AnyCount> h;
    void release() {
        if (buf) (void)hipFree(buf);
        if (rec) (void)hipFree(rec);
        buf = rec = nullptr;
        bytes = rec_bytes = 0;
        lcap = tcap = 0;
        h.release();
    }
};

// Workspace of the tiled generic-width decode (tdt_anyws.h), one per context, as AnyTiledWS: the
// calls that use it hold the context's lock.
struct AnyDecWS {
    uint8_t *buf = nullptr;  // counters (kPlanCounterBytes) | one mark word per entry of the deferred list
    size_t bytes = 0;
    uint8_t *rec = nullptr;  // AnyDecLarge records | block sums
    size_t rec_bytes = 0;
    uint32_t lcap = 0, bcap = 0, tcap = 0;  // (tiles need no records: their budget bounds the launch)
    CountHist<psy::AnyDecCount> h;
    // pinned: the length of the last deferred list that was not empty (0: every list so far was empty),
    // written by tdt_decode_any_kernel.  A hint only, read without waiting: while it is 0 (a context that
    // has decoded tuned widths only) a call launches neither the plan nor the snapshot; from the first
    // listed blob on, every call of the context runs the plan.
    uint32_t *seen = nullptr;
    void release() {
        if (buf) (void)hipFree(buf);
        if (rec) (void)hipFree(rec);
        if (seen) (void)hipHostFree(seen);
        buf = rec = nullptr;
        seen = nullptr;
        bytes = rec_bytes = 0;
        lcap = bcap = tcap = 0;
        h.release();
    }
};

// host pipeline slots (chunks in flight per tdt_encode_host / tdt_decode_host call)
constexpr int kHostSlots = 4;

struct tdt_ctx {
    int device = 0;
    tdt_config cfg{};
    std::atomic<double> bandwidth{100.0};  // reference defaults :352-354
    std::atomic<double> latency{1.0};
    std::atomic<double> cpu{0.5};
    std::atomic<uint64_t> size_hint{65536};
    std::mutex mu;
    // workspace: [0..64) counters (ticket, timeout), then one u64 look-back word per message
    uint8_t *ws = nullptr;
    // device buffers a captured graph may still reference after a growth (ws, slot_sums): freed
    // at tdt_ctx_destroy, never while the context lives
    std::vector<void *> retired;
    std::vector<void *> retired_host;  // pinned host-pipeline buffers replaced by larger ones
    size_t ws_bytes = 0;
    // per-chunk sums of tdt_decode_slots' two-pass scan (one u64 per 8192 messages; stream-ordered
    // like `ws`: one slotted decode per context at a time)
    uint64_t *slot_sums = nullptr;
    uint32_t slot_sums_n = 0;
    // host-path device buffers and stream (tdt_analyze_host)
    uint8_t *h_dev = nullptr;
    size_t h_dev_bytes = 0;
    hipStream_t astream = nullptr;
    // host pipeline (tdt_encode_host / tdt_decode_host): kHostSlots slots, each with its own stream,
    // device buffer (input, offsets, output, status, look-back workspace) and pinned offsets
    struct HostSlot {
        hipStream_t stream = nullptr;
        hipEvent_t ev = nullptr;
        uint8_t *dev = nullptr;
        size_t dev_bytes = 0;
        uint64_t *pin = nullptr;  // pinned: in_off (n+1) | slots (n+1) | out_off or lengths (n+1) | status (n int32)
        size_t pin_words = 0;
        uint32_t *flag = nullptr;  // pinned: the last chunk's device error flags
        uint8_t *stage_in = nullptr, *stage_out = nullptr;  // pinned staging for pageable callers
        size_t sin_bytes = 0, sout_bytes = 0;
        hipEvent_t evc = nullptr;  // after the chunk's output copy (orders the next chunk's)
        hipEvent_t evi = nullptr;  // after the chunk's input copy (orders the next chunk's)
        PlanWS pw;
    } hs[kHostSlots];
    // the host pipeline's two streams (chunk buffers stay per slot): every input copy on `hin`, in
    // chunk order; every kernel and read-back on `hex`.  Per-slot streams (PSYNE_TDT_SLOT_STREAMS=1,
    // round 4) outnumber the HIP runtime's default 4 hardware queues together with the caller's
    // streams: streams sharing a queue serialised the chunks (profiles/r05_diag/host_decode/)
    hipStream_t hin = nullptr, hex = nullptr;
    bool slot_streams = false;
    // one-message fast path (tdt_encode_host / tdt_decode_host with one message of at most
    // kOneMax bytes: the per-call Protocol::encode / decode of the drop-in class): a mapped pinned
    // block holding the call's offsets, list, status, input and output, read and written by ONE
    // class kernel in place (zero-copy), so a call is two host memcpys, one launch and one sync
    uint8_t *one = nullptr;
    size_t one_bytes = 0;
    hipStream_t one_stream = nullptr;
    std::shared_ptr<CopyPool> pool;  // host threads of the staging copies (shared: tdt_host_copy)
    uint64_t *hbases = nullptr;      // host_encode: device-side running output base per chunk
    size_t hbases_n = 0;
    int copy_threads = 8;
    std::mutex hmu;
    // error flags of the host pipeline's chunks, OR-ed since the context was created
    std::atomic<uint32_t> host_flags{0};
    PlanWS pw;                        // the slotted calls' plan workspace
    // mixed-width scattered encode (tdt_encode_batch_vw): a plan workspace and count history per
    // tuned width (1, 2, 4, 8, 16 by log2; created on first use, `pw` is never touched), and the
    // pair tables of every width of the call (psy::mixed_routes)
    std::unique_ptr<PlanWS> mx_pw[5];
    uint8_t *mx_tab = nullptr;
    size_t mx_bytes = 0;
    // two-phase compacted encode (batches with messages > 64 KiB): slotted blobs, their slots
    // and lengths, then a scan and a gather into the caller's compacted buffer
    uint8_t *cp_buf = nullptr;
    size_t cp_bytes = 0;
    uint64_t *cp_idx = nullptr;  // slots (n + 1) | lengths (n) | flag
    size_t cp_idx_n = 0;
    // packed scattered encode (tdt_encode_batch_vp) keeps its slots in cp_buf and its tables in
    // cp_idx: slots (n + 1) | blob addresses (n) | capacities (n) | lengths (n) — or, sizes first, no
    // slots at all and blob addresses (n) | capacities (n).  That call may be
    // captured, so from its first capture on a buffer replaced by a larger one is retired, not freed
    bool cp_in_graph = false;
    // TDT_OPT_PACK_SIZES_FIRST: tdt_encode_batch_vp sizes the blobs first (the size pass), scans, and
    // encodes straight into the caller's buffer — cp_buf is not used, cp_idx holds addresses (n) | capacities (n).
    // 2: the size pass also exports every message's mapping bits (cp_idx: n more u64) and the second
    // pass runs as the known-mapping encode with them — no histogram, no entropies, no decision again
    int pack_sizes_first = 0;
    // the pack kernel's knobs (PSYNE_TDT_PACK_CUT, PSYNE_TDT_PACK_GRID: tools/pack_bench.py)
    uint32_t pack_cut = psy::kPackCut, pack_grid = psy::kPackGridCap;
    uint64_t large_min = 256 * 1024;  // messages (decode: decoded blobs) above this take the tiled path
    uint32_t tile_cap = ~0u;          // lower tile budget (tests)
    // TDT_OPT_ANY_TILED (PSYNE_TDT_ANY_TILED): generic-width messages above the threshold take the tile
    // pipeline; off: every one of them on the one-workgroup kernel
    bool any_tiled = true;
    AnyTiledWS anyw;
    // TDT_OPT_ANY_DEC_TILED (PSYNE_TDT_ANY_DEC_TILED): generic-width blobs that decode to more than the
    // threshold take the decode tile pipeline; off: every one of them on the one-workgroup kernel
    bool any_dec_tiled = true;
    AnyDecWS anydw;
    // diagnostic knobs (read once at tdt_ctx_create from the environment, or tdt_ctx_set_option)
    bool no_side = false;       // PSYNE_TDT_NO_SIDE: no side stream for the tile pipeline
    bool small_main = false;    // PSYNE_TDT_SMALL_MAIN: small lists on the caller's stream
    bool no_two_phase = false;  // PSYNE_TDT_NO_TWO_PHASE: compacted calls take the one-pass kernels
    bool no_one = false;        // PSYNE_TDT_NO_ONE: one-message host calls take the pipeline too
    bool one_wave = false;      // PSYNE_TDT_ONE_WAVE=1: one-message decode as one wave (round-4 path)
    uint64_t one_wave_max = 4096;  // one-message decode: outputs up to this size take the one-wave kernel
    bool dout_sdma = false;     // PSYNE_TDT_DOUT_SDMA=1: host_decode's output by hipMemcpyAsync (round 4)
    bool one_spin = true;       // PSYNE_TDT_ONE_SPIN=0: one-message calls wait in hipStreamSynchronize
    uint32_t one_seq = 0;
    uint32_t copy_wgs = 8;      // PSYNE_TDT_COPY_WGS: copy-list workgroups per CU
    // PSYNE_TDT_DSMALL_MAX: blobs decoding to at most this many bytes take the one-round-window
    // list on the side stream (C4 decode 11.80 -> 11.42 ms at 8 KiB against 1 KiB; 16-64 KiB
    // gave 11.6-11.8, profiles/r03_dsm2/ab.txt)
    uint64_t dsmall_max = 8192;
    uint64_t dbig_min = 128 * 1024;  // PSYNE_TDT_DBIG_MIN: one-wave blobs above this are dispatched first
    int cus = 256;              // compute units (overflow grids)
    // TDT_OPT_RAW_FALLBACK (PSYNE_TDT_RAW_FALLBACK): the device-batch encodes store a message whose TDT
    // blob would exceed n + 4 bytes as its UNCP blob (tdt_rawfb.h).  Its workspace, rf_buf: counters
    // (kPlanCounterBytes) | clamped capacities (n) | raw lengths, scanned (n + 1) | lengths (n, where the
    // caller gave none) | a contiguous batch's tables (4n) | statuses (n int32, where the caller gave none)
    bool raw_fallback = false;
    uint8_t *rf_buf = nullptr;
    size_t rf_bytes = 0;
    CountHist<psy::RawCount> rf_h;          // TDT_STAT_RAW_FALLBACKS: the flagged messages of a call
    std::atomic<bool> rf_last_on{false};    // the most recent device-batch encode ran under the option
    // TDT_OPT_HOST_RAW_FALLBACK (PSYNE_TDT_HOST_RAW_FALLBACK): the same rule for the host calls
    // (host_encode, host_one).  Independent of the option above; its flag words live in each chunk's own
    // device layout (Chunk), since up to kHostSlots chunks are in flight.
    bool host_raw_fallback = false;
    std::atomic<uint64_t> host_rf_count{0};  // TDT_STAT_HOST_RAW_FALLBACKS: of the most recent host encode call
};

namespace {

constexpr size_t kCounterBytes = 64;

// workspace: counters | one look-back word per message (+ 1) | the deferred-blob list of the
// compacted decode (one u32 per message, tdt_anyws.h)
int ensure_ws(tdt_ctx *c, uint32_t n_msgs, hipStream_t s) {
    const size_t need = kCounterBytes + 8ull * (n_msgs + 1) + 4ull * n_msgs;
    return grow_retiring(c->ws, c->ws_bytes, need, psy::cap_double(need, c->ws_bytes), c->retired, s);
}

bool ws_supported(int ws) { return psy::anyws_tuned(ws) || (PSY_HAVE_ANYWS && psy::anyws_generic(ws)); }

// the generic encode kernel (any word size in 1..64 the tuned kernels do not cover)
// (tiled: the tile pipeline's workspace for the long messages, any_tiled_begin below; null: none)
int launch_any_encode(const psy::EncodeArgs &a, int ws, int mode, hipStream_t s, bool pair = false,
                      const psy::AnyTiledArgs *tiled = nullptr) {
#if PSY_HAVE_ANYWS
    if (psy::anyws_generic(ws)) {
        const int e = psy::launch_encode_any(a, ws, mode, s, pair, tiled);
        if (e) return set_err(TDT_E_HIP, std::string("generic encode launch: ") + hipGetErrorString((hipError_t)e));
        return TDT_OK;
    }
#endif
    (void)a, (void)mode, (void)s, (void)ws, (void)pair, (void)tiled;
    return set_err(TDT_E_UNSUPPORTED, "word_size not supported on the GPU path");
}
// the follow-up launch of a decode call: the blobs of a generic word size its kernels deferred
// (grid: workgroups striding over the device-side list; any grid decodes every listed blob)
// (tiled: the decode tile pipeline's workspace for the long blobs, any_dec_begin below; null: none)
int launch_any_decode(const psy::DecodeArgs &a, uint32_t grid, hipStream_t s, bool pair = false,
                      const psy::AnyDecArgs *tiled = nullptr, uint32_t *seen = nullptr) {
#if PSY_HAVE_ANYWS
    if (!a.dlist) return TDT_OK;
    const int e = psy::launch_decode_any(a, std::max(1u, std::min(a.n_msgs, grid)), s, pair, tiled, seen);
    if (e) return set_err(TDT_E_HIP, std::string("generic decode launch: ") + hipGetErrorString((hipError_t)e));
#else
    (void)a, (void)grid, (void)s, (void)pair, (void)tiled, (void)seen;
#endif
    return TDT_OK;
}

bool policy_on(const tdt_ctx *c) {
    // should_transform :192-200 (the size / tensor-shape terms are evaluated per message on
    // the device)
    return !(c->cpu.load() > c->cfg.cpu_usage_threshold) &&
           c->bandwidth.load() < c->cfg.bandwidth_threshold_mbps;
}

template <int WS, int TEAM, int G, int MODE, int LB, int PATH = psy::PATH_BOTH>
int launch_encode_t(psy::EncodeArgs a, hipStream_t s) {
    // one workgroup per message; a launch holds < 2^32 threads, so very large batches take
    // several (message ids come from the ticket, so the look-back order spans them)
    const uint32_t maxb = 0xffffffffu / TEAM;
    for (uint32_t b = 0; b < a.n_msgs; b += maxb)
        hipLaunchKernelGGL((psy::tdt_encode_kernel<WS, TEAM, G, MODE, LB, 0, 0, PATH>), dim3(std::min(maxb, a.n_msgs - b)),
                           dim3(TEAM), 0, s, a);
    return TDT_OK;
}

// ---------------------------------------------------------------------------------------
// Passthrough copies (UNCP): messages that stay UNCP (encode :227-266: below min_tensor_size, the
// policy off, or a size that is not a whole number of words) and UNCP blobs (decode :271-304) get
// a copy list of their own.  Sixteen lanes per entry, 16 entries per 256-lane workgroup,
// grid-stride over the list (its length is device data); a one-wave team per 64-byte message
// cost a whole wave's launch, LDS and header work.  The sixteen lanes run the shared copy
// (psy::copy_shifted, tdt_copy.h); its sources here are the batch's device buffers.
constexpr uint32_t kCopyListLanes = 16;  // (q and l of the kernels below: threadIdx.x >> 4, & 15)
static_assert(kCopyListLanes >= psy::kCopyMinT, "copy_shifted: one byte store per lane covers the head and the tail");

// encode: blob = "UNCP" + payload in the message's slot (slotted batches; PAIR: a scattered batch's
// pair tables, psy::table_at)
template <bool PAIR = false>
__global__ __launch_bounds__(256) void tdt_encode_copy_kernel(psy::EncodeArgs a) {
    const uint32_t n = __builtin_amdgcn_readfirstlane(*a.list_count);
    const uint32_t q = threadIdx.x >> 4, l = threadIdx.x & 15u;
    for (uint32_t i = blockIdx.x * 16u + q; i < n; i += gridDim.x * 16u) {
        const uint32_t msg = a.list[i];
        const uint64_t off0 = a.in_off[psy::table_at<PAIR>(msg, 0)], len = a.in_off[psy::table_at<PAIR>(msg, 1)] - off0;
        const uint64_t sb = a.slot_off[psy::table_at<PAIR>(msg, 0)], E = len + 4;
        const bool fits = E <= a.slot_off[psy::table_at<PAIR>(msg, 1)] - sb;
        if (l == 0) {
            if (a.status) a.status[msg] = fits ? psy::ST_OK : psy::ST_CAPACITY;
            if (a.out_len) a.out_len[msg] = fits ? E : 0;
        }
        if (!fits) continue;
        uint8_t *dst = a.out + sb;
        if (l < 4) dst[l] = (uint8_t)(psy::kMagicUNCP >> (8 * l));
        psy::copy_shifted<1, false>(dst + 4, a.in + off0, len, l, kCopyListLanes);
    }
}

// the size pass (MODE_SIZES) over the copy list: the marker and the payload, nothing is copied (one
// thread per entry; the batch is read through its pair table)
__global__ __launch_bounds__(256) void tdt_encode_copy_sizes_kernel(psy::EncodeArgs a) {
    const uint32_t n = *a.list_count;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t msg = a.list[i];
        const uint64_t len = a.in_off[psy::table_at<true>(msg, 1)] - a.in_off[psy::table_at<true>(msg, 0)];
        if (a.status) a.status[msg] = psy::ST_OK;
        if (a.out_len) a.out_len[msg] = len + 4;
    }
}

// decode: payload of a UNCP blob into its slot
template <bool PAIR = false>
__global__ __launch_bounds__(256) void tdt_decode_copy_kernel(psy::DecodeArgs a) {
    const uint32_t n = __builtin_amdgcn_readfirstlane(*a.list_count);
    const uint32_t q = threadIdx.x >> 4, l = threadIdx.x & 15u;
    for (uint32_t i = blockIdx.x * 16u + q; i < n; i += gridDim.x * 16u) {
        const uint32_t msg = a.list[i];
        const uint64_t boff = a.in_off[msg];
        const uint64_t len = a.in_len ? a.in_len[msg] : a.in_off[msg + 1] - boff;  // >= 4 (the plan)
        const uint64_t ob = a.slot_off[psy::table_at<PAIR>(msg, 0)], osize = len - 4;
        const bool fits = osize <= a.slot_off[psy::table_at<PAIR>(msg, 1)] - ob;
        if (l == 0) {
            if (a.out_len) a.out_len[msg] = fits ? osize : 0;
            if (a.status) a.status[msg] = fits ? psy::ST_OK : psy::ST_CAPACITY;
        }
        if (fits) psy::copy_shifted<1, false>(a.out + ob, a.in + boff + 4, osize, l, kCopyListLanes);
    }
}

// ---------------------------------------------------------------------------------------
// Slotted encode (the hot path): a plan kernel sorts the messages into classes — large
// messages as 64 KiB tiles (histogram + mapping, count, scan, emit), medium messages one
// 512-lane team each, small ones one wave each — into lists whose lengths stay in device
// memory.  The host never reads them: each class kernel is launched twice, a main launch of
// one workgroup per entry whose grid comes from an EARLIER call's counts (CountHist: slack on
// top; the batch size before any count is known), and an overflow launch that walks the
// entries past that grid (grid-stride; it exits at once when there are none).  A class that
// an earlier plan found empty is switched off in the plan (its messages join the medium list,
// which takes any size), so repeated batches of one shape launch exactly what they need.
// Calls are therefore asynchronous and capturable (hipGraphs).
constexpr uint64_t kSmallMax = 4096;  // one-wave teams up to this size
// medium messages above this (the streaming body: more than 8 resident rounds per wave) are
// dispatched first
constexpr uint64_t kBigMin = 65536;
// 256-lane teams (4 waves, 8 resident rounds each: 32 KiB) above kSmallMax up to this size: a
// message-sized 512-lane team would give each wave at most four rounds, and the per-wave fixed
// work (entropy share, flush set-up, header) would weigh twice as much per byte
constexpr uint64_t kMidMax = 32768;
constexpr uint32_t kLmax = 1u << 16;   // large messages per batch (full budget)
// tiles per batch at the full budget: 256 MiB of span histograms (WS KiB per 512 KiB span) —
// 32 GiB of large messages at word size 4 (C4's 4 Mi-message Zipf batch holds 12 GiB of them);
// further large messages in the batch stay medium (one 512-lane team each, streaming)
uint32_t tile_cap_of(int ws) { return (262144u / (uint32_t)ws) * psy::kSpanTiles; }
// the budget a context starts with (512 MiB of large messages); plans that claim more grow it
constexpr uint32_t kL0 = 1024, kT0 = 8192;
// the large-message records (PlanWS::elarge): LMeta | tile entries | tile records | span entries |
// span bins | count-pass tile list, as byte offsets
struct ELargeLayout { size_t tiles, trec, spans, shist, rtiles, bytes; };  // (LMeta at 0)
ELargeLayout elarge_layout(uint32_t lcap, uint32_t tcap, int ws) {
    const size_t sc = tcap / psy::kSpanTiles, tiles = (size_t)lcap * sizeof(psy::LMeta), trec = tiles + 8ull * tcap,
                 spans = trec + sizeof(psy::TileRec) * (size_t)tcap, shist = spans + 8 * sc,
                 rtiles = shist + sc * ws * 1024;  // (WS x 256 u32 bins per span)
    return {tiles, trec, spans, shist, rtiles, rtiles + 8ull * tcap};
}
uint32_t pow2_at_least(uint64_t x, uint32_t lo, uint32_t hi) {
    uint64_t p = lo;
    while (p < x && p < hi) p *= 2;
    return (uint32_t)std::min<uint64_t>(p, hi);
}

int ensure_plan(PlanWS &w, uint32_t n, hipStream_t s, bool scattered = false) {
    const size_t need = psy::plan_layout(n, scattered).bytes;
    return grow_retiring(w.buf, w.bytes, need, psy::cap_double(need, w.bytes), w.retired, s);
}

// ---------------------------------------------------------------------------------------
// Scattered batches (tdt_encode_batch_v / tdt_decode_batch_v): message i at ptr[i], size[i] bytes;
// output i at out_ptr[i], capacity out_cap[i].  With null base pointers an address is an offset, so
// the class kernels' PAIR instances read such a batch through (begin, end) pair tables (table_at,
// tdt_plan.h) that one small kernel writes into the plan buffer in stream order.  It also sums the
// sizes into a plan counter: the tiled-path threshold's "bytes of the batch", which no pointer
// difference gives here.
struct Scatter {
    const uint64_t *ptr, *size;         // messages (encode) or blobs (decode)
    const uint64_t *out_ptr, *out_cap;  // blobs (encode) or decoded messages (decode)
};
struct TableArgs {
    Scatter v;
    uint32_t n;
    ulonglong2 *in_pair;        // null: no input table (decode reads ptr / size as in_off / in_len)
    ulonglong2 *out_pair;
    unsigned long long *bytes;  // += the sizes (zeroed with the plan's counters; null: no plan)
};
__global__ __launch_bounds__(256) void tdt_table_kernel(TableArgs t) {
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    unsigned long long sz = 0;
    if (i < t.n) {
        sz = t.v.size[i];
        if (t.in_pair) {
            const uint64_t b = t.v.ptr[i];
            t.in_pair[i] = make_ulonglong2(b, b + sz);
        }
        const uint64_t ob = t.v.out_ptr[i];
        t.out_pair[i] = make_ulonglong2(ob, ob + t.v.out_cap[i]);
    }
    if (!t.bytes) return;  // (uniform)
    for (int d = 32; d > 0; d >>= 1) sz += __shfl_down(sz, d, 64);
    if ((threadIdx.x & 63u) == 0 && sz) atomicAdd(&s_sum, sz);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(t.bytes, s_sum);
}
// the pair tables of a scattered call in plan buffer `pw` (ensure_plan(..., true) has made the room)
int launch_table(PlanWS &pw, const Scatter &v, uint32_t n, bool in_table, unsigned long long *bytes,
                 const uint64_t *&in_pair, const uint64_t *&out_pair, hipStream_t s) {
    const psy::PlanLayout PL = psy::plan_layout(n, true);
    if (pw.bytes < PL.bytes) return set_err(TDT_E_ARG, "plan buffer without room for the pair tables");
    TableArgs t{v, n, in_table ? reinterpret_cast<ulonglong2 *>(pw.buf + PL.pair[psy::PT_IN]) : nullptr,
                reinterpret_cast<ulonglong2 *>(pw.buf + PL.pair[psy::PT_OUT]), bytes};
    hipLaunchKernelGGL(tdt_table_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, t);
    HIPCHK(hipGetLastError());
    in_pair = reinterpret_cast<const uint64_t *>(t.in_pair);
    out_pair = reinterpret_cast<const uint64_t *>(t.out_pair);
    return TDT_OK;
}

// A contiguous batch read through the PAIR instances (tdt_encoded_sizes_batch: the size pass has no
// instances of its own for offset tables): message i is [base + off[i], base + off[i + 1]), and the
// batch's bytes, off[n] - off[0], go to the plan counter the scattered table kernel sums them into.
struct Contig {
    const uint8_t *base;
    const uint64_t *off;  // n + 1 entries
};
__global__ __launch_bounds__(256) void tdt_offsets_table_kernel(Contig g, uint32_t n, ulonglong2 *in_pair,
                                                                unsigned long long *bytes) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = (uint64_t)(uintptr_t)g.base;
    in_pair[i] = make_ulonglong2(b + g.off[i], b + g.off[i + 1]);
    if (i == 0 && bytes) atomicAdd(bytes, (unsigned long long)(g.off[n] - g.off[0]));
}
int launch_offsets_table(PlanWS &pw, const Contig &g, uint32_t n, unsigned long long *bytes, const uint64_t *&in_pair,
                         hipStream_t s) {
    const psy::PlanLayout PL = psy::plan_layout(n, true);
    if (pw.bytes < PL.bytes) return set_err(TDT_E_ARG, "plan buffer without room for the pair tables");
    auto *tab = reinterpret_cast<ulonglong2 *>(pw.buf + PL.pair[psy::PT_IN]);
    hipLaunchKernelGGL(tdt_offsets_table_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, g, n, tab, bytes);
    HIPCHK(hipGetLastError());
    in_pair = reinterpret_cast<const uint64_t *>(tab);
    return TDT_OK;
}

// Small device → pinned-host copies (plan counters, a host chunk's lengths / statuses / error
// flags) as one kernel's stores over PCIe rather than DMA commands: a DMA read-back queued behind
// a chunk's kernels held up the next chunks' input DMAs behind it (profiles/r05_diag/host_decode/)
struct SmallCopies {
    const uint32_t *src[3];
    uint32_t *dst[3];
    uint32_t words[3];
};
__global__ __launch_bounds__(256) void small_copy_kernel(SmallCopies a) {
    for (int k = 0; k < 3; ++k)
        for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < a.words[k]; i += gridDim.x * 256) a.dst[k][i] = a.src[k][i];
}
int small_copies(hipStream_t s, const void *s0, void *d0, size_t b0, const void *s1 = nullptr, void *d1 = nullptr,
                 size_t b1 = 0, const void *s2 = nullptr, void *d2 = nullptr, size_t b2 = 0) {
    SmallCopies a{{static_cast<const uint32_t *>(s0), static_cast<const uint32_t *>(s1), static_cast<const uint32_t *>(s2)},
                  {static_cast<uint32_t *>(d0), static_cast<uint32_t *>(d1), static_cast<uint32_t *>(d2)},
                  {(uint32_t)(b0 / 4), (uint32_t)(b1 / 4), (uint32_t)(b2 / 4)}};
    const size_t mx = std::max(b0, std::max(b1, b2)) / 4;
    hipLaunchKernelGGL(small_copy_kernel, dim3((uint32_t)std::min<size_t>(64, mx / 1024 + 1)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    return TDT_OK;
}

// The plan counters of this call → pinned snapshot (not under stream capture).
template <class K>
int record_counts(CountHist<K> &h, const void *dcnt, uint32_t n_msgs, hipStream_t s) {
    if (!h.pin) {
        HIPCHK(hipHostMalloc(&h.pin, psy::kPlanSnapBytes, hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&h.ev, hipEventDisableTiming));
    }
    if (int st = small_copies(s, dcnt, h.pin, psy::kPlanSnapBytes)) return st;
    HIPCHK(hipEventRecord(h.ev, s));
    h.n_pending = n_msgs;
    h.pending = true;
    return TDT_OK;
}

// Main-launch grid of a class: the earlier count plus slack (capped), or `dflt` before any.
template <class K>
uint32_t guess(const CountHist<K> &h, K k, uint32_t bound, uint32_t dflt) {
    if (!h.valid) return std::min(dflt, bound);
    const uint64_t x = h[k];
    return (uint32_t)std::min<uint64_t>(x + x / 8 + 64, bound);
}

// fork `s` onto the side stream (high priority: the tile pipeline is a chain of dependent
// kernels; the independent medium/small lists fill the CUs it leaves idle at each boundary)
int fork_side(PlanWS &w, hipStream_t s) {
    if (!w.side) {
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&w.side, hipStreamNonBlocking, hi));
        HIPCHK(hipEventCreateWithFlags(&w.fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&w.join, hipEventDisableTiming));
    }
    HIPCHK(hipEventRecord(w.fork, s));
    HIPCHK(hipStreamWaitEvent(w.side, w.fork, 0));
    return TDT_OK;
}
int join_side(PlanWS &w, hipStream_t s) {
    HIPCHK(hipEventRecord(w.join, w.side));
    HIPCHK(hipStreamWaitEvent(s, w.join, 0));
    return TDT_OK;
}

// Large-message budget: allocated on the first batch that may hold large messages, grown to
// what an earlier plan claimed.
int ensure_elarge(PlanWS &w, int ws, hipStream_t s) {
    uint32_t lc = w.e_lcap ? w.e_lcap : kL0, tc = w.e_tcap ? w.e_tcap : kT0;
    if (w.eh.valid) {
        lc = std::max(lc, pow2_at_least(w.eh[psy::EC_LARGE], kL0, kLmax));
        const uint64_t t = std::max<uint64_t>(w.eh[psy::EC_TILES], (uint64_t)w.eh[psy::EC_SPANS] * psy::kSpanTiles);
        tc = std::max(tc, pow2_at_least(t, kT0, tile_cap_of(ws)));
    }
    if (w.elarge && lc == w.e_lcap && tc == w.e_tcap) return TDT_OK;
    if (w.elarge) {
        // retired, not freed: earlier calls still queued, or a graph captured on the warm
        // context, may use the old records (their launches carry the old budgets)
        w.retired.push_back(w.elarge);
        w.elarge = nullptr;
        w.e_lcap = w.e_tcap = 0;
    }
    const size_t b = elarge_layout(lc, tc, ws).bytes;
    HIPCHK(hipMalloc(&w.elarge, b));
    HIPCHK(hipMemsetAsync(w.elarge, 0, b, s));
    w.e_lcap = lc;
    w.e_tcap = tc;
    return TDT_OK;
}

// ---------------------------------------------------------------------------------------
// The tiled generic-width encode's workspace (AnyTiledWS; the kernels: tdt_anyws.h).  A call that
// may launch the generic encode brackets it: any_tiled_begin (grows the buffers, zeroes the
// counters, fills the kernels' arguments), the pair tables with AnyTiled::bytes as their byte
// counter, launch_any_encode(..., AnyTiled::args()), any_tiled_end (the counters → the pinned
// snapshot).  The host reads nothing back: the next call sizes the budgets from the snapshot.
constexpr uint32_t kAnyL0 = 64, kAnyLmax = 4096;         // large messages per batch: the start, the full budget (64 KiB of histogram each)
constexpr uint32_t kAnyT0 = 8192, kAnyTmax = 1u << 20;   // tiles per batch: 512 MiB of long messages, 64 GiB
struct AnyRecLayout { size_t tiles, hist, bytes; };      // (the AnyLarge records at 0)
AnyRecLayout any_rec_layout(uint32_t lcap, uint32_t tcap) {
    const size_t tiles = (size_t)lcap * sizeof(psy::AnyLarge), hist = tiles + (size_t)tcap * sizeof(psy::AnyTile);
    return {tiles, hist, hist + (size_t)lcap * psy::kAnyWsMax * 256 * sizeof(uint32_t)};
}
struct AnyTiled {
    psy::AnyTiledArgs t{};
    bool on = false;
    // the byte counter of a pair-table batch (`route`: the width's index in a mixed-width call)
    unsigned long long *bytes(int route = 0) const { return on ? t.cnt + psy::AC_BYTES + route : nullptr; }
    const psy::AnyTiledArgs *args(int route = 0) {
        t.bytes_at = (uint32_t)(psy::AC_BYTES + route);
        return on ? &t : nullptr;
    }
};
// own: the call holds the context's lock (a host-pipeline slot does not: its messages stay untiled)
int any_tiled_begin(tdt_ctx *c, bool own, uint32_t n, hipStream_t s, AnyTiled &x) {
    x = AnyTiled{};
    if (!PSY_HAVE_ANYWS || !own || !c->any_tiled || n == 0) return TDT_OK;
    AnyTiledWS &w = c->anyw;
    const bool cap = capturing(s);
    auto &H = w.h;
    if (!cap) H.refresh();  // (event queries are not capturable)
    const size_t need = psy::kPlanCounterBytes + 4ull * n;
    if (int st = grow_retiring(w.buf, w.bytes, need, psy::cap_double(need, w.bytes), c->retired, s)) return st;
    // the tile pipeline is off when an earlier plan found no long message (its launches would find none)
    const bool tiles_on = !H.valid || H[psy::AC_LARGE] > 0;
    if (tiles_on) {
        uint32_t lc = w.lcap ? w.lcap : kAnyL0, tc = w.tcap ? w.tcap : kAnyT0;
        if (H.valid) {  // what an earlier plan claimed, beyond its budget too
            lc = std::max(lc, pow2_at_least(H[psy::AC_LARGE], kAnyL0, kAnyLmax));
            tc = std::max(tc, pow2_at_least(H[psy::AC_TILES], kAnyT0, kAnyTmax));
        }
        if (lc != w.lcap || tc != w.tcap) {
            if (int st = no_growth_in_capture(s)) return st;
            const AnyRecLayout RL = any_rec_layout(lc, tc);
            w.lcap = w.tcap = 0;
            // (retired, not freed: calls still queued, or a captured graph, may use the old records)
            if (int st = psy::grow(w.rec, w.rec_bytes, RL.bytes, RL.bytes, retire_to(c->retired), DevAlloc{})) return st;
            HIPCHK(hipMemsetAsync(w.rec, 0, RL.bytes, s));  // (the histograms are zero between calls)
            w.lcap = lc;
            w.tcap = tc;
        }
    }
    HIPCHK(hipMemsetAsync(w.buf, 0, psy::kPlanSnapBytes, s));
    const AnyRecLayout RL = any_rec_layout(w.lcap, w.tcap);
    x.on = true;
    x.t.large = reinterpret_cast<psy::AnyLarge *>(w.rec);
    x.t.tiles = reinterpret_cast<psy::AnyTile *>(w.rec + RL.tiles);
    x.t.hist = reinterpret_cast<uint32_t *>(w.rec + RL.hist);
    x.t.mark = reinterpret_cast<uint32_t *>(w.buf + psy::kPlanCounterBytes);
    x.t.cnt = reinterpret_cast<unsigned long long *>(w.buf);
    x.t.lcap = tiles_on && w.rec ? w.lcap : 0u;
    x.t.tcap = tiles_on && w.rec ? std::min(w.tcap, std::max(c->tile_cap, 1u)) : 0u;
    x.t.grid = (uint32_t)c->cus * 8u;
    x.t.large_min = c->large_min;
    return TDT_OK;
}
int any_tiled_end(tdt_ctx *c, const AnyTiled &x, uint32_t n, hipStream_t s) {
    if (!x.on || capturing(s)) return TDT_OK;
    return record_counts(c->anyw.h, c->anyw.buf, n, s);
}

// ---------------------------------------------------------------------------------------
// The tiled generic-width decode's workspace (AnyDecWS; the kernels: tdt_anyws.h), handled as the
// encode's above: budgets that start small, the claims in a counter block, the pinned snapshot behind
// the call, growth in powers of two on a later call with the old buffer retired.  The host reads
// nothing back.  Under stream capture nothing grows and nothing is snapshotted, and the call never
// fails because of this workspace: what finds no budget stays on the one-workgroup kernel.
constexpr uint32_t kAnyDL0 = 64, kAnyDLmax = 1u << 16;      // long blobs per batch
constexpr uint32_t kAnyDB0 = 1u << 18, kAnyDBmax = 1u << 26; // block sums (4 KiB of pairs each): 512 MiB of long blobs and more, 256 GiB
constexpr uint32_t kAnyDT0 = 16384, kAnyDTmax = 1u << 22;   // 32 KiB tiles: 512 MiB of output, 128 GiB
size_t any_dec_rec_bytes(uint32_t lcap, uint32_t bcap) { return (size_t)lcap * sizeof(psy::AnyDecLarge) + 4ull * bcap; }
// The follow-up launch of a decode call (launch_any_decode) with the tile pipeline beside it.
// own: the call holds the context's lock (a host-pipeline slot does not: its blobs stay untiled).
// batch_bytes: a scattered batch's byte counter (DC_BYTES of its plan).
int decode_deferred(tdt_ctx *c, bool own, const psy::DecodeArgs &a, hipStream_t s, bool pair = false,
                    const unsigned long long *batch_bytes = nullptr) {
    const uint32_t grid = (uint32_t)c->cus * 4u, n = a.n_msgs;
    if (!PSY_HAVE_ANYWS || !a.dlist) return TDT_OK;
    if (!own || !c->any_dec_tiled || n == 0) return launch_any_decode(a, grid, s, pair);
    AnyDecWS &w = c->anydw;
    const bool cap = capturing(s);
    if (!w.seen) {
        if (cap) return launch_any_decode(a, grid, s, pair);  // (a cold context: nothing to allocate under capture)
        HIPCHK(hipHostMalloc(&w.seen, sizeof(uint32_t), hipHostMallocDefault));
        *w.seen = ~0u;  // (unknown)
    }
    // no call has listed a blob yet: a call like them pays no launch for the long blobs it does not have
    if (*static_cast<volatile uint32_t *>(w.seen) == 0u) return launch_any_decode(a, grid, s, pair, nullptr, w.seen);
    auto &H = w.h;
    if (!cap) H.refresh();  // (event queries are not capturable)
    const size_t need = psy::kPlanCounterBytes + 4ull * n;
    if (need > w.bytes) {
        if (cap) return launch_any_decode(a, grid, s, pair, nullptr, w.seen);
        if (int st = grow_retiring(w.buf, w.bytes, need, psy::cap_double(need, w.bytes), c->retired, s)) return st;
    }
    // the tile pipeline is off when an earlier plan found no long blob (its launches would find none)
    const bool tiles_on = !H.valid || H[psy::ADC_LARGE] > 0;
    if (tiles_on && !cap) {
        uint32_t lc = w.lcap ? w.lcap : kAnyDL0, bc = w.bcap ? w.bcap : kAnyDB0, tc = w.tcap ? w.tcap : kAnyDT0;
        if (H.valid) {  // what an earlier plan claimed, beyond its budget too
            lc = std::max(lc, pow2_at_least(H[psy::ADC_LARGE], kAnyDL0, kAnyDLmax));
            bc = std::max(bc, pow2_at_least(H[psy::ADC_BLOCKS], kAnyDB0, kAnyDBmax));
            tc = std::max(tc, pow2_at_least(H[psy::ADC_TILES], kAnyDT0, kAnyDTmax));
        }
        if (lc != w.lcap || bc != w.bcap) {
            const size_t b = any_dec_rec_bytes(lc, bc);
            w.lcap = w.bcap = 0;
            // (retired, not freed: calls still queued, or a captured graph, may use the old records)
            if (int st = psy::grow(w.rec, w.rec_bytes, b, b, retire_to(c->retired), DevAlloc{})) return st;
            w.lcap = lc;
            w.bcap = bc;
        }
        w.tcap = tc;
    }
    HIPCHK(hipMemsetAsync(w.buf, 0, psy::kPlanSnapBytes, s));
    psy::AnyDecArgs t{};
    t.large = reinterpret_cast<psy::AnyDecLarge *>(w.rec);
    t.bsum = reinterpret_cast<uint32_t *>(w.rec + (size_t)w.lcap * sizeof(psy::AnyDecLarge));
    t.mark = reinterpret_cast<uint32_t *>(w.buf + psy::kPlanCounterBytes);
    t.cnt = reinterpret_cast<unsigned long long *>(w.buf);
    t.batch_bytes = batch_bytes;
    const bool on = tiles_on && w.rec;
    t.lcap = on ? w.lcap : 0u;
    t.bcap = on ? w.bcap : 0u;
    t.tcap = on ? std::min(w.tcap, std::max(c->tile_cap, 1u)) : 0u;
    t.grid = (uint32_t)c->cus * 8u;
    t.large_min = c->large_min;
    if (int st = launch_any_decode(a, grid, s, pair, &t, w.seen)) return st;
    return cap ? TDT_OK : record_counts(H, w.buf, n, s);
}

// grid of one list-driven launch of TEAM-lane workgroups over `count` entries (launches of
// < 2^32 threads each)
template <class F>
void launch_list(uint32_t count, uint32_t team, F &&launch) {
    const uint32_t mx = 0xffffffffu / team;
    for (uint32_t b = 0; b < count; b += mx) launch(b, std::min(mx, count - b));
}

// One class of a slotted call: the main launch, one workgroup per entry over [0, g) (g from an
// earlier plan's count, guess(); launches of < 2^32 threads each), then the overflow launch of at
// most `ovf` workgroups striding over [g, bound).  `list` and its length, counter `k`, go into the
// kernels' arguments (null for the tile passes: their entries are the large-message records).
template <class Args>
struct ClassLaunch {
    Args &a;
    const uint32_t *cnt;  // u32 view of the plan's counter block
    template <class K, class KM, class KO>
    void operator()(const uint32_t *list, K k, uint32_t g, uint32_t bound, uint32_t team, uint32_t ovf, hipStream_t s,
                    KM main_k, KO over_k) const {
        if (list) {
            a.list = list;
            a.list_count = cnt + psy::lo32(k);
        }
        launch_list(g, team, [&](uint32_t b, uint32_t grid) {
            a.list_base = b;
            hipLaunchKernelGGL(main_k, dim3(grid), dim3(team), 0, s, a);
        });
        if (g < bound) {
            a.list_base = g;
            hipLaunchKernelGGL(over_k, dim3(std::min(ovf, bound - g)), dim3(team), 0, s, a);
        }
    }
};

// cfg.word_size as a compile-time WS: f(Int<WS>), W() in f, for the tuned word sizes (diagnostic
// builds: 4 only); false for every other one (the callers' generic-width routes)
template <int V>
using Int = std::integral_constant<int, V>;
template <class F>
bool with_word_size(int ws, F &&f) {
    switch (ws) {
#ifndef PSY_FAST_BUILD
        case 1: f(Int<1>{}); return true;
        case 2: f(Int<2>{}); return true;
        case 8: f(Int<8>{}); return true;
        case 16: f(Int<16>{}); return true;
#endif
        case 4: f(Int<4>{}); return true;
        default: return false;
    }
}

// The tables of one width of a mixed-width batch (tdt_encode_batch_vw): the route kernel has written
// them, behind the zeroing of this width's plan counters, and has summed the width's bytes into EC_BYTES
struct Routed {
    const uint64_t *in_pair, *out_pair;
};

// PAIR: a scattered batch (`v`): its pair tables first, then the same classes through the PAIR
// instances; or one width of a mixed-width batch (`r`), whose tables are there already.
// MODE_SIZES (PAIR only): the size pass — the same plan, lists, grids and count history, through
// the size-pass instances of every class; the emit pass of the tiles is not launched, the copy
// list is sized by its own kernel, and the batch has no outputs: a scattered one's out_ptr / out_cap
// are any readable arrays of n entries (the table kernel reads them, nothing reads what it writes
// from them), a contiguous one (`g`) gets its input table from its offsets.
// MODE_MAPPED (PAIR only): the known-mapping encode (a.mapping_in: one u64 of mapping bits per
// message) — the same plan, lists, grids, side stream and count history through the mapped
// instances of every whole-message class.  In the tile pipeline two small kernels (tdt_enc_lmap.h)
// stand in for the span and map passes, which have nothing to compute; the count pass, the scan and
// the emit pass are the ordinary encode's own instances (they read the mapping from LMeta).
template <int WS, bool PAIR = false, int MODE = psy::MODE_ENCODE>
int launch_slotted(tdt_ctx *c, PlanWS &pw, psy::EncodeArgs a, hipStream_t s, const Scatter *v = nullptr,
                   const Routed *r = nullptr, const Contig *g = nullptr) {
    static_assert(MODE == psy::MODE_ENCODE || ((MODE == psy::MODE_SIZES || MODE == psy::MODE_MAPPED) && PAIR),
                  "slotted encode, its size pass, or its known-mapping form");
    constexpr bool SIZES = MODE == psy::MODE_SIZES, MAPPED = MODE == psy::MODE_MAPPED;
    using namespace psy;  // (counter, list and kernel names)
    const uint32_t n = a.n_msgs;
    // the list-entry prefetch of the slotted kernels (EncodeArgs::list) reads entry
    // min(i, n - 1) of a class list before its count: n >= 1, and every list holds n entries
    // (ensure_plan: five lists of n entries behind the counters)
    if (n == 0) return set_err(TDT_E_ARG, "slotted encode launch without messages");
    if (PAIR != (v != nullptr || r != nullptr || g != nullptr)) return set_err(TDT_E_ARG, "scattered launch without its arrays");
    if (g && !SIZES) return set_err(TDT_E_ARG, "a contiguous batch runs the PAIR instances in the size pass only");
    int st = ensure_plan(pw, n, s, PAIR && !r);
    if (st) return st;
    const PlanLayout PL = plan_layout(n);
    if (pw.bytes < PL.bytes) return set_err(TDT_E_ARG, "plan buffer smaller than five lists of n entries");
    const bool capturing = ::capturing(s);
    auto &H = pw.eh;
    if (!capturing) H.refresh();  // (event queries are not capturable)
    // classes an earlier plan found empty are off (their messages, if any, go medium)
    const bool small_on = !H.valid || H[EC_SMALL_ALL] > 0;
    const bool mid_on = !H.valid || H[EC_MID_ALL] > 0;
    const bool copy_on = !H.valid || H[EC_UNCP_ALL] > 0;
    bool tiles_on = !H.valid || H[EC_LARGE] > 0;
    if (tiles_on && !capturing) {
        st = ensure_elarge(pw, WS, s);
        if (st) return st;
    }
    tiles_on = tiles_on && pw.elarge;
    auto *cnt64 = reinterpret_cast<unsigned long long *>(pw.buf);
    auto *cnt = reinterpret_cast<uint32_t *>(pw.buf);  // cnt[lo32(k)]: the low word of counter k
    auto list = [&](EncList l) { return reinterpret_cast<uint32_t *>(pw.buf + PL.list[l]); };
    const uint32_t lcap = tiles_on ? pw.e_lcap : 0u;
    const uint32_t tcap = tiles_on ? std::min(pw.e_tcap, std::max(c->tile_cap, kSpanTiles)) : 0u;
    const uint32_t scap = tcap / kSpanTiles;
    // (the records lie where the allocated budgets put them, whatever this call's tcap)
    const ELargeLayout EL = elarge_layout(pw.e_lcap, pw.e_tcap, WS);
    auto *lmeta = reinterpret_cast<LMeta *>(pw.elarge);
    auto *tiles = reinterpret_cast<uint64_t *>(pw.elarge + EL.tiles);
    auto *spans = reinterpret_cast<uint64_t *>(pw.elarge + EL.spans);
    if (!r) HIPCHK(hipMemsetAsync(cnt, 0, kPlanSnapBytes, s));
    if constexpr (PAIR) {  // the pair tables and the batch's byte count, then every kernel below as usual
        if (r) {
            a.in_off = r->in_pair;
            a.slot_off = r->out_pair;
        } else if (g) {
            if ((st = launch_offsets_table(pw, *g, n, cnt64 + EC_BYTES, a.in_off, s))) return st;
        } else if ((st = launch_table(pw, *v, n, true, cnt64 + EC_BYTES, a.in_off, a.slot_off, s))) {
            return st;
        }
        if constexpr (SIZES) {  // the table holds addresses; there are no slots, and nothing may read any
            a.in = nullptr;
            a.out = nullptr;
            a.slot_off = nullptr;
        }
    }
    PlanArgs p{a.in, a.in_off, n, cnt64, list(EL_SMALL), list(EL_MEDIUM), list(EL_MID), list(EL_BIG), list(EL_COPY),
               tiles, spans, lmeta, lcap, tcap, kSmallMax, kMidMax, kBigMin, c->large_min, small_on ? 1u : 0u,
               mid_on ? 1u : 0u, a.min_tensor, (uint32_t)a.policy_on, (uint32_t)WS, copy_on ? 1u : 0u};
    const uint32_t per = kPlanThreads * kPlanPer;
    hipLaunchKernelGGL(tdt_encode_plan_kernel<PAIR>, dim3((uint32_t)(((uint64_t)n + per - 1) / per)), dim3(kPlanThreads), 0, s,
                       p);
    HIPCHK(hipGetLastError());
    // (with tiles, the snapshot follows the map pass instead: it also holds the count pass's list length)
    if (!capturing && !tiles_on && (st = record_counts(H, cnt, n, s))) return st;
    a.pcnt = cnt;
    const uint32_t ovf512 = (uint32_t)c->cus * 3, ovf256 = (uint32_t)c->cus * 6, ovf64 = (uint32_t)c->cus * 24;
    const ClassLaunch<EncodeArgs> cls{a, cnt};
    bool forked = false;
    hipStream_t ts = s;  // the tile pipeline's (and the small / mid-sized lists') stream
    // the side stream carries the tile pipeline and the small / mid-sized lists beside the medium
    // list (queued behind it on one stream they would run alone in its tail)
    const bool medium_on = !H.valid || H[EC_MEDIUM] + H[EC_BIG] > 0;
    if (tiles_on || ((small_on || mid_on || copy_on) && medium_on && !c->small_main)) {
        const int fr = c->no_side || pw.no_side ? -1 : fork_side(pw, s);
        if (fr > 0) return fr;
        forked = fr == TDT_OK;
        if (forked) ts = pw.side;
    }
    if (tiles_on) {
        a.tiles = tiles;
        a.spans = spans;
        a.lmeta = lmeta;
        a.trec = reinterpret_cast<TileRec *>(pw.elarge + EL.trec);
        a.shist = reinterpret_cast<uint32_t *>(pw.elarge + EL.shist);
        a.rtiles = reinterpret_cast<uint64_t *>(pw.elarge + EL.rtiles);
        a.rcount = cnt64 + EC_RECOUNT;
        a.lcap = lcap;
        a.tcap = tcap;
        // (a known-mapping batch counts and emits with the ordinary encode's tile instances)
        constexpr int TMODE = MAPPED ? (int)MODE_ENCODE : MODE;
        auto tile_pass = [&](auto TL, EncCount k, uint32_t bound) {  // (no main launch before any count is known)
            cls(nullptr, k, guess(H, k, bound, 0), bound, 512, ovf512, ts,
                tdt_encode_kernel<WS, 512, 8, TMODE, 0, TL(), 0, PATH_BOTH, PAIR>,
                tdt_encode_kernel<WS, 512, 8, TMODE, 0, TL(), 1, PATH_BOTH, PAIR>);
        };
        if constexpr (MAPPED) {
            // the caller's mappings into the records, every tile on the count list; large passthrough copies
            hipLaunchKernelGGL(tdt_encode_lcopy_kernel, dim3(std::max(1u, std::min(scap, ovf512))), dim3(512), 0, ts, a,
                               (uint32_t)WS);
            hipLaunchKernelGGL(tdt_encode_lmap_kernel, dim3(std::max(1u, std::min(lcap, 1024u))), dim3(64), 0, ts, a,
                               (uint32_t)WS);
        } else {
            tile_pass(Int<1>{}, EC_SPANS, scap);  // span histograms (and counts under the speculated mapping)
            tile_pass(Int<4>{}, EC_LARGE, lcap);  // mapping per large message; lists the tiles to count again
        }
        if (!capturing && (st = record_counts(H, cnt, n, ts))) return st;
        tile_pass(Int<2>{}, EC_RECOUNT, tcap);  // per-tile counts of the listed tiles
        if constexpr (SIZES) {  // the scan alone: it has the pair counts, and there is nothing to emit
            hipLaunchKernelGGL((tdt_encode_lscan_sizes_kernel<WS>), dim3(std::max(1u, std::min(lcap, 1024u))), dim3(64), 0, ts,
                               a, cnt + lo32(EC_LARGE), lcap);
        } else {
            hipLaunchKernelGGL((tdt_encode_lscan_kernel<WS, PAIR>), dim3(std::max(1u, std::min(lcap, 1024u))), dim3(64), 0, ts, a,
                               cnt + lo32(EC_LARGE), lcap);
            tile_pass(Int<3>{}, EC_TILES, tcap);  // emit
        }
    }
    // medium messages: one workgroup per list entry — the big list first (longer or unaligned
    // messages: the streaming-only kernel; a long team started last would run alone in the
    // kernel's tail), then the medium list (resident-only kernel).  Both are always launched
    // (messages of a class switched off join them; the overflow launch ends at once when the list
    // is empty); the big list has no main launch when the history says it is empty
    a.list2 = nullptr;
    cls(list(EL_BIG), EC_BIG, H.valid && !H[EC_BIG] ? 0u : guess(H, EC_BIG, n, n), n, 512, ovf512, s,
        tdt_encode_kernel<WS, 512, 8, MODE, 0, 0, 0, PATH_STREAM, PAIR>,
        tdt_encode_kernel<WS, 512, 8, MODE, 0, 0, 1, PATH_STREAM, PAIR>);
    cls(list(EL_MEDIUM), EC_MEDIUM, guess(H, EC_MEDIUM, n, n), n, 512, ovf512, s,
        tdt_encode_kernel<WS, 512, 8, MODE, 0, 0, 0, PATH_RES, PAIR>,
        tdt_encode_kernel<WS, 512, 8, MODE, 0, 0, 1, PATH_RES, PAIR>);
    // the small, copy and mid-sized lists behind the tile pipeline on the side stream (the two
    // streams' loads balance better: C4's tile pipeline is shorter than its medium list)
    const hipStream_t ss = forked && !c->small_main ? pw.side : s;
    if (small_on)  // one-wave teams
        cls(list(EL_SMALL), EC_SMALL, guess(H, EC_SMALL, n, n), n, 64, ovf64, ss,
            tdt_encode_kernel<WS, 64, 4, MODE, 0, 0, 0, PATH_BOTH, PAIR>,
            tdt_encode_kernel<WS, 64, 4, MODE, 0, 0, 1, PATH_BOTH, PAIR>);
    if (copy_on) {  // passthrough copies
        a.list = list(EL_COPY);
        a.list_count = cnt + lo32(EC_UNCP);
        if constexpr (SIZES)
            hipLaunchKernelGGL(tdt_encode_copy_sizes_kernel, dim3(std::max(1u, std::min((uint32_t)c->cus, (n + 255) / 256))),
                               dim3(256), 0, ss, a);
        else
            hipLaunchKernelGGL(tdt_encode_copy_kernel<PAIR>,
                               dim3(std::max(1u, std::min((uint32_t)c->cus * c->copy_wgs, (n + 15) / 16))), dim3(256), 0, ss, a);
    }
    if (mid_on)  // 256-lane teams
        cls(list(EL_MID), EC_MID, guess(H, EC_MID, n, n), n, 256, ovf256, ss,
            tdt_encode_kernel<WS, 256, 8, MODE, 0, 0, 0, PATH_BOTH, PAIR>,
            tdt_encode_kernel<WS, 256, 8, MODE, 0, 0, 1, PATH_BOTH, PAIR>);
    if (forked) return join_side(pw, s);
    return TDT_OK;
}

// mapped: the known-mapping form of a scattered batch (a.mapping_in: mapping bits, tdt_mapbits.h)
int launch_slotted_any(tdt_ctx *c, PlanWS &pw, psy::EncodeArgs a, hipStream_t s, const Scatter *v = nullptr,
                       bool mapped = false) {
    int st = TDT_OK;
    if (mapped && !v) return set_err(TDT_E_ARG, "the known-mapping slotted encode is a scattered call");
    if (with_word_size(c->cfg.word_size, [&](auto W) {
            st = mapped ? launch_slotted<W(), true, psy::MODE_MAPPED>(c, pw, a, s, v)
                 : v    ? launch_slotted<W(), true>(c, pw, a, s, v)
                        : launch_slotted<W()>(c, pw, a, s);
        }))
        return st;
    // generic widths: one workgroup per message, message id = block index; the long ones as tiles
    AnyTiled x;
    if (psy::anyws_generic(c->cfg.word_size) && (st = any_tiled_begin(c, &pw == &c->pw, a.n_msgs, s, x))) return st;
    if (v && psy::anyws_generic(c->cfg.word_size)) {  // (the plan buffer holds the pair tables alone)
        if ((st = ensure_plan(pw, a.n_msgs, s, true))) return st;
        if ((st = launch_table(pw, *v, a.n_msgs, true, x.bytes(), a.in_off, a.slot_off, s))) return st;
    }
    st = launch_any_encode(a, c->cfg.word_size, mapped ? psy::MODE_MAPPED : psy::MODE_ENCODE, s, v != nullptr, x.args());
    return st ? st : any_tiled_end(c, x, a.n_msgs, s);
}

// ---------------------------------------------------------------------------------------
// Mixed word sizes (tdt_encode_batch_vw): a scattered batch with one record width per message.  The
// host knows the widths that may occur (the caller's mask), never which message has which.  One
// route kernel writes a pair of tables per width of the mask — a message's entry in its own
// width's tables, psy's ABSENT entry in every other — and sums each width's sizes into that
// width's EC_BYTES; then every width runs its usual pipeline over its tables: launch_slotted for a
// tuned width (a PlanWS and count history of its own), the generic encode for any other.  A class
// kernel reaches a message only through a plan list, the generic encode's workgroup leaves at an
// absent entry, and status / out_len are indexed by message id: each message is written by its
// width's pipeline alone, or — a width outside 1..64 or outside the mask — by the route kernel.
struct RouteArgs {
    Scatter v;
    const int32_t *ws;  // width per message
    uint32_t n, n_routes;
    int32_t width[psy::kMixedMaxWidths];
    ulonglong2 *in_pair[psy::kMixedMaxWidths], *out_pair[psy::kMixedMaxWidths];
    unsigned long long *bytes[psy::kMixedMaxWidths];  // += the width's sizes (null: a generic width, no plan)
    int32_t *status;
    uint64_t *out_len;
};
__global__ __launch_bounds__(256) void tdt_route_kernel(RouteArgs t) {
    __shared__ unsigned long long s_sum[psy::kMixedMaxWidths];
    if (threadIdx.x < psy::kMixedMaxWidths) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    int route = -1;
    unsigned long long sz = 0;
    uint64_t ib = psy::kAbsentBegin, ie = psy::kAbsentEnd, ob = psy::kAbsentBegin, oe = psy::kAbsentEnd;
    if (i < t.n) {
        const int32_t w = t.ws[i];
#pragma unroll  // (constant indices: the argument arrays stay in scalar registers)
        for (uint32_t k = 0; k < (uint32_t)psy::kMixedMaxWidths; ++k)
            if (k < t.n_routes && t.width[k] == w) route = (int)k;
        if (route >= 0) {
            sz = t.v.size[i];
            ib = t.v.ptr[i];
            ie = ib + sz;
            ob = t.v.out_ptr[i];
            oe = ob + t.v.out_cap[i];
        } else {  // rejected: no pipeline sees it
            if (t.status) t.status[i] = w <= 0 ? psy::ST_CONFIG : w > psy::kMixedWsMax ? psy::ST_UNSUPPORTED : psy::ST_ARG;
            if (t.out_len) t.out_len[i] = 0;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)psy::kMixedMaxWidths; ++k) {  // (uniform)
        if (k >= t.n_routes) continue;
        const bool mine = route == (int)k;
        if (i < t.n) {
            t.in_pair[k][i] = make_ulonglong2(mine ? ib : psy::kAbsentBegin, mine ? ie : psy::kAbsentEnd);
            t.out_pair[k][i] = make_ulonglong2(mine ? ob : psy::kAbsentBegin, mine ? oe : psy::kAbsentEnd);
        }
        if (!t.bytes[k]) continue;
        unsigned long long x = mine ? sz : 0ull;
        for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
        if ((threadIdx.x & 63u) == 0 && x) atomicAdd(&s_sum[k], x);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)psy::kMixedMaxWidths; ++k)
        if (threadIdx.x == k && k < t.n_routes && t.bytes[k] && s_sum[k]) atomicAdd(t.bytes[k], s_sum[k]);
}

// Where a batch call runs.  What it works on goes in psy::EncodeArgs / psy::DecodeArgs, whose
// caller-visible fields the entry points fill by name (in, in_off, n_msgs, out, out_cap, out_off,
// status, mapping_in, hist_out, ent_out, map_out, slot_off, out_len, in_len, sizes_out).
struct Where {
    hipStream_t stream = nullptr;
    uint8_t *wsp = nullptr;     // an explicit workspace (host-pipeline slots own theirs); null: the context's
    PlanWS *pws = nullptr;      // the slotted calls' plan workspace; null: the context's
    int small_teams = -1;       // look-back team shape (launch_encode)
    const Scatter *v = nullptr; // a scattered batch: in, out and the offset tables are null
    Where(void *s) : stream((hipStream_t)s) {}
};

// The fields no caller sets: the workspace's words (a null `wsp`: the one-message block, which
// holds its own error flags) and, for encode, the context's policy.
template <class Args>
void wire_workspace(Args &a, uint8_t *wsp) {
    a.ticket = reinterpret_cast<uint32_t *>(wsp);
    a.errflags = reinterpret_cast<uint32_t *>(wsp) + 1;
    a.lookback = reinterpret_cast<uint64_t *>(wsp + kCounterBytes);
}
void wire_encode(const tdt_ctx *c, psy::EncodeArgs &a, uint8_t *wsp) {
    if (wsp) wire_workspace(a, wsp);
    a.min_tensor = c->cfg.min_tensor_size;
    a.policy_on = policy_on(c) ? 1 : 0;
}
// lookback: the one-pass route, whose deferred-blob list (generic word sizes) lies in the workspace
// behind the look-back words (the slotted route keeps it in the plan buffer)
void wire_decode(psy::DecodeArgs &a, uint8_t *wsp, bool lookback) {
    wire_workspace(a, wsp);
    if (PSY_HAVE_ANYWS && lookback) {
        a.dlist = reinterpret_cast<uint32_t *>(wsp + kCounterBytes + 8ull * (a.n_msgs + 1));
        a.dcount = reinterpret_cast<uint32_t *>(wsp) + 2;  // (zeroed with the counters by prep)
    }
}

int tuned_index(int ws) { return ws == 1 ? 0 : ws == 2 ? 1 : ws == 4 ? 2 : ws == 8 ? 3 : 4; }
int prep(tdt_ctx *c, uint32_t n_msgs, hipStream_t s, uint8_t *&wsp, bool lookback);  // (below)

// mode: MODE_ENCODE, or MODE_SIZES — the size pass of every width over the same routes and plan
// workspaces (v.out_ptr / v.out_cap: any readable arrays of n entries, see launch_slotted), which
// also writes the mapping bits of every compressed message to d_mapbits when that is set — or
// MODE_MAPPED, the known-mapping encode of every width, which reads d_mapbits (n u64, tdt_mapbits.h)
int encode_mixed(tdt_ctx *c, const Scatter &v, const int32_t *d_word_size, uint64_t width_mask, uint32_t n,
                 uint64_t *d_out_len, int32_t *d_status, hipStream_t s, int mode = psy::MODE_ENCODE,
                 uint64_t *d_mapbits = nullptr) {
    if (!c) return set_err(TDT_E_ARG, "null context");
    if (n == 0) return TDT_OK;
    if (!(v.ptr && v.size && v.out_ptr && v.out_cap && d_word_size))
        return set_err(TDT_E_ARG, "null pointer, size or word-size array");
    if (mode == psy::MODE_MAPPED && !d_mapbits) return set_err(TDT_E_ARG, "null mapping");
    psy::MixedRoutes R{};
    if (!psy::mixed_routes(width_mask, n, R))
        return set_err(TDT_E_ARG, "width_mask must name between 1 and 8 word sizes");
    std::lock_guard<std::mutex> lk(c->mu);
    uint8_t *wsp = nullptr;
    int st = prep(c, n, s, wsp, false);
    if (st) return st;
    // the workspaces: the tables of every width, and a plan buffer per tuned width
    st = grow_retiring(c->mx_tab, c->mx_bytes, R.bytes, psy::cap_double(R.bytes, c->mx_bytes), c->retired, s);
    if (st) return st;
    AnyTiled x;  // the generic widths of the call share one workspace: a byte counter each, one pool of records
    if (R.n_generic && (st = any_tiled_begin(c, true, n, s, x))) return st;
    RouteArgs t{};
    t.v = v;
    t.ws = d_word_size;
    t.n = n;
    t.n_routes = (uint32_t)R.n_routes;
    t.status = d_status;
    t.out_len = d_out_len;
    for (int k = 0; k < R.n_routes; ++k) {
        const psy::MixedRoute &q = R.route[k];
        t.width[k] = q.ws;
        t.in_pair[k] = reinterpret_cast<ulonglong2 *>(c->mx_tab + q.pair[psy::PT_IN]);
        t.out_pair[k] = reinterpret_cast<ulonglong2 *>(c->mx_tab + q.pair[psy::PT_OUT]);
        if (!q.tuned) {
            if (!(PSY_HAVE_ANYWS)) return set_err(TDT_E_UNSUPPORTED, "this build holds no generic-width kernels");
            t.bytes[k] = x.bytes(k);
            continue;
        }
        if (!with_word_size(q.ws, [](auto) {})) return set_err(TDT_E_UNSUPPORTED, "this build holds word size 4 only");
        auto &pw = c->mx_pw[tuned_index(q.ws)];
        if (!pw) {
            if ((st = no_growth_in_capture(s))) return st;
            pw.reset(new PlanWS());
        }
        if ((st = ensure_plan(*pw, n, s))) return st;
        HIPCHK(hipMemsetAsync(pw->buf, 0, psy::kPlanSnapBytes, s));
        t.bytes[k] = reinterpret_cast<unsigned long long *>(pw->buf) + psy::EC_BYTES;
    }
    hipLaunchKernelGGL(tdt_route_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, t);
    HIPCHK(hipGetLastError());
    psy::EncodeArgs a{};
    a.n_msgs = n;
    a.status = d_status;
    a.out_len = d_out_len;
    if (mode == psy::MODE_MAPPED) a.mapping_in = reinterpret_cast<const int32_t *>(d_mapbits);
    if (mode == psy::MODE_SIZES) a.map_out = reinterpret_cast<int32_t *>(d_mapbits);
    wire_encode(c, a, wsp);
    // one width after another on the caller's stream, each tuned one forking its own side stream
    for (int k = 0; k < R.n_routes; ++k) {
        const psy::MixedRoute &q = R.route[k];
        const Routed r{reinterpret_cast<const uint64_t *>(t.in_pair[k]), reinterpret_cast<const uint64_t *>(t.out_pair[k])};
        if (q.tuned) {
            PlanWS &pw = *c->mx_pw[tuned_index(q.ws)];
            with_word_size(q.ws, [&](auto W) {
                st = mode == psy::MODE_SIZES    ? launch_slotted<W(), true, psy::MODE_SIZES>(c, pw, a, s, nullptr, &r)
                     : mode == psy::MODE_MAPPED ? launch_slotted<W(), true, psy::MODE_MAPPED>(c, pw, a, s, nullptr, &r)
                                                : launch_slotted<W(), true>(c, pw, a, s, nullptr, &r);
            });
        } else {
            psy::EncodeArgs g = a;
            g.in_off = r.in_pair;
            g.slot_off = mode == psy::MODE_SIZES ? nullptr : r.out_pair;
            st = launch_any_encode(g, q.ws, mode, s, true, x.args(k));
        }
        if (st) return st;
    }
    if ((st = any_tiled_end(c, x, n, s))) return st;
    HIPCHK(hipGetLastError());
    return TDT_OK;
}

// messages > 4 KiB: TEAM threads per message, G resident rounds per wave (64 KiB resident)
#ifndef PSY_BIG_TEAM
#define PSY_BIG_TEAM 512
#define PSY_BIG_G 8
#endif

// res: every message is aligned, a whole number of 16-byte groups and at most 64 KiB (the
// caller checked): the resident-only kernel (without the streaming body's live registers; the
// one-pass compacted C3 encode 9.58 ms with both bodies)
template <int WS, int MODE, int LB>
int launch_encode_ws(psy::EncodeArgs a, bool small, bool res, hipStream_t s) {
    if (small) return launch_encode_t<WS, 64, 4, MODE, LB>(a, s);
    if constexpr (MODE == psy::MODE_ENCODE && LB == 1 && PSY_BIG_TEAM == 512 && PSY_BIG_G == 8)
        if (res) return launch_encode_t<WS, 512, 8, MODE, LB, psy::PATH_RES>(a, s);
    return launch_encode_t<WS, PSY_BIG_TEAM, PSY_BIG_G, MODE, LB>(a, s);
}

// LB: compacted output (look-back) vs slotted output
// Team shape of a one-pass (look-back) launch when the caller does not know the batch's sizes:
// one-wave teams when most messages of this context's latest slotted plan were small (<= 4 KiB),
// the size hint only before any plan has been observed.
bool lb_small_teams(tdt_ctx *c, hipStream_t s) {
    auto &H = c->pw.eh;
    if (!capturing(s)) H.refresh();
    if (H.valid && H.n) return 2ull * ((uint64_t)H[psy::EC_SMALL_ALL] + H[psy::EC_UNCP_ALL]) > H.n;
    return c->size_hint.load() <= kSmallMax;
}

// small_teams: -1 from the context's history, 0 message-sized teams, 1 one-wave teams, 2
// message-sized resident-only teams (see launch_encode_ws)
// own: the call holds the context's lock (any_tiled_begin)
template <int MODE, int LB>
int launch_encode(tdt_ctx *c, psy::EncodeArgs a, hipStream_t s, int small_teams, bool own = false) {
    const bool small = small_teams < 0 ? lb_small_teams(c, s) : small_teams == 1;
    const bool res = small_teams == 2;
    int st = TDT_OK;
    if (with_word_size(c->cfg.word_size, [&](auto W) { st = launch_encode_ws<W(), MODE, LB>(a, small, res, s); }))
        return st;
    // generic widths: analysis, or a blob into its slot (the compacted entry points take the
    // two-phase route, encode_two_phase_any)
    if (MODE != psy::MODE_ANALYZE && !a.slot_off && psy::anyws_generic(c->cfg.word_size))
        return set_err(TDT_E_UNSUPPORTED, "compacted one-pass encode needs word_size 1, 2, 4, 8 or 16");
    AnyTiled x;
    if (MODE != psy::MODE_ANALYZE && psy::anyws_generic(c->cfg.word_size) && (st = any_tiled_begin(c, own, a.n_msgs, s, x)))
        return st;
    st = launch_any_encode(a, c->cfg.word_size, MODE, s, false, x.args());
    return st ? st : any_tiled_end(c, x, a.n_msgs, s);
}

// Zero the counters + look-back words of a batch; `wsp` = an explicit workspace (host
// pipeline slots) or null for the context's own.  Slotted batches (no look-back, message id =
// block index) only need the counter block for the error flags, zeroed once per context.
int prep(tdt_ctx *c, uint32_t n_msgs, hipStream_t s, uint8_t *&wsp, bool lookback = true) {
    HIPCHK(hipSetDevice(c->device));
    if (!wsp) {
        const bool fresh = c->ws == nullptr;
        int st = ensure_ws(c, lookback ? n_msgs : 0, s);
        if (st) return st;
        wsp = c->ws;
        if (!lookback) {
            if (fresh) HIPCHK(hipMemsetAsync(wsp, 0, kCounterBytes, s));
            return TDT_OK;
        }
    } else if (!lookback) {
        HIPCHK(hipMemsetAsync(wsp, 0, kCounterBytes, s));  // pipeline chunk: fresh error flags
        return TDT_OK;
    }
    HIPCHK(hipMemsetAsync(wsp, 0, kCounterBytes + 8ull * n_msgs, s));
    return TDT_OK;
}

int encode_common(tdt_ctx *c, int mode, psy::EncodeArgs a, const Where &w) {
    const Scatter *v = w.v;
    if (!c) return set_err(TDT_E_ARG, "null context");
    if (a.n_msgs == 0) return TDT_OK;
    if (v && !(v->ptr && v->size && v->out_ptr && v->out_cap)) return set_err(TDT_E_ARG, "null pointer or size array");
    if (!v && !a.in_off) return set_err(TDT_E_ARG, "null input offsets");  // a.in may be null: all-empty batch
    const bool slotted = a.slot_off != nullptr || v;
    if (!v && mode != psy::MODE_ANALYZE && (!a.out || (!slotted && !a.out_off))) return set_err(TDT_E_ARG, "null output");
    if (mode == psy::MODE_MAPPED && !a.mapping_in) return set_err(TDT_E_ARG, "null mapping");
    hipStream_t s = w.stream;
    std::unique_lock<std::mutex> lk(c->mu, std::defer_lock);
    uint8_t *wsp = w.wsp;
    if (!wsp) lk.lock();  // pipeline slots own their workspace
    int st = prep(c, a.n_msgs, s, wsp, !slotted);
    if (st) return st;
    wire_encode(c, a, wsp);
    if (mode == psy::MODE_ENCODE) {
        st = slotted ? launch_slotted_any(c, w.pws ? *w.pws : c->pw, a, s, v)
                     : launch_encode<psy::MODE_ENCODE, 1>(c, a, s, w.small_teams, !w.wsp);
    } else if (mode == psy::MODE_MAPPED) {
        st = v ? launch_slotted_any(c, w.pws ? *w.pws : c->pw, a, s, v, true)
               : launch_encode<psy::MODE_MAPPED, 1>(c, a, s, w.small_teams, !w.wsp);
    } else {
        st = launch_encode<psy::MODE_ANALYZE, 1>(c, a, s, w.small_teams);
    }
    if (st) return st;
    HIPCHK(hipGetLastError());
    return TDT_OK;
}

// The size pass at the context's width (tdt_encoded_sizes_batch / _v): d_enc[i] and d_status[i] are
// what the scattered encode reports for a slot of the encode bound.  One of `v` (scattered: ptr and
// size; there are no outputs, and out_ptr / out_cap name the size array, see launch_slotted) and `g`
// (contiguous) names the batch.  The plan workspace and count history are the encode's own: both
// passes plan the same batch into the same lists.
// d_mapbits (optional, n u64): the mapping bits of every compressed message (tdt_mappings_v).
int encoded_sizes_one(tdt_ctx *c, const Scatter *v, const Contig *g, uint32_t n, uint64_t *d_enc, int32_t *d_status,
                      hipStream_t s, uint64_t *d_mapbits = nullptr) {
    if (!c) return set_err(TDT_E_ARG, "null context");
    if (n == 0) return TDT_OK;
    if (!d_enc || (v && !(v->ptr && v->size)) || (g && !g->off)) return set_err(TDT_E_ARG, "null pointer, size or output array");
    std::lock_guard<std::mutex> lk(c->mu);
    uint8_t *wsp = nullptr;
    int st = prep(c, n, s, wsp, false);
    if (st) return st;
    psy::EncodeArgs a{};
    a.n_msgs = n;
    a.status = d_status;
    a.out_len = d_enc;
    a.map_out = reinterpret_cast<int32_t *>(d_mapbits);
    wire_encode(c, a, wsp);
    if (!with_word_size(c->cfg.word_size, [&](auto W) {
            st = launch_slotted<W(), true, psy::MODE_SIZES>(c, c->pw, a, s, v, nullptr, g);
        })) {
        // generic widths: one workgroup per message, no plan (the plan buffer holds the input table alone)
        if (!psy::anyws_generic(c->cfg.word_size)) return set_err(TDT_E_UNSUPPORTED, "word_size not supported on the GPU path");
        AnyTiled x;
        if ((st = any_tiled_begin(c, true, n, s, x))) return st;
        if ((st = ensure_plan(c->pw, n, s, true))) return st;
        st = g ? launch_offsets_table(c->pw, *g, n, x.bytes(), a.in_off, s)
               : launch_table(c->pw, *v, n, true, x.bytes(), a.in_off, a.slot_off, s);
        if (st) return st;
        a.slot_off = nullptr;
        st = launch_any_encode(a, c->cfg.word_size, psy::MODE_SIZES, s, true, x.args());
        if (!st) st = any_tiled_end(c, x, n, s);
    }
    if (st) return st;
    HIPCHK(hipGetLastError());
    return TDT_OK;
}

// Slotted decode: a plan kernel separates the large blobs (decoded size > large_min and
// > 1/4096 of the batch) and the blobs decoding to <= 1 KiB from the rest; the rest decode one
// wave each, the small ones one wave each with one-round windows, the large ones through the
// prep / block / scan / tile passes (tdt_decode.h).  As for encode, the list lengths stay on
// the device: main grids from an earlier call's counts, overflow launches past them.
constexpr uint32_t kDLmax = 1u << 16, kDBcap = 1u << 23, kDTcap = 1u << 20;  // full budgets
constexpr uint32_t kDL0 = 1024, kDB0 = 1u << 16, kDT0 = 8192;                 // starting budgets
// the large-blob records (PlanWS::dlarge): DMeta | block entries | block sums | tile entries | tile
// blocks (two per tile), as byte offsets
struct DLargeLayout { size_t bent, bsum, tent, tblk, bytes; };  // (DMeta at 0)
DLargeLayout dlarge_layout(uint32_t lcap, uint32_t bcap, uint32_t tcap) {
    const size_t bent = (size_t)lcap * sizeof(psy::DMeta), bsum = bent + 4ull * bcap, tent = bsum + 4ull * bcap,
                 tblk = tent + 4ull * tcap;
    return {bent, bsum, tent, tblk, tblk + 8ull * tcap};
}

int ensure_dlarge(PlanWS &w) {
    uint32_t lc = w.d_lcap ? w.d_lcap : kDL0, bc = w.d_bcap ? w.d_bcap : kDB0, tc = w.d_tcap ? w.d_tcap : kDT0;
    if (w.dh.valid) {
        lc = std::max(lc, pow2_at_least(w.dh[psy::DC_LARGE], kDL0, kDLmax));
        tc = std::max(tc, pow2_at_least(w.dh[psy::DC_TILES], kDT0, kDTcap));
        bc = std::max(bc, pow2_at_least(w.dh[psy::DC_BLOCKS], kDB0, kDBcap));
    }
    if (w.dlarge && lc == w.d_lcap && bc == w.d_bcap && tc == w.d_tcap) return TDT_OK;
    if (w.dlarge) {
        w.retired.push_back(w.dlarge);  // (as ensure_elarge)
        w.dlarge = nullptr;
        w.d_lcap = w.d_bcap = w.d_tcap = 0;
    }
    HIPCHK(hipMalloc(&w.dlarge, dlarge_layout(lc, bc, tc).bytes));
    w.d_lcap = lc;
    w.d_bcap = bc;
    w.d_tcap = tc;
    return TDT_OK;
}

// PAIR: a scattered batch (`v`): its slot table first, then the same classes through the PAIR instances
template <bool PAIR = false>
int launch_decode_slotted(tdt_ctx *c, PlanWS &pw, psy::DecodeArgs a, hipStream_t s, const Scatter *v = nullptr) {
    using namespace psy;  // (counter, list and kernel names)
    const uint32_t n = a.n_msgs;
    if (PAIR != (v != nullptr)) return set_err(TDT_E_ARG, "scattered launch without its arrays");
    int st = ensure_plan(pw, n, s, PAIR);
    if (st) return st;
    const bool capturing = ::capturing(s);
    auto &H = pw.dh;
    if (!capturing) H.refresh();
    const bool small_on = !H.valid || H[DC_SMALL_ALL] > 0;
    const bool copy_on = !H.valid || H[DC_UNCP_ALL] > 0;
    bool large_on = !H.valid || H[DC_LARGE] > 0;
    if (large_on && !capturing) {
        st = ensure_dlarge(pw);
        if (st) return st;
    }
    large_on = large_on && pw.dlarge;
    auto *cnt = reinterpret_cast<unsigned long long *>(pw.buf);
    auto *cnt32 = reinterpret_cast<uint32_t *>(pw.buf);
    const PlanLayout PL = plan_layout(n);
    auto list = [&](DecList l) { return reinterpret_cast<uint32_t *>(pw.buf + PL.list[l]); };
#if PSY_HAVE_ANYWS
    // the deferred-blob list (generic word sizes): the plan buffer's fifth list and last counter
    a.dlist = list(DL_DEFERRED);
    a.dcount = cnt32 + lo32(DC_DEFERRED);
#endif
    const uint32_t lcap = large_on ? pw.d_lcap : 0u, bcap = large_on ? pw.d_bcap : 0u,
                   tcap = large_on ? pw.d_tcap : 0u;
    const DLargeLayout DL = dlarge_layout(pw.d_lcap, pw.d_bcap, pw.d_tcap);
    a.dmeta = reinterpret_cast<DMeta *>(pw.dlarge);
    auto *bent = reinterpret_cast<uint32_t *>(pw.dlarge + DL.bent);
    auto *tent = reinterpret_cast<uint32_t *>(pw.dlarge + DL.tent);
    HIPCHK(hipMemsetAsync(cnt, 0, kPlanSnapBytes, s));
    if constexpr (PAIR) {  // the blobs through in_off / in_len as they are, the slots through a pair table
        const uint64_t *none = nullptr;
        if ((st = launch_table(pw, *v, n, false, cnt + DC_BYTES, none, a.slot_off, s))) return st;
    }
    DPlanArgs p{a.in, a.in_off, a.in_len, n, cnt, list(DL_MAIN), list(DL_SMALL), c->dsmall_max, list(DL_BIG), c->dbig_min,
                list(DL_COPY), a.dmeta, bent, tent, lcap, bcap, tcap, c->large_min, small_on ? 1u : 0u, copy_on ? 1u : 0u};
    hipLaunchKernelGGL(tdt_decode_plan_kernel<PAIR>, dim3((uint32_t)(((uint64_t)n + 4095) / 4096)), dim3(1024), 0, s, p);
    HIPCHK(hipGetLastError());
    if (!capturing && (st = record_counts(H, cnt, n, s))) return st;
    a.bent = bent;
    a.bsum = reinterpret_cast<uint32_t *>(pw.dlarge + DL.bsum);
    a.tent = tent;
    a.tblk = reinterpret_cast<uint32_t *>(pw.dlarge + DL.tblk);
    a.pcnt = cnt32;
    a.lcap = lcap;
    a.bcap = bcap;
    a.tcap = tcap;
    const uint32_t ovf = (uint32_t)c->cus * 32;
    const ClassLaunch<DecodeArgs> cls{a, cnt32};
    bool forked = false;
    hipStream_t ts = s;
    // the side stream carries the large-blob pipeline and the small-blob list beside the main
    // list (the small list queued behind the main list ran alone in its tail: C4 1.6 ms)
    const bool main_on = !H.valid || H[DC_MAIN] + H[DC_BIG] > 0;
    if (large_on || ((small_on || copy_on) && main_on && !c->small_main)) {
        const int fr = c->no_side || pw.no_side ? -1 : fork_side(pw, s);
        if (fr > 0) return fr;
        forked = fr == TDT_OK;
        if (forked) ts = pw.side;
    }
    if (large_on) {
        const uint32_t gl = std::max(1u, std::min(lcap, 1024u));
        hipLaunchKernelGGL(tdt_decode_lprep_kernel<PAIR>, dim3(gl), dim3(256), 0, ts, a);
        hipLaunchKernelGGL(tdt_decode_lblock_kernel, dim3(std::max(1u, std::min((bcap + 3) / 4, ovf / 4))), dim3(256), 0,
                           ts, a);
        hipLaunchKernelGGL(tdt_decode_lscan_kernel, dim3(gl, 2), dim3(64), 0, ts, a);
        // (the tile entries are large-blob records, not a list; no main launch before any count is known)
        cls(nullptr, DC_TILES, guess(H, DC_TILES, tcap, 0), tcap, 64, ovf, ts, tdt_decode_ltile_kernel<0>,
            tdt_decode_ltile_kernel<1>);
    }
    // the main list (one wave per blob), its kernels taking the big list's blobs first
    a.blist = list(DL_BIG);
    a.blist_count = cnt32 + lo32(DC_BIG);
    cls(list(DL_MAIN), DC_MAIN, (uint32_t)std::min<uint64_t>(n, (uint64_t)guess(H, DC_MAIN, n, n) + guess(H, DC_BIG, n, n)),
        n, 64, ovf, s, tdt_decode_kernel<0, kDecWR, 0, PAIR>, tdt_decode_kernel<0, kDecWR, 1, PAIR>);
    a.blist = nullptr;
    const hipStream_t ss = forked && !c->small_main ? pw.side : s;
    // passthrough copies beside the main list
    if (copy_on) {
        a.list = list(DL_COPY);
        a.list_count = cnt32 + lo32(DC_UNCP);
        hipLaunchKernelGGL(tdt_decode_copy_kernel<PAIR>, dim3(std::max(1u, std::min((uint32_t)c->cus * c->copy_wgs, (n + 15) / 16))),
                           dim3(256), 0, ss, a);
    }
    // small blobs: one-round windows (a third less LDS per wave: more blobs in flight per CU)
    if (small_on)
        cls(list(DL_SMALL), DC_SMALL, guess(H, DC_SMALL, n, n), n, 64, ovf, ss, tdt_decode_kernel<0, 1, 0, PAIR>,
            tdt_decode_kernel<0, 1, 1, PAIR>);
    if (forked && (st = join_side(pw, s))) return st;
    // the deferred blobs (generic word sizes): near-empty when no kernel above listed one.  (A
    // fixed grid: the plan's count snapshot is taken before the class kernels append to the list,
    // so the history cannot size it — 64 workgroups for 4,096 listed blobs ran at a twelfth of the rate.)
    return decode_deferred(c, &pw == &c->pw, a, s, PAIR, cnt + DC_BYTES);
}

int decode_common(tdt_ctx *c, bool sizes_only, psy::DecodeArgs a, const Where &w) {
    const Scatter *v = w.v;
    const uint32_t n_msgs = a.n_msgs;
    if (!c) return set_err(TDT_E_ARG, "null context");
    if (n_msgs == 0) return TDT_OK;
    if (v && !(v->ptr && v->size && v->out_ptr && v->out_cap)) return set_err(TDT_E_ARG, "null pointer or size array");
    if (!a.in_off) return set_err(TDT_E_ARG, "null input offsets");
    const bool slotted = a.slot_off != nullptr || v;  // (a scattered batch: in_off / in_len are its blobs)
    if (!sizes_only && !slotted && !a.out_off) return set_err(TDT_E_ARG, "null output offsets");
    if (sizes_only && !a.sizes_out) return set_err(TDT_E_ARG, "null sizes");
    hipStream_t s = w.stream;
    std::unique_lock<std::mutex> lk(c->mu, std::defer_lock);
    uint8_t *wsp = w.wsp;
    if (!wsp) lk.lock();
    const bool lookback = !(slotted || sizes_only);
    int st = prep(c, n_msgs, s, wsp, lookback);
    if (st) return st;
    wire_decode(a, wsp, lookback);
    if (sizes_only) {
        hipLaunchKernelGGL(psy::tdt_decode_sizes_kernel, dim3((n_msgs + 255) / 256), dim3(256), 0, s, a);
    } else if (slotted) {
        st = v ? launch_decode_slotted<true>(c, w.pws ? *w.pws : c->pw, a, s, v)
               : launch_decode_slotted(c, w.pws ? *w.pws : c->pw, a, s);
        if (st) return st;
    } else {
        launch_list(n_msgs, 64, [&](uint32_t, uint32_t g) {  // ids from the ticket
            hipLaunchKernelGGL((psy::tdt_decode_kernel<1>), dim3(g), dim3(64), 0, s, a);
        });
        st = decode_deferred(c, lk.owns_lock(), a, s);
        if (st) return st;
    }
    HIPCHK(hipGetLastError());
    return TDT_OK;
}

int ensure_host_dev(tdt_ctx *c, size_t bytes) {
    return psy::grow(c->h_dev, c->h_dev_bytes, bytes, psy::cap_double(bytes, c->h_dev_bytes), dev_free, DevAlloc{});
}

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---------------------------------------------------------------------------------------
// Host pipeline (the TCP socket-buffer case: SimpleTCP sends from and receives into host
// memory, tcp_simple.hpp:68-91, :153-194).  The batch is cut into chunks of whole messages
// (<= kHostChunk input bytes); chunk c runs on slot c % kHostSlots — its own stream, device
// buffer, plan workspace and pinned buffers — as H2D → batch kernels → D2H, and the host finishes
// chunk c - 3 (its output) while chunks c - 2 .. c are on the GPU: with two slots the next H2D
// waited for the D2H of the chunk before (the pinned 50 x 1 MiB decode moved its bytes one PCIe
// direction at a time: 22.6 GB/s, profiles/r04_hp1).  Caller buffers that are not pinned
// (std::vector socket buffers, numpy arrays) are staged through the slot's pinned buffers by a
// pool of host threads (parallel memcpy: one thread's memcpy is far below the PCIe rate);
// pinned caller buffers are DMA'd directly.  Every device → host copy lands in pinned memory,
// so no copy blocks the host behind the kernels.
constexpr uint64_t kHostChunk = 64ull << 20;

bool is_pinned(const void *p) {
    hipPointerAttribute_t at{};
    if (!p || hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

int ensure_slot(tdt_ctx *c, int k, size_t dev_bytes, size_t pin_words, size_t sin, size_t sout) {
    auto &h = c->hs[k];
    if (!c->hin) {
        HIPCHK(hipStreamCreateWithFlags(&c->hin, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&c->hex, hipStreamNonBlocking));
    }
    if (!h.stream) {
        h.pw.no_side = true;
        HIPCHK(hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&h.ev, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h.evc, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h.evi, hipEventDisableTiming));
        HIPCHK(hipHostMalloc(&h.flag, 4, hipHostMallocDefault));
        *h.flag = 0;
    }
    // growth takes 1.5x (whole MiB, psy::cap_slot) and retires the old buffer until tdt_ctx_destroy
    // instead of freeing it: a hipFree waits for the whole device (every stream, the other contexts'
    // of the process too: a C1 loopback end stalled the other end's pipeline for milliseconds), and
    // pinning host memory costs milliseconds
    int st = psy::grow(h.dev, h.dev_bytes, dev_bytes, psy::cap_slot(dev_bytes, h.dev_bytes), retire_to(c->retired),
                       DevAlloc{});  // (the slot's earlier chunks are done: synced)
    if (st) return st;
    auto pinned = [&](auto *&buf, size_t &have, size_t need, size_t unit) {
        return psy::grow(buf, have, need, psy::cap_slot(unit * need, unit * have) / unit, retire_to(c->retired_host),
                         PinAlloc{unit});
    };
    if ((st = pinned(h.pin, h.pin_words, pin_words, 8)) || (st = pinned(h.stage_in, h.sin_bytes, sin, 1)) ||
        (st = pinned(h.stage_out, h.sout_bytes, sout, 1)))
        return st;
    return TDT_OK;
}

// every host-pipeline stream idle (an error mid-pipeline: copies and kernels may still touch the
// caller's buffers)
void drain_host(tdt_ctx *c) {
    for (auto &h : c->hs)
        if (h.stream) (void)hipStreamSynchronize(h.stream);
    if (c->hin) (void)hipStreamSynchronize(c->hin);
    if (c->hex) (void)hipStreamSynchronize(c->hex);
}

// Once a slot's last chunk is done: fold its device error flags into the context.
int sync_slot(tdt_ctx *c, tdt_ctx::HostSlot &h) {
    // (the slot's last command is its chunk's h.ev record; never recorded: complete)
    HIPCHK(c->slot_streams ? hipStreamSynchronize(h.stream) : hipEventSynchronize(h.ev));
    if (h.flag) {
        c->host_flags.fetch_or(*h.flag);
        *h.flag = 0;
    }
    return TDT_OK;
}

struct Chunk {
    uint32_t m0 = 0, n = 0;
    uint64_t in_bytes = 0, cap = 0, base = 0;
    uint64_t scap = 0;  // encode through the slotted kernels: the blobs' slot bytes (Σ bounds)
    // encode under TDT_OPT_HOST_RAW_FALLBACK: slots of n + 4 (always slotted), and the flag pass's words —
    // the chunk's count behind out_off, a flag per message in front of the slot buffer
    bool raw = false;
    // device layout: input | in_off (n+1), slots (n+1) | out (cap) | out_off (n+1) [raw: | count] | status (n)
    // | workspace | lengths (n) [raw: | flags (n u32)] | slotted blobs (scap)
    size_t o_off = 0, o_out = 0, o_ooff = 0, o_st = 0, o_ws = 0, o_len = 0, o_rf = 0, o_sbuf = 0, end = 0;
};

// Chunk size of a call: an eighth of its input (with four slots in flight the H2D of later
// chunks, the kernels of one and the D2H of earlier ones overlap even for a socket-sized batch
// of tens of MiB), between 2 and 64 MiB.
uint64_t host_chunk_bytes(const uint64_t *h_in_off, uint32_t n_msgs) {
    const uint64_t total = h_in_off[n_msgs] - h_in_off[0];
    return std::min<uint64_t>(kHostChunk, std::max<uint64_t>(2ull << 20, (total / 8 + 4095) & ~4095ull));
}

Chunk plan_chunk(const uint64_t *h_in_off, uint32_t m0, uint32_t n_msgs, bool encode, bool slotted, int ws,
                 const uint64_t *dec_sizes, uint64_t chunk_bytes, bool raw = false) {
    Chunk k;
    k.m0 = m0;
    k.raw = raw;
    uint32_t m = m0;
    uint64_t cap = 0;
    while (m < n_msgs) {
        const uint64_t len = h_in_off[m + 1] - h_in_off[m];
        if (m > m0 && h_in_off[m + 1] - h_in_off[m0] > chunk_bytes) break;
        cap += !encode ? dec_sizes[m] : raw ? psy::raw_blob_bytes(len) : tdt_encode_bound(len, ws);
        ++m;
    }
    k.n = m - m0;
    k.in_bytes = h_in_off[m] - h_in_off[m0];
    k.cap = cap;
    k.scap = encode && slotted ? cap : 0;
    k.o_off = align_up(k.in_bytes, 256);
    k.o_out = align_up(k.o_off + 16ull * (k.n + 1), 256);
    // (the slotted encode writes its blobs into the slot buffer at o_sbuf: no compacted region)
    k.o_ooff = align_up(k.o_out + (k.scap ? 1ull : std::max<uint64_t>(cap, 1)), 256);
    k.o_st = align_up(k.o_ooff + 8ull * (k.n + 1 + (raw ? 1 : 0)), 256);
    k.o_ws = align_up(k.o_st + 4ull * k.n, 256);
    k.o_len = align_up(k.o_ws + kCounterBytes + 8ull * (k.n + 1), 256);
    k.o_rf = align_up(k.o_len + 8ull * k.n, 256);
    k.o_sbuf = align_up(k.o_rf + (raw ? 4ull * k.n : 0), 256);
    k.end = k.o_sbuf + (k.scap ? k.scap + 16 : 0);  // (+16: more than the gather's copy needs — the over-read rule, tdt_copy.h)
    return k;
}

size_t chunk_dev_bytes(const Chunk &k) { return k.end; }
// pinned words of a slot: in_off (n+1) | slots (n+1) | out_off or lengths (n+1) [raw: | count] | status (n int32)
size_t chunk_back_words(const Chunk &k) { return (size_t)k.n + 1 + (k.raw ? 1 : 0); }
size_t chunk_pin_words(const Chunk &k) { return 2ull * k.n + 2 + chunk_back_words(k) + (k.n + 1) / 2; }
uint64_t *pin_slots(tdt_ctx::HostSlot &h, const Chunk &k) { return h.pin + (k.n + 1); }
uint64_t *pin_back(tdt_ctx::HostSlot &h, const Chunk &k) { return h.pin + 2ull * (k.n + 1); }
int32_t *pin_status(tdt_ctx::HostSlot &h, const Chunk &k) {
    return reinterpret_cast<int32_t *>(h.pin + 2ull * k.n + 2 + chunk_back_words(k));
}

// decode: the decoded size of every blob from its header (the kernel validates; a blob it
// rejects gets 0 and its bytes are dropped when the output is compacted)
uint64_t host_decoded_size(const uint8_t *b, uint64_t len) {
    if (len < 4) return 0;
    uint32_t magic;
    std::memcpy(&magic, b, 4);
    if (magic == psy::kMagicUNCP) return len - 4;
    if (magic != psy::kMagicTDT || len < 8) return 0;
    uint32_t orig;
    std::memcpy(&orig, b + 4, 4);
    return orig;
}

// Chunk ci's compacted output → host memory, issued behind the encode kernel so that no host
// wait sits between a chunk's kernel and its copy (the length is device-side: the chunk's last
// offset).  dst: the slot's pinned staging (direct = 0), or the caller's pinned buffer at the
// running base (direct = 1; bases[ci] = the totals of the chunks before, written by the previous
// chunk's launch, which this one follows by an event).  Past out_cap nothing is copied (the host
// reports TDT_E_CAPACITY).
// total bytes src → d (mapped host memory over PCIe, or device) by the whole grid of 256-lane
// workgroups: the shared copy (tdt_copy.h) with generic stores.  src is a chunk's device buffer at
// both call sites (d + k.o_out of host_encode and of host_decode), so its loads are global ones;
// what it reads beyond src + total is the over-read rule's, inside the buffer's 256-byte alignment.
__device__ __forceinline__ void grid_copy_out(uint8_t *d, const uint8_t *src, uint64_t total) {
    psy::copy_shifted<1, false>(d, src, total, (uint64_t)blockIdx.x * 256 + threadIdx.x, (uint64_t)gridDim.x * 256);
}

__global__ __launch_bounds__(256) void host_out_kernel(const uint8_t *src, const uint64_t *chunk_off, uint32_t n,
                                                       uint8_t *dst, uint64_t *bases, uint32_t ci, uint64_t cap,
                                                       int direct) {
    const uint64_t total = chunk_off[n];
    const uint64_t base = bases[ci];
    if (blockIdx.x == 0 && threadIdx.x == 0) bases[ci + 1] = base + total;
    if (base + total > cap || total == 0) return;
    grid_copy_out(direct ? dst + base : dst, src, total);
}

// host_decode: a chunk's slotted output → the caller's pinned buffer (or the pinned staging)
__global__ __launch_bounds__(256) void host_dout_kernel(const uint8_t *src, uint8_t *dst, uint64_t total) {
    grid_copy_out(dst, src, total);
}

// A slotted chunk's blob lengths → exclusive offsets (total at [n]): one workgroup, 4096
// lengths per step (a chunk holds at most kHostChunk bytes of messages).
__global__ __launch_bounds__(1024) void host_scan_kernel(const uint64_t *len, uint64_t *out_off, uint32_t n) {
    __shared__ uint64_t wsum[16];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint64_t carry = 0;
    for (uint32_t b = 0; b < n; b += 4096) {
        uint64_t v[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = b + 4u * (uint32_t)t + (uint32_t)k;
            v[k] = i < n ? len[i] : 0ull;
            s += v[k];
        }
        uint64_t x = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        uint64_t pre = carry, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const uint64_t q = wsum[w];
            pre += w < wv ? q : 0ull;
            tot += q;
        }
        uint64_t e = pre + x - s;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = b + 4u * (uint32_t)t + (uint32_t)k;
            if (i < n) out_off[i] = e;
            e += v[k];
        }
        carry += tot;
        __syncthreads();  // wsum is reused
    }
    if (t == 0) out_off[n] = carry;
}

// A slotted chunk's blobs → host memory at their compacted places (the output copy of
// host_out_kernel, gathering from the slots): P waves per blob, each a contiguous part; the
// running base is chained as there.  A wave's part goes through the shared copy (tdt_copy.h): compacted
// offsets have any alignment, so a byte loop would be the common case otherwise.  src is the chunk's
// slot buffer on the device (d + k.o_sbuf).
__global__ __launch_bounds__(256) void host_gather_kernel(const uint8_t *src, const uint64_t *slot, const uint64_t *len,
                                                          const uint64_t *out_off, uint32_t n, uint32_t P, uint8_t *dst,
                                                          uint64_t *bases, uint32_t ci, uint64_t cap, int direct) {
    const uint64_t total = out_off[n];
    const uint64_t base = bases[ci];
    if (blockIdx.x == 0 && threadIdx.x == 0) bases[ci + 1] = base + total;
    if (base + total > cap || total == 0) return;
    uint8_t *d = direct ? dst + base : dst;
    const uint64_t nw = (uint64_t)n * P;
    for (uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nw; w += (uint64_t)gridDim.x * 4) {
        const uint32_t i = (uint32_t)(w / P), p = (uint32_t)(w % P);
        const uint64_t l = len[i], a = l * p / P, e = l * (p + 1) / P;
        if (e > a) psy::copy_shifted<1, false>(d + out_off[i] + a, src + slot[i] + a, e - a, threadIdx.x & 63u, 64);
    }
}

// TDT_OPT_HOST_RAW_FALLBACK: the flag pass behind a chunk's slotted encode into slots of n + 4 bytes.
// One workgroup striding over the chunk's messages, one lane per message at a time, as the scan that
// follows it: so the chunk's count is a plain sum with no word to clear first.  The decision is
// tdt_rawfb.h's; a flagged message gets its final status and length here, flag[i] says where the gather
// takes blob i from, and *count is the chunk's share of TDT_STAT_HOST_RAW_FALLBACKS.
__global__ __launch_bounds__(1024) void host_raw_flag_kernel(const uint64_t *in_off, const uint64_t *slot, int32_t *status,
                                                             uint64_t *len, uint32_t *flag, uint64_t *count, uint32_t n) {
    __shared__ uint32_t wsum[16];
    uint32_t mine = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 1024) {
        const uint64_t sz = in_off[i + 1] - in_off[i];
        const bool f = psy::raw_flagged(status[i], len[i], sz, slot[i + 1] - slot[i]);
        if (f) {
            status[i] = TDT_OK;
            len[i] = psy::raw_blob_bytes(sz);
        }
        flag[i] = f ? 1u : 0u;
        mine += f ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_down(mine, d);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t tot = 0;
        for (int w = 0; w < 16; ++w) tot += wsum[w];
        *count = tot;
    }
}

// host_gather_kernel under TDT_OPT_HOST_RAW_FALLBACK: the same P waves per blob, running base and
// `direct` handling, with the source chosen per blob.  An unflagged blob comes from its slot.  A flagged
// one was never written there: a wave's part [a, e) of its n + 4 bytes is tdt_rawfb.h's raw_span — marker
// bytes from raw_marker_byte, and payload bytes straight from the chunk's input at in + in_off[i].  That
// source obeys the copy's over-read rule (tdt_copy.h) inside the chunk buffer: the input starts the
// buffer, and the offset tables follow it.
__global__ __launch_bounds__(256) void host_raw_gather_kernel(const uint8_t *in, const uint64_t *in_off, const uint8_t *src,
                                                              const uint64_t *slot, const uint64_t *len,
                                                              const uint32_t *flag, const uint64_t *out_off, uint32_t n,
                                                              uint32_t P, uint8_t *dst, uint64_t *bases, uint32_t ci,
                                                              uint64_t cap, int direct) {
    const uint64_t total = out_off[n];
    const uint64_t base = bases[ci];
    if (blockIdx.x == 0 && threadIdx.x == 0) bases[ci + 1] = base + total;
    if (base + total > cap || total == 0) return;
    uint8_t *d = direct ? dst + base : dst;
    const uint64_t nw = (uint64_t)n * P;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nw; w += (uint64_t)gridDim.x * 4) {
        const uint32_t i = (uint32_t)(w / P), p = (uint32_t)(w % P);
        const uint64_t l = len[i], a = l * p / P, e = l * (p + 1) / P;
        if (e <= a) continue;
        uint8_t *o = d + out_off[i];
        if (!flag[i]) {
            psy::copy_shifted<1, false>(o + a, src + slot[i] + a, e - a, lane, 64);
            continue;
        }
        const psy::RawSeg s = psy::raw_span(a, e);
        if (lane < s.marker_n) o[s.marker_at + lane] = psy::raw_marker_byte(s.marker_at + lane);
        if (s.len) psy::copy_shifted<1, false>(o + s.dst_off, in + in_off[i] + s.src_off, s.len, lane, 64);
    }
}

// The issue / finish loop of a host call: chunk ci is issued on slot ci % kHostSlots once that
// slot's previous chunk is done, and finished (its outputs and statuses read back) kHostSlots - 1
// chunks later, so that up to kHostSlots chunks are in flight.
template <class I, class F>
int host_loop(size_t nc, I &&issue, F &&finish) {
    constexpr size_t L = kHostSlots - 1;
    for (size_t ci = 0; ci < nc; ++ci) {
        int st = issue(ci);
        if (!st && ci >= L) st = finish(ci - L);
        if (st) return st;
    }
    for (size_t ci = nc > L ? nc - L : 0; ci < nc; ++ci)
        if (int st = finish(ci)) return st;
    return TDT_OK;
}

// A host call's input: one buffer with offsets, or (msgs / sizes: gather input, tdt_encode_host_v)
// message i = msgs[i][0 .. sizes[i]), h_in then unused and h_in_off the prefix sums of sizes.
// direct: the caller's memory is pinned and DMA'd as it is, not staged by the copy pool.
struct HostIn {
    const uint8_t *h_in;
    const uint64_t *h_in_off;
    const uint8_t *const *msgs;
    const uint64_t *sizes;
    bool direct;
};
// What a chunk's issue works with once its prologue is done
struct ChunkView {
    uint64_t *doff, *dslot, *dooff, *dlen;  // device: in_off, slots, out_off, lengths
    int32_t *dst;                           // device: statuses
    const uint8_t *src;        // the chunk's input in pinned memory (null: pinned gather input, copied run by run)
    uint64_t slot_bytes;       // Σ slot sizes (0 without a slot table)
    hipStream_t s_in, s_ex;    // the input copies' stream, the kernels' and read-backs' stream
};
// The prologue of a chunk's issue, encode and decode alike: the slot's buffers (stage_out bytes:
// `sout`), the wait for the slot's previous chunk, the pinned offset table and — slots — the slot
// table (slot_size(i): message i's slot, the encode bound or the decoded size), the staged input,
// the chunk's device pointers and its two streams.
template <class SlotSize>
int chunk_prologue(tdt_ctx *c, const Chunk &k, size_t ci, const HostIn &in, size_t sout, bool slots, SlotSize &&slot_size,
                   ChunkView &v) {
    const int si = (int)(ci % kHostSlots);
    auto &h = c->hs[si];
    int st = ensure_slot(c, si, chunk_dev_bytes(k), chunk_pin_words(k), in.direct ? 0 : k.in_bytes, sout);
    if (st || (st = sync_slot(c, h))) return st;  // (the slot's previous chunk is done with its buffers)
    uint64_t *pin_in_off = h.pin, *pin_slot = pin_slots(h, k);
    const uint64_t b0 = in.h_in_off[k.m0];
    uint64_t acc = 0;
    for (uint32_t i = 0; i <= k.n; ++i) {
        pin_in_off[i] = in.h_in_off[k.m0 + i] - b0;
        if (slots) {
            pin_slot[i] = acc;
            if (i < k.n) acc += slot_size(k.m0 + i);
        }
    }
    v.src = in.msgs ? nullptr : in.h_in + b0;
    if (!in.direct) {
        if (in.msgs) c->pool->gather(h.stage_in, in.msgs + k.m0, in.sizes + k.m0, k.n);
        else c->pool->copy(h.stage_in, v.src, k.in_bytes);
        v.src = h.stage_in;
    }
    uint8_t *d = h.dev;
    v.doff = reinterpret_cast<uint64_t *>(d + k.o_off);
    v.dslot = v.doff + (k.n + 1);
    v.dooff = reinterpret_cast<uint64_t *>(d + k.o_ooff);
    v.dst = reinterpret_cast<int32_t *>(d + k.o_st);
    v.dlen = reinterpret_cast<uint64_t *>(d + k.o_len);
    v.slot_bytes = acc;
    v.s_in = c->slot_streams ? h.stream : c->hin;
    v.s_ex = c->slot_streams ? h.stream : c->hex;
    return TDT_OK;
}

int host_encode(tdt_ctx *c, const uint8_t *h_in, const uint64_t *h_in_off, uint32_t n_msgs, uint8_t *h_out,
                uint64_t out_cap, uint64_t *h_out_off, int32_t *h_status, const uint8_t *const *msgs = nullptr,
                const uint64_t *sizes = nullptr) {
    const int ws = c->cfg.word_size;
    const bool pin_in = !msgs && is_pinned(h_in + h_in_off[0]);
    // gather input from pinned caller buffers (a channel's pinned message memory): DMA'd run by
    // run of adjacent messages instead of staged by the copy pool.  A pointer-attribute query per
    // message (~1 µs): only for calls of up to 4096 messages whose first message is pinned (a
    // pageable first message — the common case — costs one query)
    bool msgs_pinned = msgs && n_msgs <= 4096;
    for (uint32_t i = 0; i < n_msgs && msgs_pinned; ++i) msgs_pinned = sizes[i] == 0 || is_pinned(msgs[i]);
    // a pinned caller buffer receives the chunks' output straight from the copy kernels
    uint8_t *d_out = nullptr;
    if (is_pinned(h_out) && hipHostGetDevicePointer(reinterpret_cast<void **>(&d_out), h_out, 0) != hipSuccess) {
        (void)hipGetLastError();
        d_out = nullptr;
    }
    const bool pin_out = d_out != nullptr;
    // one pass with the look-back when every message is <= 64 KiB and they average >= 16 KiB (as
    // tdt_encode_batch); otherwise the slotted message-class kernels (a 1 MiB message spreads over
    // 64 KiB tiles instead of running in one workgroup) and a gather into the host buffer
    bool lb = h_in_off[n_msgs] - h_in_off[0] >= 16384ull * n_msgs;
    for (uint32_t i = 0; i < n_msgs && lb; ++i) lb = h_in_off[i + 1] - h_in_off[i] <= kBigMin;
    // TDT_OPT_HOST_RAW_FALLBACK: always the slots, of n + 4 bytes each (the look-back kernel publishes a
    // blob's TDT length from inside, so it cannot serve), and behind the chunk's encode the flag pass, the
    // scan of the final lengths and the gather that takes a flagged blob from the chunk's input
    const bool raw = c->host_raw_fallback;
    if (raw) lb = false;
    // generic word sizes have no one-pass kernel (encode_common refuses them): their chunks are slotted
    if (psy::anyws_generic(ws)) lb = false;
    uint64_t fallen = 0;
    std::vector<Chunk> ch;
    const uint64_t cb = host_chunk_bytes(h_in_off, n_msgs);
    for (uint32_t m = 0; m < n_msgs;) {
        ch.push_back(plan_chunk(h_in_off, m, n_msgs, true, !lb, ws, nullptr, cb, raw));
        m += ch.back().n;
    }
    if (int st = psy::grow(c->hbases, c->hbases_n, ch.size() + 1, psy::cap_exact(ch.size() + 1, c->hbases_n), dev_free,
                           DevAlloc{8}))
        return st;
    uint64_t base = 0;  // output bytes of the chunks finished so far
    bool capacity = false;
    const HostIn in{h_in, h_in_off, msgs, sizes, pin_in || msgs_pinned};
    auto bound_of = [&](uint32_t i) {
        const uint64_t len = h_in_off[i + 1] - h_in_off[i];
        return raw ? psy::raw_blob_bytes(len) : tdt_encode_bound(len, ws);
    };
    auto issue = [&](size_t ci) -> int {
        const Chunk &k = ch[ci];
        auto &h = c->hs[ci % kHostSlots];
        ChunkView v;
        int st = chunk_prologue(c, k, ci, in, pin_out ? 0 : k.cap, k.scap != 0, bound_of, v);
        if (st) return st;
        uint8_t *d = h.dev;
        const hipStream_t s_in = v.s_in, s_ex = v.s_ex;
        if (v.src) {
            HIPCHK(hipMemcpyAsync(d, v.src, k.in_bytes, hipMemcpyHostToDevice, s_in));
        } else {  // pinned gather input: DMA'd run by run of adjacent messages
            for (uint32_t i = 0; i < k.n;) {
                const uint8_t *p0 = msgs[k.m0 + i];
                uint64_t len = sizes[k.m0 + i];
                uint32_t j = i + 1;
                while (j < k.n && msgs[k.m0 + j] == p0 + len) len += sizes[k.m0 + j++];
                if (len) HIPCHK(hipMemcpyAsync(d + h.pin[i], p0, len, hipMemcpyHostToDevice, s_in));
                i = j;
            }
        }
        // in_off and (slotted) the slots: one copy
        HIPCHK(hipMemcpyAsync(v.doff, h.pin, (k.scap ? 16ull : 8ull) * (k.n + 1), hipMemcpyHostToDevice, s_in));
        if (s_in != s_ex) {
            HIPCHK(hipEventRecord(h.evi, s_in));
            HIPCHK(hipStreamWaitEvent(s_ex, h.evi, 0));
        }
        psy::EncodeArgs a{};
        a.in = d;
        a.in_off = v.doff;
        a.n_msgs = k.n;
        a.status = v.dst;
        Where w(s_ex);
        w.wsp = d + k.o_ws;
        if (k.scap) {
            a.out = d + k.o_sbuf;
            a.out_cap = k.scap;
            a.slot_off = v.dslot;
            a.out_len = v.dlen;
            w.pws = &h.pw;
            if ((st = encode_common(c, psy::MODE_ENCODE, a, w))) return st;
            if (raw) {  // (the count: the word behind the chunk's out_off, read back with it)
                hipLaunchKernelGGL(host_raw_flag_kernel, dim3(1), dim3(1024), 0, s_ex, v.doff, v.dslot, v.dst, v.dlen,
                                   reinterpret_cast<uint32_t *>(d + k.o_rf), v.dooff + k.n + 1, k.n);
                HIPCHK(hipGetLastError());
            }
            hipLaunchKernelGGL(host_scan_kernel, dim3(1), dim3(1024), 0, s_ex, v.dlen, v.dooff, k.n);
            HIPCHK(hipGetLastError());
        } else {
            a.out = d + k.o_out;
            a.out_cap = k.cap;
            a.out_off = v.dooff;
            w.small_teams = k.in_bytes <= kSmallMax * k.n ? 1 : 0;  // (the chunk's sizes are host data)
            if ((st = encode_common(c, psy::MODE_ENCODE, a, w))) return st;
        }
        // the output, in chunk order (each copy follows the previous chunk's: the running base)
        if (ci == 0) HIPCHK(hipMemsetAsync(c->hbases, 0, 8, s_ex));
        else if (c->slot_streams) HIPCHK(hipStreamWaitEvent(s_ex, c->hs[(ci - 1) % kHostSlots].evc, 0));
        uint8_t *odst = pin_out ? d_out : h.stage_out;
        if (k.scap) {
            const uint32_t P = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, k.in_bytes / k.n / 16384));
            const uint32_t grid = (uint32_t)std::min<uint64_t>(2048, ((uint64_t)k.n * P + 3) / 4);
            if (raw)
                hipLaunchKernelGGL(host_raw_gather_kernel, dim3(grid), dim3(256), 0, s_ex, d, v.doff, d + k.o_sbuf, v.dslot,
                                   v.dlen, reinterpret_cast<const uint32_t *>(d + k.o_rf), v.dooff, k.n, P, odst,
                                   c->hbases, (uint32_t)ci, out_cap, pin_out ? 1 : 0);
            else
                hipLaunchKernelGGL(host_gather_kernel, dim3(grid), dim3(256), 0, s_ex, d + k.o_sbuf, v.dslot, v.dlen,
                                   v.dooff, k.n, P, odst, c->hbases, (uint32_t)ci, out_cap, pin_out ? 1 : 0);
        } else {
            const uint32_t grid = (uint32_t)std::min<uint64_t>(1024, k.cap / 4096 + 1);
            hipLaunchKernelGGL(host_out_kernel, dim3(grid), dim3(256), 0, s_ex, d + k.o_out, v.dooff, k.n, odst,
                               c->hbases, (uint32_t)ci, out_cap, pin_out ? 1 : 0);
        }
        HIPCHK(hipGetLastError());
        if (c->slot_streams) HIPCHK(hipEventRecord(h.evc, s_ex));
        if ((st = small_copies(s_ex, d + k.o_ws + 4, h.flag, 4, v.dooff, pin_back(h, k), 8ull * chunk_back_words(k), v.dst,
                               pin_status(h, k), 4ull * k.n)))
            return st;
        HIPCHK(hipEventRecord(h.ev, s_ex));
        return TDT_OK;
    };
    // chunk ci's compacted size is known once its event fires; then its output comes back
    auto finish = [&](size_t ci) -> int {
        const Chunk &k = ch[ci];
        auto &h = c->hs[ci % kHostSlots];
        HIPCHK(hipEventSynchronize(h.ev));
        const uint64_t *pin_out_off = pin_back(h, k);
        const uint64_t total = pin_out_off[k.n];
        if (capacity || base + total > out_cap) capacity = true;
        for (uint32_t i = 0; i < k.n; ++i) h_out_off[k.m0 + i] = base + (capacity ? 0 : pin_out_off[i]);
        if (h_status) std::memcpy(h_status + k.m0, pin_status(h, k), 4ull * k.n);
        if (raw) fallen += pin_out_off[k.n + 1];
        // (the copy kernel has written the output: into h_out directly, or into the staging)
        if (!capacity && total && !pin_out) c->pool->copy(h_out + base, h.stage_out, total);
        if (!capacity) base += total;
        return TDT_OK;
    };
    int st = host_loop(ch.size(), issue, finish);
    if (st) return st;
    for (auto &h : c->hs)
        if (h.stream && (st = sync_slot(c, h))) return st;
    h_out_off[n_msgs] = base;
    c->host_rf_count.store(fallen);
    if (capacity) return set_err(TDT_E_CAPACITY, "host output capacity exceeded");
    return TDT_OK;
}

int host_decode(tdt_ctx *c, const uint8_t *h_in, const uint64_t *h_in_off, uint32_t n_msgs, uint8_t *h_out,
                uint64_t out_cap, uint64_t *h_out_off, int32_t *h_status) {
    // decoded sizes from the headers → every chunk's output offsets are known up front: the
    // decode is slotted at those offsets
    std::vector<uint64_t> dsz(n_msgs);
    uint64_t need = 0;
    for (uint32_t i = 0; i < n_msgs; ++i) {
        dsz[i] = host_decoded_size(h_in + h_in_off[i], h_in_off[i + 1] - h_in_off[i]);
        need += dsz[i];
    }
    if (need > out_cap) return set_err(TDT_E_CAPACITY, "host output capacity exceeded");
    const bool pin_in = is_pinned(h_in + h_in_off[0]), pin_out = is_pinned(h_out);
    // the device's view of a pinned caller buffer (registered memory may map elsewhere)
    uint8_t *d_hout = nullptr;
    if (pin_out && hipHostGetDevicePointer(reinterpret_cast<void **>(&d_hout), h_out, 0) != hipSuccess) {
        (void)hipGetLastError();
        d_hout = nullptr;
    }
    const bool dma_out = c->dout_sdma || (pin_out && !d_hout);
    std::vector<Chunk> ch;
    uint64_t base = 0;
    const uint64_t cb = host_chunk_bytes(h_in_off, n_msgs);
    for (uint32_t m = 0; m < n_msgs;) {
        ch.push_back(plan_chunk(h_in_off, m, n_msgs, false, false, c->cfg.word_size, dsz.data(), cb));
        ch.back().base = base;
        base += ch.back().cap;
        m += ch.back().n;
    }
    std::vector<uint64_t> lens(n_msgs);
    std::vector<int32_t> stv(n_msgs);
    const HostIn in{h_in, h_in_off, nullptr, nullptr, pin_in};
    auto issue = [&](size_t ci) -> int {
        const Chunk &k = ch[ci];
        auto &h = c->hs[ci % kHostSlots];
        ChunkView v;
        int st = chunk_prologue(c, k, ci, in, pin_out ? 0 : k.cap, true, [&](uint32_t i) { return dsz[i]; }, v);
        if (st) return st;
        uint8_t *d = h.dev;
        const uint64_t acc = v.slot_bytes;  // the chunk's decoded bytes
        // input copies in chunk order, each after the previous chunk's: concurrent copies of
        // several slots share the link and all land late, the earliest-needed one included
        // (decode 31 -> 37 GiB/s pinned; the same ordering cost host_encode 44 -> 36 GiB/s,
        // profiles/r05_diag/host_decode/)
        const hipStream_t s_in = v.s_in, s_ex = v.s_ex;
        if (ci > 0 && c->slot_streams) HIPCHK(hipStreamWaitEvent(s_in, c->hs[(ci - 1) % kHostSlots].evi, 0));
        HIPCHK(hipMemcpyAsync(d, v.src, k.in_bytes, hipMemcpyHostToDevice, s_in));
        HIPCHK(hipMemcpyAsync(v.doff, h.pin, 16ull * (k.n + 1), hipMemcpyHostToDevice, s_in));  // offsets + slots
        HIPCHK(hipEventRecord(h.evi, s_in));
        if (s_in != s_ex) HIPCHK(hipStreamWaitEvent(s_ex, h.evi, 0));
        psy::DecodeArgs a{};
        a.in = d;
        a.in_off = v.doff;
        a.n_msgs = k.n;
        a.out = d + k.o_out;
        a.status = v.dst;
        a.slot_off = v.dslot;
        a.out_len = v.dlen;
        Where w(s_ex);
        w.wsp = d + k.o_ws;
        w.pws = &h.pw;
        if ((st = decode_common(c, false, a, w))) return st;
        if (acc && dma_out) {
            HIPCHK(hipMemcpyAsync(pin_out ? h_out + k.base : h.stage_out, d + k.o_out, acc, hipMemcpyDeviceToHost,
                                  s_ex));
        } else if (acc) {
            // the output crosses PCIe as a copy kernel's stores (as host_encode's), not a DMA: the
            // DMA engines then carry only the H2D direction
            hipLaunchKernelGGL(host_dout_kernel, dim3((uint32_t)std::min<uint64_t>(1024, acc / 4096 + 1)), dim3(256), 0,
                               s_ex, d + k.o_out, pin_out ? d_hout + k.base : h.stage_out, acc);
            HIPCHK(hipGetLastError());
        }
        if ((st = small_copies(s_ex, d + k.o_ws + 4, h.flag, 4, v.dlen, pin_back(h, k), 8ull * k.n, v.dst,
                               pin_status(h, k), 4ull * k.n)))
            return st;
        HIPCHK(hipEventRecord(h.ev, s_ex));
        return TDT_OK;
    };
    auto finish = [&](size_t ci) -> int {
        const Chunk &k = ch[ci];
        auto &h = c->hs[ci % kHostSlots];
        HIPCHK(hipEventSynchronize(h.ev));
        if (!pin_out && k.cap) c->pool->copy(h_out + k.base, h.stage_out, k.cap);
        std::memcpy(lens.data() + k.m0, pin_back(h, k), 8ull * k.n);
        std::memcpy(stv.data() + k.m0, pin_status(h, k), 4ull * k.n);
        return TDT_OK;
    };
    int st = host_loop(ch.size(), issue, finish);
    if (st) return st;
    for (auto &h : c->hs) {
        st = h.stream ? sync_slot(c, h) : TDT_OK;
        if (st) return st;
    }
    // offsets; blobs the kernel rejected (status != OK, length 0) leave a gap: compact it
    uint64_t w = 0, r = 0;
    for (uint32_t i = 0; i < n_msgs; ++i) {
        h_out_off[i] = w;
        if (lens[i] && w != r) std::memmove(h_out + w, h_out + r, lens[i]);
        w += lens[i];
        r += dsz[i];
        if (h_status) h_status[i] = stv[i];
    }
    h_out_off[n_msgs] = w;
    return TDT_OK;
}

// ---------------------------------------------------------------------------------------
// One-message fast path.  Block layout (`one`, mapped pinned memory): [0, 256) argument words,
// then the input at kOneIn, then the output.  The class kernel of the message's size runs as a
// single workgroup on a one-entry list; every argument, the input and the output live in host
// memory the kernel reads and writes over PCIe.
constexpr uint64_t kOneMax = 256 * 1024;  // largest message (encode) / decoded message the path takes
constexpr size_t kOneIn = 256;
struct OneArgs {
    uint64_t off[2];   // input offsets
    uint64_t slot[2];  // output slot
    uint64_t len;      // output length
    int32_t status;
    uint32_t list, cnt, flags;
    uint32_t done, pad;  // completion word (one_spin: written by the stream after the kernel)
};

int ensure_one(tdt_ctx *c, size_t bytes) {
    if (!c->one_stream) HIPCHK(hipStreamCreateWithFlags(&c->one_stream, hipStreamNonBlocking));
    // coherent (fine-grained, uncached on the device): the kernel's result stores reach host
    // memory before the stream writes the completion word the host spins on, with no cache
    // write-back to order; the block is read and written once per call anyway
    return psy::grow(c->one, c->one_bytes, bytes, std::max<size_t>(bytes, 64 * 1024), pin_free,
                     PinAlloc{1, hipHostMallocCoherent});
}

template <int WS>
void launch_one_encode(const psy::EncodeArgs &a, uint64_t n, hipStream_t s) {
    using psy::MODE_ENCODE;
    if (n <= kSmallMax)
        hipLaunchKernelGGL((psy::tdt_encode_kernel<WS, 64, 4, MODE_ENCODE, 0, 0, 0>), dim3(1), dim3(64), 0, s, a);
    else if (n <= kMidMax)
        hipLaunchKernelGGL((psy::tdt_encode_kernel<WS, 256, 8, MODE_ENCODE, 0, 0, 0>), dim3(1), dim3(256), 0, s, a);
    else if (n <= 65536 && (n & 15) == 0)  // (the block's input is 16-byte aligned: resident)
        hipLaunchKernelGGL((psy::tdt_encode_kernel<WS, 512, 8, MODE_ENCODE, 0, 0, 0, psy::PATH_RES>), dim3(1),
                           dim3(512), 0, s, a);
    else
        hipLaunchKernelGGL((psy::tdt_encode_kernel<WS, 512, 8, MODE_ENCODE, 0, 0, 0, psy::PATH_STREAM>), dim3(1),
                           dim3(512), 0, s, a);
}

// returns TDT_OK, an error, or -1: not taken (the pipeline serves the call)
int host_one(tdt_ctx *c, bool encode, const uint8_t *h_in, const uint64_t *h_in_off, uint8_t *h_out,
             uint64_t out_cap, uint64_t *h_out_off, int32_t *h_status) {
    const uint64_t len = h_in_off[1] - h_in_off[0];
    const uint8_t *src = h_in + h_in_off[0];
    uint64_t osize;
    if (encode) {
        if (len > kOneMax || !psy::anyws_tuned(c->cfg.word_size)) return -1;  // (generic widths: the pipeline)
        // (TDT_OPT_HOST_RAW_FALLBACK: a slot of n + 4 — a longer TDT blob leaves TDT_E_CAPACITY, below)
        osize = c->host_raw_fallback ? psy::raw_blob_bytes(len) : tdt_encode_bound(len, c->cfg.word_size);
    } else {
        // a TDT blob of a generic word size is decoded by the pipeline's follow-up launch
        if (len >= 16) {
            uint32_t magic, bws;
            std::memcpy(&magic, src, 4);
            std::memcpy(&bws, src + 12, 4);
            if (magic == psy::kMagicTDT && !psy::anyws_tuned((int)bws)) return -1;
        }
        osize = host_decoded_size(src, len);
        if (osize > kOneMax || len > 2 * kOneMax + 1024) return -1;
        if (osize > out_cap) return set_err(TDT_E_CAPACITY, "host output capacity exceeded");
    }
    const size_t o_out = kOneIn + align_up(std::max<uint64_t>(len, 1), 256);
    int st = ensure_one(c, o_out + align_up(std::max<uint64_t>(osize, 1), 256) + 256);
    if (st) return st;
    uint8_t *hb = c->one;
    uint8_t *db = nullptr;
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&db), hb, 0));
    OneArgs *A = reinterpret_cast<OneArgs *>(hb);
    const OneArgs *dA = reinterpret_cast<const OneArgs *>(db);
    A->off[0] = 0;
    A->off[1] = len;
    A->slot[0] = 0;
    A->slot[1] = osize;
    A->len = 0;
    A->status = -1;
    A->list = 0;
    A->cnt = 1;
    A->flags = 0;
    A->done = 0;
    if (len) std::memcpy(hb + kOneIn, src, len);
    hipStream_t s = c->one_stream;
    if (encode) {
        psy::EncodeArgs a{};
        a.in = db + kOneIn;
        a.in_off = dA->off;
        a.n_msgs = 1;
        a.out = db + o_out;
        a.slot_off = dA->slot;
        a.out_len = const_cast<uint64_t *>(&dA->len);
        a.status = const_cast<int32_t *>(&dA->status);
        wire_encode(c, a, nullptr);  // (no workspace: the block's own flag word)
        a.errflags = const_cast<uint32_t *>(&dA->flags);
        a.list = &dA->list;
        a.list_count = &dA->cnt;
        if (!with_word_size(c->cfg.word_size, [&](auto W) { launch_one_encode<W()>(a, len, s); }))
            return -1;  // (generic widths took the pipeline above)
    } else {
        psy::DecodeArgs a{};
        a.in = db + kOneIn;
        // (blobs are read in place over PCIe: staging them into HBM first, in the kernel or by a
        // copy, measured no faster — profiles/r05_diag/one_message/)
        const bool one_wave = c->one_wave || osize <= c->one_wave_max;
        a.in_off = dA->off;
        a.n_msgs = 1;
        a.out = db + o_out;
        a.slot_off = dA->slot;
        a.out_len = const_cast<uint64_t *>(&dA->len);
        a.status = const_cast<int32_t *>(&dA->status);
        a.errflags = const_cast<uint32_t *>(&dA->flags);
        a.list = &dA->list;
        a.list_count = &dA->cnt;
        if (one_wave)
            hipLaunchKernelGGL((psy::tdt_decode_kernel<0, psy::kDecWR, 0>), dim3(1), dim3(64), 0, s, a);
        else  // a workgroup of kOneWaves waves: tiles of the blob (tdt_decode_one_kernel)
            hipLaunchKernelGGL((psy::tdt_decode_one_kernel<psy::kOneWaves>), dim3(1), dim3(64 * psy::kOneWaves), 0,
                               s, a);
    }
    HIPCHK(hipGetLastError());
    bool done = false;
    if (c->one_spin) {
        // the stream writes `done` after the kernel; the host spins on it (1 ms at most, then the
        // stream sync, which also reports a failed kernel)
        const uint32_t seq = ++c->one_seq ? c->one_seq : ++c->one_seq;
        HIPCHK(hipStreamWriteValue32(s, const_cast<uint32_t *>(&dA->done), seq, 0));
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t k = 1;; ++k) {
            if (__atomic_load_n(&A->done, __ATOMIC_ACQUIRE) == seq) {
                done = true;
                break;
            }
            __builtin_ia32_pause();
            if ((k & 255) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(1)) break;
        }
    }
    if (!done) HIPCHK(hipStreamSynchronize(s));
    c->host_flags.fetch_or(A->flags);
    uint64_t olen = A->len;
    int32_t ost = A->status;
    // TDT_OPT_HOST_RAW_FALLBACK: the TDT blob did not fit n + 4 bytes — the host stores the message raw,
    // from the caller's own bytes: no second launch, and no blob byte crosses PCIe
    const bool fell = encode && c->host_raw_fallback && psy::raw_flagged(ost, olen, len, osize);
    if (fell) {
        olen = psy::raw_blob_bytes(len);
        ost = TDT_OK;
    }
    if (h_status) h_status[0] = ost;
    h_out_off[0] = 0;
    if (encode && olen > out_cap) {
        h_out_off[1] = 0;
        return set_err(TDT_E_CAPACITY, "host output capacity exceeded");
    }
    if (fell) {
        for (uint32_t k = 0; k < psy::kRawMarkerBytes; ++k) h_out[k] = psy::raw_marker_byte(k);
        std::memcpy(h_out + psy::kRawMarkerBytes, src, len);
        c->host_rf_count.store(1);
    } else if (olen) {
        std::memcpy(h_out, hb + o_out, olen);
    }
    h_out_off[1] = olen;
    return TDT_OK;
}

// msgs / sizes: gather input (encode, more than one message; HostIn)
int host_path(tdt_ctx *c, bool encode, const uint8_t *h_in, const uint64_t *h_in_off, uint32_t n_msgs,
              uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_off, int32_t *h_status,
              const uint8_t *const *msgs = nullptr, const uint64_t *sizes = nullptr) {
    if (!c) return set_err(TDT_E_ARG, "null context");
    if (encode) c->host_rf_count.store(0);  // (TDT_STAT_HOST_RAW_FALLBACKS: of the most recent host encode call)
    if (n_msgs == 0) {
        if (h_out_off) h_out_off[0] = 0;
        return TDT_OK;
    }
    if (!h_in_off || !h_out_off) return set_err(TDT_E_ARG, "null offsets");
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->hmu);  // the pipeline slots belong to the context
    if (n_msgs == 1 && !msgs && !c->no_one) {
        const int st1 = host_one(c, encode, h_in, h_in_off, h_out, out_cap, h_out_off, h_status);
        if (st1 >= 0) return st1;
    }
    if (!c->pool) c->pool.reset(new CopyPool(c->copy_threads));
    const int st = encode ? host_encode(c, h_in, h_in_off, n_msgs, h_out, out_cap, h_out_off, h_status, msgs, sizes)
                          : host_decode(c, h_in, h_in_off, n_msgs, h_out, out_cap, h_out_off, h_status);
    if (st != TDT_OK) {
        // an error mid-pipeline: the other slot's copies and kernels may still read the caller's
        // input or write its output — drain both slots before the caller gets its buffers back
        drain_host(c);
        (void)hipGetLastError();
    }
    return st;
}

}  // namespace

namespace {
// any message longer than `lim` bytes → *flag |= 1; any message that the resident-only kernel
// cannot hold (unaligned start, a partial 16-byte group, over 64 KiB) → *flag |= 2 (one atomic
// per workgroup and bit)
__global__ __launch_bounds__(256) void cp_big_kernel(const uint8_t *in, const uint64_t *in_off, uint32_t n,
                                                     uint64_t lim, uint64_t *flag) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint64_t len = i < n ? in_off[i + 1] - in_off[i] : 0;
    const bool big = i < n && len > lim;
    const bool nonres = i < n && (len > 65536 || (len & 15) != 0 || (((uintptr_t)in + in_off[i]) & 15) != 0);
    const bool any_big = __syncthreads_or(big), any_nonres = __syncthreads_or(nonres);
    if (threadIdx.x == 0 && (any_big || any_nonres))
        atomicOr(reinterpret_cast<unsigned long long *>(flag), (any_big ? 1ull : 0ull) | (any_nonres ? 2ull : 0ull));
}
// lengths → the scan's input (in place in out_off)
__global__ __launch_bounds__(256) void cp_len_kernel(const uint64_t *len, uint64_t *out_off, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out_off[i] = len[i];
}
// blob i (one wave each, four per workgroup): slot → its compacted place (capacity: the
// TDT_E_CAPACITY of the look-back path; out_off keeps the full prefix sum either way), by the
// shared copy (tdt_copy.h).  src is the context's slot buffer on the device (cp_buf).
__global__ __launch_bounds__(256) void cp_gather_kernel(const uint8_t *src, const uint64_t *slot, const uint64_t *len,
                                                      uint8_t *dst, const uint64_t *out_off, uint64_t cap,
                                                      int32_t *status, uint32_t n) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const uint64_t o = out_off[i], l = len[i];
    if (o + l > cap) {
        if ((threadIdx.x & 63) == 0 && status && status[i] == 0) status[i] = TDT_E_CAPACITY;
        return;
    }
    psy::copy_shifted<1, false>(dst + o, src + slot[i], l, threadIdx.x & 63u, 64);
}
}  // namespace

static int scan_sizes(tdt_ctx *ctx, uint64_t *d_off, uint32_t n_msgs, hipStream_t stream);
// A cp_buf / cp_idx buffer that a larger one replaces (under ctx->mu): freed, unless a captured
// tdt_encode_batch_vp may still point at it — then it lives as long as the context.
static int cp_drop(tdt_ctx *ctx, void *p) { return ctx->cp_in_graph ? retire_to(ctx->retired)(p) : dev_free(p); }
// Room in the compaction buffers: idx_words u64 in cp_idx, buf_bytes in cp_buf (exact sizes), under
// ctx->mu — the caller lets go of it before encode_common takes it.  capturable: the call may run
// under stream capture (tdt_encode_batch_vp), where nothing grows and from which on nothing is freed.
static int ensure_cp(tdt_ctx *ctx, size_t idx_words, size_t buf_bytes, hipStream_t s, bool capturable = false) {
    if (capturable && capturing(s)) ctx->cp_in_graph = true;
    auto room = [&](auto *&p, size_t &have, size_t need, size_t unit) -> int {
        if (need <= have) return TDT_OK;
        if (capturable)
            if (int st = no_growth_in_capture(s)) return st;
        return psy::grow(p, have, need, psy::cap_exact(need, have), [ctx](void *old) { return cp_drop(ctx, old); },
                         DevAlloc{unit});
    };
    if (int st = room(ctx->cp_idx, ctx->cp_idx_n, idx_words, 8)) return st;
    return room(ctx->cp_buf, ctx->cp_bytes, buf_bytes, 1);
}
// The caller-visible fields every batch over one input buffer sets; the rest by name at the call.
template <class Args>
static Args batch_args(const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs, uint8_t *d_out, int32_t *d_status) {
    Args a{};
    a.in = d_in;
    a.in_off = d_in_off;
    a.n_msgs = n_msgs;
    a.out = d_out;
    a.status = d_status;
    return a;
}
static const Scatter scatter_of(const uint8_t *const *d_ptr, const uint64_t *d_size, uint8_t *const *d_out_ptr,
                                const uint64_t *d_out_cap) {
    // (device addresses are 64 bits wide: a pointer table read as u64 is the offset table of a null base)
    static_assert(sizeof(uint8_t *) == sizeof(uint64_t), "pointer tables are read as u64 offsets");
    return {reinterpret_cast<const uint64_t *>(d_ptr), d_size, reinterpret_cast<const uint64_t *>(d_out_ptr), d_out_cap};
}

// lengths → d_out_off, scanned in place: exclusive offsets, the total at [n]
static int scan_lengths(tdt_ctx *ctx, const uint64_t *d_len, uint64_t *d_out_off, uint32_t n_msgs, hipStream_t s) {
    hipLaunchKernelGGL(cp_len_kernel, dim3((n_msgs + 255) / 256), dim3(256), 0, s, d_len, d_out_off, n_msgs);
    HIPCHK(hipGetLastError());
    return scan_sizes(ctx, d_out_off, n_msgs, s);
}

// The two-phase compaction reads a few bytes back to choose its path: not under stream capture
// (the one-pass kernels need no read-back), nor with the no-two-phase knob.
static bool two_phase_ok(const tdt_ctx *ctx, void *stream) {
    if (ctx->no_two_phase) return false;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) return false;
    return cap == hipStreamCaptureStatusNone;
}

// tdt_copy_device (include/psyne_tdt.h): one 512-lane workgroup per 64 KiB piece, its eight
// 16-byte loads per lane in flight before the non-temporal stores (tools/ubench_hbm.hip "chunk"
// row: the fastest hand-written copy shape measured on the box).  Both pointers 16-byte aligned;
// the caller handles any ragged head / tail.
constexpr uint32_t kCopyPiece = 512u * 8u * 16u;
__global__ __launch_bounds__(512) void hbm_copy_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst,
                                                       uint64_t n16) {
    const uint64_t base = (uint64_t)blockIdx.x * (kCopyPiece / 16u) + threadIdx.x;
    if (base + 7u * 512u < n16) {
        uint4 v[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) v[g] = src[base + (uint64_t)g * 512u];
#pragma unroll
        for (int g = 0; g < 8; ++g) psy::st16_nt(dst + base + (uint64_t)g * 512u, v[g]);
    } else {
        for (int g = 0; g < 8; ++g)
            if (base + (uint64_t)g * 512u < n16) dst[base + (uint64_t)g * 512u] = src[base + (uint64_t)g * 512u];
    }
}
__global__ __launch_bounds__(256) void byte_copy_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                        uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) dst[i] = src[i];
}

extern "C" {

// (the raw fallback's routes, defined with the scattered encodes below)
static int encode_v_any(tdt_ctx *ctx, const Scatter &v, const int32_t *d_word_size, uint64_t width_mask, uint32_t n,
                        uint64_t *d_out_len, int32_t *d_status, void *stream, const uint64_t *d_mapbits);
static int encode_into_raw(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n, uint8_t *d_out,
                           const uint64_t *d_slot_off, uint64_t *d_out_len, int32_t *d_status, void *stream);
static int encode_compacted_raw(tdt_ctx *ctx, const psy::EncodeArgs &a, void *stream);
static int raw_min_sizes(tdt_ctx *ctx, const uint64_t *d_sizes, const uint64_t *d_in_off, uint64_t *d_enc, uint32_t n,
                         hipStream_t s);

int tdt_copy_device(void *d_dst, const void *d_src, uint64_t bytes, void *hip_stream) {
    if (bytes == 0) return TDT_OK;
    if (!d_dst || !d_src) return set_err(TDT_E_ARG, "null buffer");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    uint8_t *dst = static_cast<uint8_t *>(d_dst);
    const uint8_t *src = static_cast<const uint8_t *>(d_src);
    if ((((uintptr_t)dst ^ (uintptr_t)src) & 15u) != 0) {
        // different 16-byte phases: a byte copy (no caller of the codec needs this form fast)
        const uint64_t g = std::min<uint64_t>((bytes + 255) / 256, 65536);
        hipLaunchKernelGGL(byte_copy_kernel, dim3((uint32_t)g), dim3(256), 0, s, src, dst, bytes);
        HIPCHK(hipGetLastError());
        return TDT_OK;
    }
    const uint64_t head = std::min<uint64_t>((16u - ((uintptr_t)dst & 15u)) & 15u, bytes);
    if (head) hipLaunchKernelGGL(byte_copy_kernel, dim3(1), dim3(256), 0, s, src, dst, head);
    const uint64_t n16 = (bytes - head) / 16u, tail = bytes - head - 16u * n16;
    if (n16) {
        const uint64_t pieces = (n16 * 16u + kCopyPiece - 1) / kCopyPiece;
        if (pieces >= (1ull << 31)) return set_err(TDT_E_ARG, "copy too large");
        hipLaunchKernelGGL(hbm_copy_kernel, dim3((uint32_t)pieces), dim3(512), 0, s,
                           reinterpret_cast<const uint4 *>(src + head), reinterpret_cast<uint4 *>(dst + head), n16);
    }
    if (tail) hipLaunchKernelGGL(byte_copy_kernel, dim3(1), dim3(256), 0, s, src + head + 16u * n16,
                                 dst + head + 16u * n16, tail);
    HIPCHK(hipGetLastError());
    return TDT_OK;
}

void tdt_default_config(tdt_config *cfg) {
    cfg->sample_fraction = 0.3f;
    cfg->word_size = 4;
    cfg->bandwidth_threshold_mbps = 100.0;
    cfg->cpu_usage_threshold = 0.8;
    cfg->min_tensor_size = 1024;
}

int tdt_ctx_create(int device, const tdt_config *cfg, tdt_ctx **out) {
    if (!out) return set_err(TDT_E_ARG, "null out");
    *out = nullptr;
    tdt_config c;
    if (cfg) c = *cfg;
    else tdt_default_config(&c);
    if (c.word_size <= 0) return set_err(TDT_E_CONFIG, "word_size must be positive");
    if (!ws_supported(c.word_size)) return set_err(TDT_E_UNSUPPORTED, "GPU codec supports word_size 1..64");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return set_err(TDT_E_ARG, "bad device");
    tdt_ctx *x = new tdt_ctx();
    x->device = device;
    x->cfg = c;
    // tuning / test overrides, read once here (tdt_ctx_set_option changes them later): the
    // tiled-path threshold, a lower tile budget (fallback tests), the diagnostic stream knobs
    if (const char *e = std::getenv("PSYNE_TDT_LARGE_MIN")) x->large_min = std::strtoull(e, nullptr, 10);
    if (const char *e = std::getenv("PSYNE_TDT_TILE_CAP")) x->tile_cap = (uint32_t)std::strtoul(e, nullptr, 10);
    if (const char *e = std::getenv("PSYNE_TDT_ANY_TILED")) x->any_tiled = *e != '0';
    if (const char *e = std::getenv("PSYNE_TDT_ANY_DEC_TILED")) x->any_dec_tiled = *e != '0';
    auto flag = [](const char *name) {
        const char *e = std::getenv(name);
        return e && *e == '1';
    };
    x->no_side = flag("PSYNE_TDT_NO_SIDE");
    x->small_main = flag("PSYNE_TDT_SMALL_MAIN");
    x->no_two_phase = flag("PSYNE_TDT_NO_TWO_PHASE");
    x->raw_fallback = flag("PSYNE_TDT_RAW_FALLBACK");
    x->host_raw_fallback = flag("PSYNE_TDT_HOST_RAW_FALLBACK");
    x->no_one = flag("PSYNE_TDT_NO_ONE");
    x->one_wave = flag("PSYNE_TDT_ONE_WAVE");
    x->dout_sdma = flag("PSYNE_TDT_DOUT_SDMA");
    x->slot_streams = flag("PSYNE_TDT_SLOT_STREAMS");
    if (const char *e = std::getenv("PSYNE_TDT_ONE_SPIN")) x->one_spin = *e == '1';
    if (const char *e = std::getenv("PSYNE_TDT_DBIG_MIN")) x->dbig_min = std::strtoull(e, nullptr, 10);
    if (const char *e = std::getenv("PSYNE_TDT_DSMALL_MAX")) x->dsmall_max = std::strtoull(e, nullptr, 10);
    if (const char *e = std::getenv("PSYNE_TDT_COPY_WGS")) x->copy_wgs = std::max(1ul, std::strtoul(e, nullptr, 10));
    if (const char *e = std::getenv("PSYNE_TDT_PACK_CUT")) x->pack_cut = (uint32_t)std::strtoul(e, nullptr, 10);
    if (const char *e = std::getenv("PSYNE_TDT_PACK_GRID"))
        x->pack_grid = (uint32_t)std::max(1ul, std::min(1ul << 30, std::strtoul(e, nullptr, 10)));
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        x->cus = cus;
    // staging-copy threads: up to 16, within this process's CPU affinity (PSYNE_TDT_COPY_THREADS)
    cpu_set_t cs;
    CPU_ZERO(&cs);
    if (sched_getaffinity(0, sizeof(cs), &cs) == 0) x->copy_threads = std::max(1, std::min(16, CPU_COUNT(&cs)));
    if (const char *e = std::getenv("PSYNE_TDT_COPY_THREADS"))
        x->copy_threads = std::max(1, std::min(64, (int)std::strtol(e, nullptr, 10)));
    *out = x;
    return TDT_OK;
}

void tdt_ctx_destroy(tdt_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    // every buffer the grower replaces is either freed at once or retired to exactly one list
    // (ctx->retired, ctx->retired_host, a PlanWS's own): the current buffers here, each list once
    for (void *p : {(void *)ctx->ws, (void *)ctx->slot_sums, (void *)ctx->cp_buf, (void *)ctx->cp_idx, (void *)ctx->mx_tab,
                    (void *)ctx->hbases, (void *)ctx->rf_buf})
        if (p) (void)hipFree(p);
    for (void *p : ctx->retired) (void)hipFree(p);
    for (void *p : ctx->retired_host) (void)hipHostFree(p);
    ctx->pw.release();
    ctx->anyw.release();
    ctx->anydw.release();
    ctx->rf_h.release();
    for (auto &w : ctx->mx_pw)
        if (w) w->release();
    if (ctx->one_stream) (void)hipStreamSynchronize(ctx->one_stream);
    if (ctx->one) (void)hipHostFree(ctx->one);
    if (ctx->one_stream) (void)hipStreamDestroy(ctx->one_stream);
    if (ctx->astream) (void)hipStreamSynchronize(ctx->astream);
    if (ctx->h_dev) (void)hipFree(ctx->h_dev);
    if (ctx->astream) (void)hipStreamDestroy(ctx->astream);
    for (auto &h : ctx->hs) {
        if (h.stream) (void)hipStreamSynchronize(h.stream);
        if (h.dev) (void)hipFree(h.dev);
        if (h.pin) (void)hipHostFree(h.pin);
        if (h.flag) (void)hipHostFree(h.flag);
        if (h.stage_in) (void)hipHostFree(h.stage_in);
        if (h.stage_out) (void)hipHostFree(h.stage_out);
        h.pw.release();
        if (h.ev) (void)hipEventDestroy(h.ev);
        if (h.evc) (void)hipEventDestroy(h.evc);
        if (h.evi) (void)hipEventDestroy(h.evi);
        if (h.stream) (void)hipStreamDestroy(h.stream);
    }
    if (ctx->hin) (void)hipStreamSynchronize(ctx->hin);
    if (ctx->hex) (void)hipStreamSynchronize(ctx->hex);
    if (ctx->hin) (void)hipStreamDestroy(ctx->hin);
    if (ctx->hex) (void)hipStreamDestroy(ctx->hex);
    delete ctx;
}

void tdt_ctx_set_metrics(tdt_ctx *ctx, double bandwidth_mbps, double latency_ms, double cpu_usage) {
    ctx->bandwidth.store(bandwidth_mbps);
    ctx->latency.store(latency_ms);
    ctx->cpu.store(cpu_usage);
}

void tdt_ctx_get_metrics(const tdt_ctx *ctx, double *bandwidth_mbps, double *latency_ms, double *cpu_usage) {
    if (bandwidth_mbps) *bandwidth_mbps = ctx->bandwidth.load();
    if (latency_ms) *latency_ms = ctx->latency.load();
    if (cpu_usage) *cpu_usage = ctx->cpu.load();
}

void tdt_ctx_set_size_hint(tdt_ctx *ctx, uint64_t bytes) { ctx->size_hint.store(bytes); }

int tdt_ctx_set_option(tdt_ctx *ctx, int option, uint64_t value) {
    if (!ctx) return set_err(TDT_E_ARG, "null context");
    if (option == TDT_OPT_COPY_THREADS) {
        // the copy pool belongs to the host pipeline (hmu); lock order everywhere: hmu, then mu
        std::lock_guard<std::mutex> hl(ctx->hmu);
        ctx->copy_threads = (int)std::max<uint64_t>(1, std::min<uint64_t>(value, 64));
        ctx->pool.reset();
        return TDT_OK;
    }
    if (option == TDT_OPT_HOST_RAW_FALLBACK) {  // (read by the host calls, under hmu)
        std::lock_guard<std::mutex> hl(ctx->hmu);
        ctx->host_raw_fallback = value != 0;
        return TDT_OK;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    switch (option) {
        case TDT_OPT_LARGE_MIN: ctx->large_min = value; return TDT_OK;
        case TDT_OPT_TILE_CAP: ctx->tile_cap = (uint32_t)std::min<uint64_t>(value, 0xffffffffu); return TDT_OK;
        case TDT_OPT_NO_SIDE_STREAM: ctx->no_side = value != 0; return TDT_OK;
        case TDT_OPT_SMALL_ON_CALLER_STREAM: ctx->small_main = value != 0; return TDT_OK;
        case TDT_OPT_NO_TWO_PHASE: ctx->no_two_phase = value != 0; return TDT_OK;
        case TDT_OPT_PACK_SIZES_FIRST: ctx->pack_sizes_first = value == 2 ? 2 : value != 0 ? 1 : 0; return TDT_OK;
        case TDT_OPT_ANY_TILED: ctx->any_tiled = value != 0; return TDT_OK;
        case TDT_OPT_ANY_DEC_TILED: ctx->any_dec_tiled = value != 0; return TDT_OK;
        case TDT_OPT_RAW_FALLBACK: ctx->raw_fallback = value != 0; return TDT_OK;
    }
    return set_err(TDT_E_ARG, "unknown option");
}

int tdt_ctx_get_stat(tdt_ctx *ctx, int stat, uint64_t *value) {
    if (!ctx || !value) return set_err(TDT_E_ARG, "null context or value");
    if (stat == TDT_STAT_HOST_RAW_FALLBACKS) {  // (host calls block: final when the call returned)
        *value = ctx->host_rf_count.load();
        return TDT_OK;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (stat == TDT_STAT_PACK_SCRATCH_BYTES) {
        *value = ctx->cp_bytes;
        return TDT_OK;
    }
    if (stat == TDT_STAT_RAW_FALLBACKS) {
        ctx->rf_h.refresh();  // (as below: the newest snapshot that has landed)
        *value = ctx->rf_last_on.load() && ctx->rf_h.valid ? ctx->rf_h[psy::RC_FLAGGED] : 0;
        return TDT_OK;
    }
    AnyDecWS &w = ctx->anydw;
    w.h.refresh();  // (the newest snapshot that has landed; never waits)
    switch (stat) {
        case TDT_STAT_ANY_DEC_LARGE: *value = w.h.valid ? w.h[psy::ADC_LARGE] : 0; return TDT_OK;
        case TDT_STAT_ANY_DEC_BLOCKS: *value = w.h.valid ? w.h[psy::ADC_BLOCKS] : 0; return TDT_OK;
        case TDT_STAT_ANY_DEC_TILES: *value = w.h.valid ? w.h[psy::ADC_TILES] : 0; return TDT_OK;
        case TDT_STAT_ANY_DEC_BUDGET_LARGE: *value = w.lcap; return TDT_OK;
        case TDT_STAT_ANY_DEC_BUDGET_TILES: *value = w.tcap; return TDT_OK;
    }
    return set_err(TDT_E_ARG, "unknown stat");
}

int tdt_should_transform(const tdt_ctx *ctx, uint64_t n) {
    if (n < ctx->cfg.min_tensor_size) return 0;
    if (ctx->cpu.load() > ctx->cfg.cpu_usage_threshold) return 0;
    if (!((n % 4 == 0) && (n >= 64))) return 0;
    return ctx->bandwidth.load() < ctx->cfg.bandwidth_threshold_mbps ? 1 : 0;
}

uint64_t tdt_encode_bound(uint64_t n, int32_t word_size) {
    return psy::encode_bound_of(n, word_size > 0 ? (uint32_t)word_size : 4u, false);
}

uint64_t tdt_ctx_encode_bound(const tdt_ctx *ctx, uint64_t n) {
    if (!ctx) return psy::encode_bound_of(n, 4u, false);
    return psy::encode_bound_of(n, (uint32_t)ctx->cfg.word_size, ctx->raw_fallback);
}

uint64_t tdt_ctx_host_encode_bound(const tdt_ctx *ctx, uint64_t n) {
    if (!ctx) return psy::encode_bound_of(n, 4u, false);
    return psy::encode_bound_of(n, (uint32_t)ctx->cfg.word_size, ctx->host_raw_fallback);
}


// Compacted encode.  Batches of medium messages (none over 64 KiB, >= 16 KiB on average): one
// pass, offsets by the kernels' decoupled look-back.  Batches with longer messages: a message's
// size is known only after its whole analysis, and those take far longer than the rest, so
// successors waiting in the look-back would stall every CU (head-of-line blocking); batches of
// small messages: the per-message ticket / look-back chain bounds the rate.  Both are encoded
// slotted (the message-class kernels), then the lengths are scanned and the blobs gathered.
//
// The two phases, once the host knows the batch's input bytes: the batch `a` (a compacted call's
// fields) slotted into cp_buf, its lengths scanned into a.out_off, its blobs gathered into a.out.
static int encode_two_phase(tdt_ctx *ctx, int mode, const psy::EncodeArgs &a, uint64_t in_bytes, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = a.n_msgs;
    // Σ encode bounds <= 2·(input bytes) + n·(28 + 4·ws) (and >= n + 4 per message)
    const uint64_t bound = 2 * in_bytes + (uint64_t)n * (28 + 4ull * (uint64_t)ctx->cfg.word_size + 4);
    psy::EncodeArgs e = a;  // the slotted call: no compacted output
    e.out_cap = 0;
    e.out_off = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (int st = ensure_cp(ctx, 2ull * n + 2, bound, s)) return st;
        e.out = ctx->cp_buf;
        e.slot_off = ctx->cp_idx;
        e.out_len = ctx->cp_idx + n + 1;
    }
    // (slots of the TDT bound whatever TDT_OPT_RAW_FALLBACK says: this route serves the calls that ignore
    // the option — tdt_encode_batch leaves before it when the option is set)
    hipLaunchKernelGGL(psy::tdt_encode_slots_kernel, dim3((n + 256) / 256), dim3(256), 0, s, a.in_off, ctx->cp_idx, n,
                       (uint32_t)ctx->cfg.word_size);
    HIPCHK(hipGetLastError());
    int st = encode_common(ctx, mode, e, Where(stream));
    if (st) return st;
    if ((st = scan_lengths(ctx, e.out_len, a.out_off, n, s))) return st;
    hipLaunchKernelGGL(cp_gather_kernel, dim3((n + 3) / 4), dim3(256), 0, s, e.out, e.slot_off, e.out_len, a.out, a.out_off,
                       a.out_cap, a.status, n);
    HIPCHK(hipGetLastError());
    return TDT_OK;
}

// Compacted encode at a generic word size (tdt_anyws.h): always the two phases, the generic kernel
// filling the slots.  The scratch is sized by the batch's byte count on the host, so not under
// stream capture (nor with the no-two-phase knob).
static int encode_two_phase_any(tdt_ctx *ctx, int mode, const psy::EncodeArgs &a, void *stream) {
    if (!a.in_off || !a.out || !a.out_off) return set_err(TDT_E_ARG, "null argument");
    if (mode == psy::MODE_MAPPED && !a.mapping_in) return set_err(TDT_E_ARG, "null mapping");
    if (!two_phase_ok(ctx, stream))
        return set_err(TDT_E_UNSUPPORTED, "compacted encode at a word size other than 1, 2, 4, 8, 16 reads the batch "
                                          "size back: not under stream capture or TDT_OPT_NO_TWO_PHASE (use the "
                                          "slotted entry points there)");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    uint64_t h2[2];
    HIPCHK(hipMemcpyAsync(&h2[0], a.in_off, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&h2[1], a.in_off + a.n_msgs, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return encode_two_phase(ctx, mode, a, h2[1] - h2[0], stream);
}

int tdt_encode_batch(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs, uint8_t *d_out,
                     uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status, void *stream) {
    auto a = batch_args<psy::EncodeArgs>(d_in, d_in_off, n_msgs, d_out, d_status);
    a.out_cap = out_cap;
    a.out_off = d_out_off;
    if (ctx && n_msgs && ctx->raw_fallback) return encode_compacted_raw(ctx, a, stream);
    if (ctx) ctx->rf_last_on.store(false);
    if (ctx && n_msgs && psy::anyws_generic(ctx->cfg.word_size)) return encode_two_phase_any(ctx, psy::MODE_ENCODE, a, stream);
    if (!ctx || n_msgs == 0 || !d_in_off || !d_out || !d_out_off || !two_phase_ok(ctx, stream))
        return encode_common(ctx, psy::MODE_ENCODE, a, Where(stream));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    uint64_t h3[3];
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (int st = ensure_cp(ctx, 2ull * n_msgs + 2, 0, s)) return st;  // (the probe's flag word)
        uint64_t *flag = ctx->cp_idx + 2ull * n_msgs + 1;
        HIPCHK(hipMemsetAsync(flag, 0, 8, s));
        hipLaunchKernelGGL(cp_big_kernel, dim3((n_msgs + 255) / 256), dim3(256), 0, s, d_in, d_in_off, n_msgs,
                           (uint64_t)65536, flag);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&h3[0], flag, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&h3[1], d_in_off, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&h3[2], d_in_off + n_msgs, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    // one pass with the look-back for batches of medium messages (all <= 64 KiB, 16 KiB or more
    // on average); small messages make the per-message ticket and look-back chain the limit
    // (C2: 12 ms for 1 Mi x 1 KiB), long ones stall it — both take the two phases
    if (!(h3[0] & 1) && (h3[2] - h3[1]) >= 16384ull * n_msgs) {  // (16 KiB on average: 512-lane teams)
        Where w(stream);
        w.small_teams = (h3[0] & 2) ? 0 : 2;
        return encode_common(ctx, psy::MODE_ENCODE, a, w);
    }
    return encode_two_phase(ctx, psy::MODE_ENCODE, a, h3[2] - h3[1], stream);
}

int tdt_encode_with_mapping_batch(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs,
                                  const int32_t *d_mapping, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off,
                                  int32_t *d_status, void *stream) {
    auto a = batch_args<psy::EncodeArgs>(d_in, d_in_off, n_msgs, d_out, d_status);
    a.mapping_in = d_mapping;
    a.out_cap = out_cap;
    a.out_off = d_out_off;
    if (ctx && n_msgs && psy::anyws_generic(ctx->cfg.word_size)) return encode_two_phase_any(ctx, psy::MODE_MAPPED, a, stream);
    return encode_common(ctx, psy::MODE_MAPPED, a, Where(stream));
}

int tdt_analyze_batch(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs, uint32_t *d_hist,
                      double *d_entropy, int32_t *d_mapping, int32_t *d_status, void *stream) {
    auto a = batch_args<psy::EncodeArgs>(d_in, d_in_off, n_msgs, nullptr, d_status);
    a.hist_out = d_hist;
    a.ent_out = d_entropy;
    a.map_out = d_mapping;
    return encode_common(ctx, psy::MODE_ANALYZE, a, Where(stream));
}

// Compacted decode.  Decoded sizes are in the headers, so the output offsets are computed
// first (sizes + scan) and the blobs decoded by the slotted message-class kernels straight into
// their compacted places (no copy; and no look-back, whose successors stall behind long blobs);
// batches whose total exceeds out_cap take the look-back kernel, which assigns
// TDT_E_CAPACITY per blob.
int tdt_decode_batch(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs, uint8_t *d_out,
                     uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status, void *stream) {
    if (ctx && n_msgs && d_in_off && d_out && d_out_off && two_phase_ok(ctx, stream)) {
        hipStream_t s = (hipStream_t)stream;
        HIPCHK(hipSetDevice(ctx->device));
        int st = tdt_decode_slots(ctx, d_in, d_in_off, nullptr, n_msgs, d_out_off, d_status, stream);
        if (st) return st;
        uint64_t total = 0;
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            if ((st = ensure_cp(ctx, 2ull * n_msgs + 2, 0, s))) return st;  // (the decoded lengths)
            HIPCHK(hipMemcpyAsync(&total, d_out_off + n_msgs, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        if (total <= out_cap)
            return tdt_decode_batch_into(ctx, d_in, d_in_off, nullptr, n_msgs, d_out, d_out_off, ctx->cp_idx, d_status,
                                         stream);
    }
    auto a = batch_args<psy::DecodeArgs>(d_in, d_in_off, n_msgs, d_out, d_status);
    a.out_cap = out_cap;
    a.out_off = d_out_off;
    return decode_common(ctx, false, a, Where(stream));
}

int tdt_decoded_sizes_batch(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs,
                            uint64_t *d_sizes, int32_t *d_status, void *stream) {
    auto a = batch_args<psy::DecodeArgs>(d_in, d_in_off, n_msgs, nullptr, d_status);
    a.sizes_out = d_sizes;
    return decode_common(ctx, true, a, Where(stream));
}

int tdt_encode_batch_into(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs,
                          uint8_t *d_out, const uint64_t *d_slot_off, uint64_t *d_out_len, int32_t *d_status,
                          void *stream) {
    if (n_msgs && !d_slot_off) return set_err(TDT_E_ARG, "null slot offsets");
    if (ctx && ctx->raw_fallback)
        return encode_into_raw(ctx, d_in, d_in_off, n_msgs, d_out, d_slot_off, d_out_len, d_status, stream);
    if (ctx) ctx->rf_last_on.store(false);
    auto a = batch_args<psy::EncodeArgs>(d_in, d_in_off, n_msgs, d_out, d_status);
    a.slot_off = d_slot_off;
    a.out_len = d_out_len;
    return encode_common(ctx, psy::MODE_ENCODE, a, Where(stream));
}

int tdt_decode_batch_into(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, const uint64_t *d_in_len,
                          uint32_t n_msgs, uint8_t *d_out, const uint64_t *d_slot_off, uint64_t *d_out_len,
                          int32_t *d_status, void *stream) {
    if (n_msgs && !d_slot_off) return set_err(TDT_E_ARG, "null slot offsets");
    auto a = batch_args<psy::DecodeArgs>(d_in, d_in_off, n_msgs, d_out, d_status);
    a.in_len = d_in_len;
    a.slot_off = d_slot_off;
    a.out_len = d_out_len;
    return decode_common(ctx, false, a, Where(stream));
}

// A scattered encode: the batch is `v` alone (no base pointers, no offset tables)
static int encode_scattered(tdt_ctx *ctx, const Scatter &v, uint32_t n_msgs, uint64_t *d_out_len, int32_t *d_status,
                            void *stream) {
    psy::EncodeArgs a{};
    a.n_msgs = n_msgs;
    a.status = d_status;
    a.out_len = d_out_len;
    Where w(stream);
    w.v = &v;
    return encode_common(ctx, psy::MODE_ENCODE, a, w);
}

int tdt_encode_batch_v(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes, uint32_t n_msgs,
                       uint8_t *const *d_blobs, const uint64_t *d_blob_cap, uint64_t *d_out_len, int32_t *d_status,
                       void *stream) {
    return encode_v_any(ctx, scatter_of(d_msgs, d_sizes, d_blobs, d_blob_cap), nullptr, 0, n_msgs, d_out_len, d_status,
                        stream, nullptr);
}

int tdt_encode_batch_vw(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes,
                        const int32_t *d_word_size, uint64_t width_mask, uint32_t n_msgs, uint8_t *const *d_blobs,
                        const uint64_t *d_blob_cap, uint64_t *d_out_len, int32_t *d_status, void *stream) {
    static_assert(TDT_MIXED_MAX_WIDTHS == psy::kMixedMaxWidths, "the header states the routes' limit");
    if (ctx && n_msgs && !d_word_size) return set_err(TDT_E_ARG, "null pointer, size or word-size array");
    return encode_v_any(ctx, scatter_of(d_msgs, d_sizes, d_blobs, d_blob_cap), d_word_size, width_mask, n_msgs, d_out_len,
                        d_status, stream, nullptr);
}

// lengths → d_out_off, scanned in place, then the byte-balanced pack kernel (tdt_pack.h)
static int pack_common(tdt_ctx *ctx, const uint64_t *d_blobs, const uint64_t *d_blob_len, uint32_t n_msgs, uint8_t *d_out,
                       uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status, bool keep_errors, hipStream_t s) {
    if (int st = scan_lengths(ctx, d_blob_len, d_out_off, n_msgs, s)) return st;
    HIPCHK((hipError_t)psy::launch_pack(d_blobs, d_out_off, n_msgs, d_out, out_cap, d_status, keep_errors, ctx->pack_cut,
                                        ctx->pack_grid, s));
    return TDT_OK;
}

int tdt_pack_v(tdt_ctx *ctx, const uint8_t *const *d_blobs, const uint64_t *d_blob_len, uint32_t n_msgs, uint8_t *d_out,
               uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status, void *stream) {
    if (!ctx) return set_err(TDT_E_ARG, "null context");
    if (n_msgs == 0) return TDT_OK;
    if (!d_blobs || !d_blob_len || !d_out_off) return set_err(TDT_E_ARG, "null pointer, length or offset array");
    if (!d_out && out_cap) return set_err(TDT_E_ARG, "null output");
    HIPCHK(hipSetDevice(ctx->device));
    return pack_common(ctx, reinterpret_cast<const uint64_t *>(d_blobs), d_blob_len, n_msgs, d_out, out_cap, d_out_off,
                       d_status, false, (hipStream_t)stream);
}

// A scattered known-mapping encode: `v` and the caller's mapping bits (n u64)
static int encode_scattered_mapped(tdt_ctx *ctx, const Scatter &v, uint32_t n_msgs, const uint64_t *d_mapbits,
                                   uint64_t *d_out_len, int32_t *d_status, void *stream) {
    psy::EncodeArgs a{};
    a.n_msgs = n_msgs;
    a.status = d_status;
    a.out_len = d_out_len;
    a.mapping_in = reinterpret_cast<const int32_t *>(d_mapbits);
    Where w(stream);
    w.v = &v;
    return encode_common(ctx, psy::MODE_MAPPED, a, w);
}

// ---------------------------------------------------------------------------------------
// The raw fallback (TDT_OPT_RAW_FALLBACK, tdt_rawfb.h) around the scattered encodes.  Every device-batch
// encode reaches its messages through encode_v_any: option off, the call as it always was; option on,
// the slots clamped to n + 4 in front of it and the flag, scan and copy passes behind it, all on the
// caller's stream.  The host reads nothing back.
static_assert(psy::kRawMarker == psy::kMagicUNCP, "the fallback's blob is the UNCP blob");
struct RawWS {
    unsigned long long *cnt;  // the counter block (RawCount)
    uint64_t *cap, *raw_off, *len, *tab;
    int32_t *status;
};
// rf_buf with room for n messages, under ctx->mu (a buffer a captured graph may point at: retired, not freed)
static int raw_ws(tdt_ctx *ctx, uint32_t n, hipStream_t s, RawWS &w) {
    const size_t words = 7ull * n + 1, need = psy::kPlanCounterBytes + 8 * words + 4ull * n;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int st = grow_retiring(ctx->rf_buf, ctx->rf_bytes, need, psy::cap_double(need, ctx->rf_bytes), ctx->retired, s))
        return st;
    uint64_t *u = reinterpret_cast<uint64_t *>(ctx->rf_buf + psy::kPlanCounterBytes);
    w.cnt = reinterpret_cast<unsigned long long *>(ctx->rf_buf);
    w.cap = u;
    w.raw_off = u + n;
    w.len = u + 2ull * n + 1;
    w.tab = u + 3ull * n + 1;
    w.status = reinterpret_cast<int32_t *>(u + words);
    return TDT_OK;
}
// the scattered encode of every form: one width or one per message, the analysis or the caller's mappings
static int encode_v_plain(tdt_ctx *ctx, const Scatter &v, const int32_t *d_word_size, uint64_t width_mask, uint32_t n,
                          uint64_t *d_out_len, int32_t *d_status, void *stream, const uint64_t *d_mapbits) {
    if (d_word_size)
        return encode_mixed(ctx, v, d_word_size, width_mask, n, d_out_len, d_status, (hipStream_t)stream,
                            d_mapbits ? psy::MODE_MAPPED : psy::MODE_ENCODE, const_cast<uint64_t *>(d_mapbits));
    return d_mapbits ? encode_scattered_mapped(ctx, v, n, d_mapbits, d_out_len, d_status, stream)
                     : encode_scattered(ctx, v, n, d_out_len, d_status, stream);
}
static int encode_v_any(tdt_ctx *ctx, const Scatter &v, const int32_t *d_word_size, uint64_t width_mask, uint32_t n,
                        uint64_t *d_out_len, int32_t *d_status, void *stream, const uint64_t *d_mapbits) {
    if (!ctx) return set_err(TDT_E_ARG, "null context");
    if (!ctx->raw_fallback) {
        ctx->rf_last_on.store(false);
        return encode_v_plain(ctx, v, d_word_size, width_mask, n, d_out_len, d_status, stream, d_mapbits);
    }
    if (n == 0) return TDT_OK;
    if (!(v.ptr && v.size && v.out_ptr && v.out_cap)) return set_err(TDT_E_ARG, "null pointer or size array");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    RawWS w{};
    if (int st = raw_ws(ctx, n, s, w)) return st;
    HIPCHK(hipMemsetAsync(w.cnt, 0, psy::kPlanSnapBytes, s));
    HIPCHK((hipError_t)psy::launch_raw_clamp(v.size, v.out_cap, w.cap, n, s));
    const Scatter vc{v.ptr, v.size, v.out_ptr, w.cap};
    int32_t *status = d_status ? d_status : w.status;
    uint64_t *len = d_out_len ? d_out_len : w.len;
    if (int st = encode_v_plain(ctx, vc, d_word_size, width_mask, n, len, status, stream, d_mapbits)) return st;
    HIPCHK((hipError_t)psy::launch_raw_flag(v.size, v.out_cap, status, len, w.raw_off, w.cnt + psy::RC_FLAGGED, n, s));
    if (int st = scan_sizes(ctx, w.raw_off, n, s)) return st;
    HIPCHK((hipError_t)psy::launch_raw_copy(v.ptr, v.out_ptr, w.raw_off, n, ctx->pack_cut, (uint32_t)ctx->cus * 4u, s));
    ctx->rf_last_on.store(true);
    if (capturing(s)) return TDT_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return record_counts(ctx->rf_h, w.cnt, n, s);
}
// tdt_encode_batch_into under the option: the contiguous batch as a scattered one
static int encode_into_raw(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n, uint8_t *d_out,
                           const uint64_t *d_slot_off, uint64_t *d_out_len, int32_t *d_status, void *stream) {
    if (n == 0) return TDT_OK;
    if (!d_in_off || !d_out || !d_slot_off) return set_err(TDT_E_ARG, "null offsets or output");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    RawWS w{};
    if (int st = raw_ws(ctx, n, s, w)) return st;
    uint64_t *t = w.tab;
    HIPCHK((hipError_t)psy::launch_raw_contig(d_in, d_in_off, d_out, d_slot_off, t, t + n, t + 2ull * n, t + 3ull * n, n, s));
    const Scatter v{t, t + n, t + 2ull * n, t + 3ull * n};
    return encode_v_any(ctx, v, nullptr, 0, n, d_out_len, d_status, stream, nullptr);
}
// tdt_encode_batch under the option: slots of n + 4 bytes in cp_buf, the slotted encode with the
// fallback, the lengths scanned into a.out_off, the blobs gathered into a.out (the one-pass look-back
// publishes a blob's TDT length from inside the kernel, so it cannot serve here)
static int encode_compacted_raw(tdt_ctx *ctx, const psy::EncodeArgs &a, void *stream) {
    if (!a.in_off || !a.out || !a.out_off) return set_err(TDT_E_ARG, "null argument");
    if (!two_phase_ok(ctx, stream))
        return set_err(TDT_E_UNSUPPORTED, "compacted encode under TDT_OPT_RAW_FALLBACK takes the two phases and reads the "
                                          "batch size back: not under stream capture or TDT_OPT_NO_TWO_PHASE (use the "
                                          "slotted or scattered entry points there)");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = a.n_msgs;
    HIPCHK(hipSetDevice(ctx->device));
    uint64_t h2[2];
    HIPCHK(hipMemcpyAsync(&h2[0], a.in_off, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&h2[1], a.in_off + n, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    uint8_t *buf;
    uint64_t *slot, *len;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (int st = ensure_cp(ctx, 2ull * n + 2, (h2[1] - h2[0]) + 4ull * n, s)) return st;
        buf = ctx->cp_buf, slot = ctx->cp_idx, len = ctx->cp_idx + n + 1;
    }
    HIPCHK((hipError_t)psy::launch_raw_slots(a.in_off, slot, n, s));
    if (int st = encode_into_raw(ctx, a.in, a.in_off, n, buf, slot, len, a.status, stream)) return st;
    if (int st = scan_lengths(ctx, len, a.out_off, n, s)) return st;
    hipLaunchKernelGGL(cp_gather_kernel, dim3((n + 3) / 4), dim3(256), 0, s, buf, slot, len, a.out, a.out_off, a.out_cap,
                       a.status, n);
    HIPCHK(hipGetLastError());
    return TDT_OK;
}
// the size routes under the option: min(E, n + 4) behind the size pass (sizes: the scattered sizes, or
// null and in_off the contiguous batch's offsets)
static int raw_min_sizes(tdt_ctx *ctx, const uint64_t *d_sizes, const uint64_t *d_in_off, uint64_t *d_enc, uint32_t n,
                         hipStream_t s) {
    if (!ctx || !ctx->raw_fallback || n == 0) return TDT_OK;
    HIPCHK((hipError_t)psy::launch_raw_min(d_sizes, d_in_off, d_enc, n, s));
    return TDT_OK;
}

// tdt_encode_batch_vp (d_mapbits null) and tdt_encode_mapped_vp (the caller's mapping bits: always the
// two phases — the sizes-first form would need the sizes under the caller's mapping, a size pass
// that takes the mapping instead of deciding it, which the mode parameters do not hold)
static int encode_packed(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes, const int32_t *d_word_size,
                         uint64_t width_mask, uint32_t n_msgs, uint64_t total_bytes, const uint64_t *d_mapbits,
                         uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status, void *stream) {
    if (!d_msgs || !d_sizes || !d_out_off) return set_err(TDT_E_ARG, "null pointer, size or offset array");
    if (!d_out && out_cap) return set_err(TDT_E_ARG, "null output");
    uint64_t wmax = (uint64_t)ctx->cfg.word_size;
    if (d_word_size) {
        psy::MixedRoutes R{};
        if (!psy::mixed_routes(width_mask, n_msgs, R))
            return set_err(TDT_E_ARG, "width_mask must name between 1 and 8 word sizes");
        wmax = 64u - (uint64_t)__builtin_clzll(width_mask);
    }
    if (total_bytes > (1ull << 62)) return set_err(TDT_E_ARG, "total_bytes too large");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    uint64_t *sf_idx = nullptr;  // sizes first: blob addresses (n) | capacities (n) | option value 2: mapping bits (n)
    bool sf_map = false;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (ctx->pack_sizes_first && !d_mapbits) {
            sf_map = ctx->pack_sizes_first == 2;
            if (int st = ensure_cp(ctx, (sf_map ? 3ull : 2ull) * n_msgs, 0, s, true)) return st;
            sf_idx = ctx->cp_idx;
        }
    }
    if (sf_idx) {
        // Sizes first: the exact lengths into d_out_off (the size pass), scanned in place into the
        // offsets, each blob's slot [off[i], off[i+1]) of d_out — capacity 0 where it would end past
        // out_cap — and the scattered / mixed encode straight into those slots.  No scratch: total_bytes
        // plays no part, cp_buf is not touched.
        // Option value 2: the size pass leaves every message's mapping bits behind the two tables (0 for
        // a passthrough or rejected message: the words are zeroed first), and the second pass is the
        // known-mapping encode with them — the same bytes, the analysis run once.
        uint64_t *ptr = sf_idx, *cap = sf_idx + n_msgs, *bits = sf_map ? sf_idx + 2ull * n_msgs : nullptr;
        const uint64_t *msgs = reinterpret_cast<const uint64_t *>(d_msgs);
        const Scatter vs{msgs, d_sizes, d_sizes, d_sizes};  // (the size pass has no outputs: launch_slotted)
        if (bits) HIPCHK(hipMemsetAsync(bits, 0, 8ull * n_msgs, s));
        int st = d_word_size ? encode_mixed(ctx, vs, d_word_size, width_mask, n_msgs, d_out_off, d_status, s, psy::MODE_SIZES, bits)
                             : encoded_sizes_one(ctx, &vs, nullptr, n_msgs, d_out_off, d_status, s, bits);
        if (st) return st;
        // (the raw fallback: the exact slots become min(E, n + 4), and the second pass falls back into them)
        if ((st = raw_min_sizes(ctx, d_sizes, nullptr, d_out_off, n_msgs, s))) return st;
        if ((st = scan_sizes(ctx, d_out_off, n_msgs, s))) return st;
        HIPCHK((hipError_t)psy::launch_pack_exact_slots(d_out_off, d_out, out_cap, ptr, cap, n_msgs, s));
        const Scatter v{msgs, d_sizes, ptr, cap};
        return encode_v_any(ctx, v, d_word_size, width_mask, n_msgs, nullptr, d_status, stream, bits);
    }
    // the scratch: every blob in a slot of its encode bound, Σ bounds <= 2·total_bytes + n·(28 + 4·wmax) —
    // under the raw fallback n + 4 per message, total_bytes + 4·n;
    // the tables: slots (n + 1) | blob addresses (n) | capacities (n) | lengths (n)
    const bool raw = ctx->raw_fallback;
    const uint64_t scratch = raw ? total_bytes + 4ull * n_msgs : 2 * total_bytes + (uint64_t)n_msgs * (28 + 4 * wmax);
    uint8_t *buf;
    uint64_t buf_bytes, *idx;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (int st = ensure_cp(ctx, 4ull * n_msgs + 2, scratch, s, true)) return st;
        buf = ctx->cp_buf, buf_bytes = ctx->cp_bytes, idx = ctx->cp_idx;
    }
    uint64_t *slot = idx, *ptr = idx + n_msgs + 1, *cap = ptr + n_msgs, *len = cap + n_msgs;
    HIPCHK((hipError_t)(raw ? psy::launch_raw_bounds(d_sizes, d_word_size, ctx->cfg.word_size, width_mask, slot, n_msgs, s)
                            : psy::launch_pack_bounds(d_sizes, d_word_size, ctx->cfg.word_size, width_mask, slot, n_msgs, s)));
    if (int st = scan_sizes(ctx, slot, n_msgs, s)) return st;
    // (a slot that would end past the scratch — total_bytes was understated — gets capacity 0:
    // TDT_E_CAPACITY for that message, never a write outside the scratch)
    HIPCHK((hipError_t)psy::launch_pack_slots(slot, buf, buf_bytes, ptr, cap, n_msgs, s));
    const Scatter v{reinterpret_cast<const uint64_t *>(d_msgs), d_sizes, ptr, cap};
    if (int st = encode_v_any(ctx, v, d_word_size, width_mask, n_msgs, len, d_status, stream, d_mapbits)) return st;
    return pack_common(ctx, ptr, len, n_msgs, d_out, out_cap, d_out_off, d_status, true, s);
}

int tdt_encode_batch_vp(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes, const int32_t *d_word_size,
                        uint64_t width_mask, uint32_t n_msgs, uint64_t total_bytes, uint8_t *d_out, uint64_t out_cap,
                        uint64_t *d_out_off, int32_t *d_status, void *stream) {
    if (!ctx) return set_err(TDT_E_ARG, "null context");
    if (n_msgs == 0) return TDT_OK;
    return encode_packed(ctx, d_msgs, d_sizes, d_word_size, width_mask, n_msgs, total_bytes, nullptr, d_out, out_cap,
                         d_out_off, d_status, stream);
}

int tdt_encode_mapped_vp(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes, const int32_t *d_word_size,
                         uint64_t width_mask, uint32_t n_msgs, uint64_t total_bytes, const uint64_t *d_mapbits,
                         uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status, void *stream) {
    if (!ctx) return set_err(TDT_E_ARG, "null context");
    if (n_msgs == 0) return TDT_OK;
    if (!d_mapbits) return set_err(TDT_E_ARG, "null mapping");
    return encode_packed(ctx, d_msgs, d_sizes, d_word_size, width_mask, n_msgs, total_bytes, d_mapbits, d_out, out_cap,
                         d_out_off, d_status, stream);
}

int tdt_encode_mapped_v(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes, const int32_t *d_word_size,
                        uint64_t width_mask, uint32_t n_msgs, const uint64_t *d_mapbits, uint8_t *const *d_blobs,
                        const uint64_t *d_blob_cap, uint64_t *d_out_len, int32_t *d_status, void *stream) {
    if (!ctx) return set_err(TDT_E_ARG, "null context");
    if (n_msgs == 0) return TDT_OK;
    if (!d_mapbits) return set_err(TDT_E_ARG, "null mapping");
    return encode_v_any(ctx, scatter_of(d_msgs, d_sizes, d_blobs, d_blob_cap), d_word_size, width_mask, n_msgs, d_out_len,
                        d_status, stream, d_mapbits);
}

int tdt_mappings_v(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes, const int32_t *d_word_size,
                   uint64_t width_mask, uint32_t n_msgs, uint64_t *d_enc_sizes, uint64_t *d_mapbits, int32_t *d_status,
                   void *stream) {
    if (!ctx) return set_err(TDT_E_ARG, "null context");
    if (n_msgs == 0) return TDT_OK;
    if (!d_enc_sizes || !d_mapbits) return set_err(TDT_E_ARG, "null output array");
    if (d_word_size) {  // (the call-level mask errors before anything is written)
        psy::MixedRoutes R{};
        if (!psy::mixed_routes(width_mask, n_msgs, R))
            return set_err(TDT_E_ARG, "width_mask must name between 1 and 8 word sizes");
    }
    if (!d_msgs || !d_sizes) return set_err(TDT_E_ARG, "null pointer, size or output array");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    // the size pass stores the bits of the messages it compresses; every other one (UNCP, a rejected width) keeps 0
    HIPCHK(hipMemsetAsync(d_mapbits, 0, 8ull * n_msgs, s));
    const uint64_t *msgs = reinterpret_cast<const uint64_t *>(d_msgs);
    const Scatter v{msgs, d_sizes, d_sizes, d_sizes};  // (the size pass has no outputs: launch_slotted)
    const int st = !d_word_size ? encoded_sizes_one(ctx, &v, nullptr, n_msgs, d_enc_sizes, d_status, s, d_mapbits)
                                : encode_mixed(ctx, v, d_word_size, width_mask, n_msgs, d_enc_sizes, d_status, s,
                                               psy::MODE_SIZES, d_mapbits);
    // (the raw fallback lowers the sizes alone: d_mapbits[i] stays the mapping the analysis decided)
    return st ? st : raw_min_sizes(ctx, d_sizes, nullptr, d_enc_sizes, n_msgs, s);
}

int tdt_encoded_sizes_batch(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, uint32_t n_msgs,
                            uint64_t *d_enc_sizes, int32_t *d_status, void *stream) {
    const Contig g{d_in, d_in_off};
    const int st = encoded_sizes_one(ctx, nullptr, &g, n_msgs, d_enc_sizes, d_status, (hipStream_t)stream);
    return st ? st : raw_min_sizes(ctx, nullptr, d_in_off, d_enc_sizes, n_msgs, (hipStream_t)stream);
}

int tdt_encoded_sizes_v(tdt_ctx *ctx, const uint8_t *const *d_msgs, const uint64_t *d_sizes, const int32_t *d_word_size,
                        uint64_t width_mask, uint32_t n_msgs, uint64_t *d_enc_sizes, int32_t *d_status, void *stream) {
    const uint64_t *msgs = reinterpret_cast<const uint64_t *>(d_msgs);
    const Scatter v{msgs, d_sizes, d_sizes, d_sizes};  // (the size pass has no outputs: launch_slotted)
    if (d_word_size && ctx && n_msgs && !d_enc_sizes) return set_err(TDT_E_ARG, "null output array");
    const int st = !d_word_size ? encoded_sizes_one(ctx, &v, nullptr, n_msgs, d_enc_sizes, d_status, (hipStream_t)stream)
                                : encode_mixed(ctx, v, d_word_size, width_mask, n_msgs, d_enc_sizes, d_status,
                                               (hipStream_t)stream, psy::MODE_SIZES);
    return st ? st : raw_min_sizes(ctx, d_sizes, nullptr, d_enc_sizes, n_msgs, (hipStream_t)stream);
}

int tdt_decode_batch_v(tdt_ctx *ctx, const uint8_t *const *d_blobs, const uint64_t *d_blob_len, uint32_t n_msgs,
                       uint8_t *const *d_outs, const uint64_t *d_out_cap, uint64_t *d_out_len, int32_t *d_status,
                       void *stream) {
    const Scatter v = scatter_of(d_blobs, d_blob_len, d_outs, d_out_cap);
    psy::DecodeArgs a{};  // (the blobs through in_off / in_len as they are)
    a.in_off = v.ptr;
    a.in_len = d_blob_len;
    a.n_msgs = n_msgs;
    a.status = d_status;
    a.out_len = d_out_len;
    Where w(stream);
    w.v = &v;
    return decode_common(ctx, false, a, w);
}

int tdt_decoded_sizes_v(tdt_ctx *ctx, const uint8_t *const *d_blobs, const uint64_t *d_blob_len, uint32_t n_msgs,
                        uint64_t *d_sizes, int32_t *d_status, void *stream) {
    if (n_msgs && !d_blob_len) return set_err(TDT_E_ARG, "null blob lengths");
    auto a = batch_args<psy::DecodeArgs>(nullptr, reinterpret_cast<const uint64_t *>(d_blobs), n_msgs, nullptr, d_status);
    a.in_len = d_blob_len;
    a.sizes_out = d_sizes;
    return decode_common(ctx, true, a, Where(stream));
}

int tdt_encode_slots(tdt_ctx *ctx, const uint64_t *d_in_off, uint32_t n_msgs, uint64_t *d_slot_off, void *stream) {
    if (!ctx) return set_err(TDT_E_ARG, "null context");
    if (!d_slot_off || (n_msgs && !d_in_off)) return set_err(TDT_E_ARG, "null offsets");
    HIPCHK(hipSetDevice(ctx->device));
    if (n_msgs == 0) {  // d_in_off may be null for an empty batch
        HIPCHK(hipMemsetAsync(d_slot_off, 0, 8, (hipStream_t)stream));
        return TDT_OK;
    }
    if (ctx->raw_fallback) {  // n + 4 per message
        HIPCHK((hipError_t)psy::launch_raw_slots(d_in_off, d_slot_off, n_msgs, (hipStream_t)stream));
        return TDT_OK;
    }
    hipLaunchKernelGGL(psy::tdt_encode_slots_kernel, dim3((n_msgs + 256) / 256), dim3(256), 0, (hipStream_t)stream,
                       d_in_off, d_slot_off, n_msgs, (uint32_t)ctx->cfg.word_size);
    HIPCHK(hipGetLastError());
    return TDT_OK;
}

int tdt_decode_slots(tdt_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, const uint64_t *d_in_len,
                     uint32_t n_msgs, uint64_t *d_slot_off, int32_t *d_status, void *stream) {
    if (!ctx) return set_err(TDT_E_ARG, "null context");
    if (!d_slot_off) return set_err(TDT_E_ARG, "null offsets");
    if (n_msgs) {
        auto a = batch_args<psy::DecodeArgs>(d_in, d_in_off, n_msgs, nullptr, d_status);
        a.in_len = d_in_len;
        a.sizes_out = d_slot_off;
        if (int st = decode_common(ctx, true, a, Where(stream))) return st;
    }
    HIPCHK(hipSetDevice(ctx->device));
    return scan_sizes(ctx, d_slot_off, n_msgs, (hipStream_t)stream);
}


int tdt_encode_host(tdt_ctx *ctx, const uint8_t *h_in, const uint64_t *h_in_off, uint32_t n_msgs, uint8_t *h_out,
                    uint64_t out_cap, uint64_t *h_out_off, int32_t *h_status) {
    return host_path(ctx, true, h_in, h_in_off, n_msgs, h_out, out_cap, h_out_off, h_status);
}

int tdt_decode_host(tdt_ctx *ctx, const uint8_t *h_in, const uint64_t *h_in_off, uint32_t n_msgs, uint8_t *h_out,
                    uint64_t out_cap, uint64_t *h_out_off, int32_t *h_status) {
    return host_path(ctx, false, h_in, h_in_off, n_msgs, h_out, out_cap, h_out_off, h_status);
}

int tdt_encode_host_v(tdt_ctx *ctx, const uint8_t *const *msgs, const uint64_t *sizes, uint32_t n_msgs, uint8_t *h_out,
                      uint64_t out_cap, uint64_t *h_out_off, int32_t *h_status) {
    if (!ctx) return set_err(TDT_E_ARG, "null context");
    if (n_msgs == 0) {
        if (h_out_off) h_out_off[0] = 0;
        return TDT_OK;
    }
    if (!msgs || !sizes || !h_out_off) return set_err(TDT_E_ARG, "null argument");
    if (n_msgs == 1) {
        const uint64_t off[2] = {0, sizes[0]};
        return host_path(ctx, true, msgs[0], off, 1, h_out, out_cap, h_out_off, h_status);
    }
    std::vector<uint64_t> voff(n_msgs + 1, 0);
    for (uint32_t i = 0; i < n_msgs; ++i) voff[i + 1] = voff[i] + sizes[i];
    return host_path(ctx, true, nullptr, voff.data(), n_msgs, h_out, out_cap, h_out_off, h_status, msgs, sizes);
}

int tdt_host_alloc(uint64_t bytes, void **ptr) {
    if (!ptr) return set_err(TDT_E_ARG, "null argument");
    *ptr = nullptr;
    HIPCHK(hipHostMalloc(ptr, std::max<uint64_t>(bytes, 1), hipHostMallocDefault));
    return TDT_OK;
}

void tdt_host_free(void *ptr) {
    if (ptr) (void)hipHostFree(ptr);
}

int tdt_host_copy(tdt_ctx *ctx, void *dst, const void *src, uint64_t bytes) {
    if (!ctx || (bytes && (!dst || !src))) return set_err(TDT_E_ARG, "null argument");
    std::shared_ptr<CopyPool> pool;
    {
        std::lock_guard<std::mutex> lk(ctx->hmu);  // (the pool is created and replaced under hmu)
        if (!ctx->pool) ctx->pool.reset(new CopyPool(ctx->copy_threads));
        pool = ctx->pool;
    }
    pool->copy(dst, src, bytes);  // (outside hmu: CopyPool::copy serialises concurrent callers itself)
    return TDT_OK;
}

int tdt_ctx_error_flags(tdt_ctx *ctx, void *stream, uint32_t *flags) {
    if (!ctx || !flags) return set_err(TDT_E_ARG, "null argument");
    *flags = ctx->host_flags.load();
    if (!ctx->ws) return TDT_OK;
    HIPCHK(hipSetDevice(ctx->device));
    // stream-ordered read of the flag word: waits for the batches issued on `stream` only
    uint32_t f = 0;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(&f, ctx->ws + 4, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *flags |= f;
    return TDT_OK;
}

int tdt_analyze_host(tdt_ctx *ctx, const uint8_t *h_in, const uint64_t *h_in_off, uint32_t n_msgs, double *h_entropy,
                     int32_t *h_mapping, int32_t *h_status) {
    if (!ctx) return set_err(TDT_E_ARG, "null context");
    if (n_msgs == 0) return TDT_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t in_bytes = h_in_off[n_msgs] - h_in_off[0];
    const size_t ws = (size_t)ctx->cfg.word_size;
    const size_t o_off = align_up(in_bytes, 256);
    const size_t o_ent = align_up(o_off + 8ull * (n_msgs + 1), 256);
    const size_t o_map = align_up(o_ent + 8ull * n_msgs * ws, 256);
    const size_t o_st = align_up(o_map + 4ull * n_msgs * ws, 256);
    const size_t total = align_up(o_st + 4ull * n_msgs, 256);
    // h_dev and astream belong to the host paths (hmu, held for the whole call, so a second
    // caller cannot reallocate h_dev under this one); encode_common then takes mu: the lock
    // order everywhere is hmu, then mu
    std::lock_guard<std::mutex> hl(ctx->hmu);
    int st = ensure_host_dev(ctx, total);
    if (st) return st;
    uint8_t *d = ctx->h_dev;
    std::vector<uint64_t> tmp(n_msgs + 1);
    for (uint32_t i = 0; i <= n_msgs; ++i) tmp[i] = h_in_off[i] - h_in_off[0];
    // on the context's own stream (synchronising that stream only, not the device)
    if (!ctx->astream) HIPCHK(hipStreamCreateWithFlags(&ctx->astream, hipStreamNonBlocking));
    hipStream_t s = ctx->astream;
    HIPCHK(hipMemcpyAsync(d, h_in + h_in_off[0], in_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d + o_off, tmp.data(), 8ull * (n_msgs + 1), hipMemcpyHostToDevice, s));
    auto a = batch_args<psy::EncodeArgs>(d, reinterpret_cast<uint64_t *>(d + o_off), n_msgs, nullptr,
                                         reinterpret_cast<int32_t *>(d + o_st));
    a.ent_out = reinterpret_cast<double *>(d + o_ent);
    a.map_out = reinterpret_cast<int32_t *>(d + o_map);
    Where w(s);
    w.small_teams = in_bytes <= kSmallMax * n_msgs ? 1 : 0;
    st = encode_common(ctx, psy::MODE_ANALYZE, a, w);
    if (st) return st;
    if (h_entropy) HIPCHK(hipMemcpyAsync(h_entropy, d + o_ent, 8ull * n_msgs * ws, hipMemcpyDeviceToHost, s));
    if (h_mapping) HIPCHK(hipMemcpyAsync(h_mapping, d + o_map, 4ull * n_msgs * ws, hipMemcpyDeviceToHost, s));
    if (h_status) HIPCHK(hipMemcpyAsync(h_status, d + o_st, 4ull * n_msgs, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TDT_OK;
}

const char *tdt_last_error(void) { return g_err.c_str(); }

const char *tdt_status_string(int status) {
    switch (status) {
        case TDT_OK: return "OK";
        case TDT_E_SHORT: return "TDT: Invalid encoded data size";
        case TDT_E_MAGIC: return "Invalid TDT magic number";
        case TDT_E_TRUNCATED: return "TDT: truncated blob";
        case TDT_E_BAD_MAPPING: return "TDT: invalid cluster mapping";
        case TDT_E_CAPACITY: return "TDT: output capacity exceeded";
        case TDT_E_UNSUPPORTED: return "TDT: word size not supported on the GPU path";  // (> 64)
        case TDT_E_BAD_HEADER: return "TDT: word size 0";
        case TDT_E_CONFIG: return "TDT: invalid configuration";
        case TDT_E_HIP: return "TDT: HIP runtime error";
        case TDT_E_CAPTURE: return "TDT: workspace growth needed under stream capture";
        case TDT_E_ARG: return "TDT: invalid argument";
    }
    return "TDT: unknown status";
}

#if defined(PSY_PROF) && PSY_PROF
// diagnostic builds only: read and clear the phase-cycle counters
int tdt_prof_read(uint64_t *out32) {
    if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(psy::psy_prof), 32 * sizeof(uint64_t)) != hipSuccess) return TDT_E_HIP;
    static const uint64_t zero[32] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(psy::psy_prof), zero, sizeof(zero)) != hipSuccess) return TDT_E_HIP;
    return TDT_OK;
}
#endif
}  // extern "C"

// In-place exclusive scan of n sizes (u64) at d_off; d_off[n] = the total.
static int scan_sizes(tdt_ctx *ctx, uint64_t *d_slot_off, uint32_t n_msgs, hipStream_t stream) {
    const uint32_t nb = (n_msgs + psy::kSlotChunk - 1) / psy::kSlotChunk;
    if (nb > 1) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (int st = grow_retiring(ctx->slot_sums, ctx->slot_sums_n, nb, psy::cap_exact(nb, ctx->slot_sums_n), ctx->retired,
                                   stream, 8))
            return st;
        hipLaunchKernelGGL(psy::tdt_slot_sums_kernel, dim3(nb - 1), dim3(psy::kSlotThreads), 0, (hipStream_t)stream,
                           d_slot_off, ctx->slot_sums, n_msgs);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(psy::tdt_slot_scan_kernel, dim3(nb ? nb : 1), dim3(psy::kSlotThreads), 0, (hipStream_t)stream,
                       d_slot_off, nb > 1 ? ctx->slot_sums : nullptr, n_msgs);
    HIPCHK(hipGetLastError());
    return TDT_OK;
}

