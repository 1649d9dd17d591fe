// tdt_plan.h — what the slotted calls' plan kernels, class kernels and host launchers share:
// the names of the plan counters and the layout of the plan buffer.  Plain C++, no HIP types.
#pragma once
#include <cstddef>
#include <cstdint>

namespace psy {

// The counter block at the head of the plan buffer, by u64 index: the plan kernel claims list and
// record ranges from the counters, the class kernels read a low word as a list length, and the host
// reads it one call later (the pinned snapshot) to size grids and switch classes on and off.
enum EncCount : int {
    EC_SMALL = 0,        // small messages, listed
    EC_MEDIUM = 1,       // medium messages, listed
    EC_LARGE = 2,        // large-message entries claimed
    EC_TILES = 3,        // tiles claimed
    EC_SPANS = 4,        // spans claimed
    EC_SMALL_ALL = 5,    // small messages, listed or not (switches the small class back on)
    EC_MID = 6,          // mid-sized messages, listed
    EC_MID_ALL = 7,      // mid-sized messages, listed or not
    EC_BIG = 8,          // medium messages over big_min (their own list, dispatched first)
    EC_UNCP_ALL = 9,     // passthrough (UNCP) messages up to large_min, listed or not
    EC_UNCP = 10,        // UNCP messages, listed (the copy list)
    EC_RECOUNT = 11,     // tiles the map pass listed for the count pass
    EC_BYTES = 12        // scattered batches: the sum of the message sizes, by the table kernel (the highest)
};
enum DecCount : int {
    DC_MAIN = 0,         // one-wave blobs (the main list)
    DC_LARGE = 1,        // large blobs claimed
    DC_TILES = 2,        // tiles claimed
    DC_BLOCKS = 3,       // block slots claimed
    DC_SMALL = 4,        // small blobs, listed
    DC_SMALL_ALL = 5,    // small blobs, listed or not (switches the small list back on)
    DC_BIG = 6,          // big one-wave blobs (their own list, dispatched first)
    DC_UNCP_ALL = 7,     // UNCP blobs, listed or not
    DC_UNCP = 8,         // UNCP blobs, listed (the copy list)
    DC_BYTES = 9,        // scattered batches: the sum of the blob lengths, by the table kernel
    DC_DEFERRED = 15     // blobs of a generic word size the class kernels deferred (the highest)
};

// The tiled generic-width encode (tdt_anyws.h) keeps a counter block of its own, one per context.
// A mixed-width call zeroes it once and every generic width of the call claims from it in turn.
enum AnyCount : int {
    AC_LARGE = 0,        // large-message records claimed (beyond the budget too: the next call grows it)
    AC_TILES = 1,        // tile records claimed (likewise)
    AC_BYTES = 2         // pair tables: the sum of the message sizes; a mixed-width call: AC_BYTES + route index
};

// The tiled generic-width decode (tdt_anyws.h) likewise: zeroed before the plan of a call that runs it.
enum AnyDecCount : int {
    ADC_LARGE = 0,       // long-blob records claimed (beyond the budget too: the next call grows it)
    ADC_BLOCKS = 1,      // block sums claimed (likewise)
    ADC_TILES = 2        // tiles claimed (likewise)
};

// u32 view of the block: index of a counter's low word (the only place the two units meet)
constexpr int lo32(EncCount k) { return 2 * (int)k; }
constexpr int lo32(DecCount k) { return 2 * (int)k; }
constexpr int lo32(AnyCount k) { return 2 * (int)k; }
constexpr int lo32(AnyDecCount k) { return 2 * (int)k; }

constexpr size_t kPlanCounterBytes = 256;  // the block
constexpr size_t kPlanSnapBytes = 128;     // zeroed per call and copied to the host's snapshot
static_assert(kPlanSnapBytes <= kPlanCounterBytes, "the snapshot is a prefix of the block");
static_assert(8 * (EC_BYTES + 1) <= kPlanSnapBytes && 8 * (DC_DEFERRED + 1) <= kPlanSnapBytes,
              "every counter is zeroed per call and snapshotted");

// The lists behind the counters, n u32 entries each, in buffer order.
enum EncList : int { EL_SMALL, EL_MEDIUM, EL_MID, EL_BIG, EL_COPY };
enum DecList : int { DL_MAIN, DL_SMALL, DL_BIG, DL_COPY, DL_DEFERRED };
constexpr int kPlanLists = 5;

// Index of message i's begin (k = 0) or end (k = 1) in an offset table: the n + 1 offsets of a
// contiguous batch, message i = [off[i], off[i + 1]), or — PAIR, the scattered batches' kernel
// instances — (begin, end) pairs, message i = [off[2i], off[2i + 1]).
template <bool PAIR>
constexpr uint64_t table_at(uint32_t i, uint32_t k) {
    return PAIR ? 2ull * i + k : (uint64_t)(i + k);
}

// The (begin, end) tables of a scattered batch (the *_v calls), written by the table kernel from the
// caller's pointer and size arrays: 2 * n u64 each, behind the lists.
enum PairTable : int { PT_IN, PT_OUT };  // message bytes (encode only) | output slots
constexpr int kPlanPairs = 2;

// The plan buffer of a batch of n messages: counters | five lists (256 + 20 * n bytes), and for a
// scattered batch | two pair tables (16-byte aligned, 32 * n bytes more).
struct PlanLayout {
    size_t list[kPlanLists];  // byte offsets
    size_t pair[kPlanPairs];  // (0: a contiguous batch has none)
    size_t bytes;
};
constexpr PlanLayout plan_layout(uint32_t n, bool scattered = false) {
    PlanLayout L{};
    for (int i = 0; i < kPlanLists; ++i) L.list[i] = kPlanCounterBytes + 4ull * n * i;
    L.bytes = kPlanCounterBytes + 4ull * n * kPlanLists;
    if (scattered) {
        L.bytes = (L.bytes + 15) & ~(size_t)15;
        for (int i = 0; i < kPlanPairs; ++i) L.pair[i] = L.bytes + 16ull * n * i;
        L.bytes += 16ull * n * kPlanPairs;
    }
    return L;
}

// ------------------------------------------------------------------ mixed word sizes
// tdt_encode_batch_vw: one scattered batch, one record width per message.  The route kernel writes
// one pair of tables per width of the caller's mask; a message of another width (or a rejected
// one) gets the ABSENT entry there.  No message equals it: a real entry has begin <= end.  The
// PAIR plan kernel lists and counts an absent entry nowhere, and the generic encode's workgroup
// for it exits at once, so each width's pipeline touches its own messages only.
constexpr uint64_t kAbsentBegin = ~0ull, kAbsentEnd = 0;
constexpr bool pair_absent(uint64_t begin, uint64_t end) { return begin == kAbsentBegin && end == kAbsentEnd; }

constexpr int kMixedMaxWidths = 8;  // widths per call (TDT_MIXED_MAX_WIDTHS): the workspace and launch bound
static_assert(8 * (AC_BYTES + kMixedMaxWidths) <= kPlanSnapBytes, "one byte counter per width of a mixed call");
constexpr int kMixedWsMax = 64;     // widest record (kAnyWsMax)
constexpr bool mixed_tuned(int ws) { return ws == 1 || ws == 2 || ws == 4 || ws == 8 || ws == 16; }

// What a width mask (bit w - 1: width w may occur) launches: its widths in ascending order, each
// with the byte offsets of its two pair tables (2 * n u64 each, 16-byte aligned) in the call's
// table workspace.  A tuned width runs the slotted pipeline over its tables, a generic one the
// generic encode.
struct MixedRoute {
    int ws;
    bool tuned;
    size_t pair[kPlanPairs];  // byte offsets of the PT_IN / PT_OUT tables
};
struct MixedRoutes {
    int n_routes, n_tuned, n_generic;
    MixedRoute route[kMixedMaxWidths];
    size_t bytes;  // the table workspace: 32 bytes per message and width
};
// false: an empty mask, or more than kMixedMaxWidths widths (`r` is then empty)
constexpr bool mixed_routes(uint64_t mask, uint32_t n, MixedRoutes &r) {
    r = MixedRoutes{};
    int bits = 0;
    for (int w = 1; w <= kMixedWsMax; ++w) bits += (int)((mask >> (w - 1)) & 1u);
    if (bits == 0 || bits > kMixedMaxWidths) return false;
    for (int w = 1; w <= kMixedWsMax; ++w) {
        if (!((mask >> (w - 1)) & 1u)) continue;
        MixedRoute &q = r.route[r.n_routes++];
        q.ws = w;
        q.tuned = mixed_tuned(w);
        (q.tuned ? r.n_tuned : r.n_generic)++;
        for (int i = 0; i < kPlanPairs; ++i) {
            q.pair[i] = r.bytes;
            r.bytes += 16ull * n;
        }
    }
    return true;
}
// route index of width `ws` in `r`, or -1
constexpr int mixed_route_of(const MixedRoutes &r, int ws) {
    for (int i = 0; i < r.n_routes; ++i)
        if (r.route[i].ws == ws) return i;
    return -1;
}

}  // namespace psy
