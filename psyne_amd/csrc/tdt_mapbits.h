// tdt_mapbits.h — the mapping bits of the known-mapping calls (tdt_mappings_v, tdt_encode_mapped_v /
// _vp): one u64 per message, bit p = the stream (0 or 1) of byte position p, for p < word_size — the
// encoding of LMeta::mapbits and M_MAPBITS, widened to 64 positions so that one word per message
// describes a mixed-width list.  Plain C++, no HIP types: the kernels, the host and the stand-alone
// test driver (tests/cpp/test_mapbits.cpp) share it.
#pragma once
#include <cstdint>

namespace psy {

// a caller's mapping is usable at width ws: the width is one the codec has, and no bit at or above
// it is set (a set bit there would name a byte position the words do not have: TDT_E_BAD_MAPPING)
constexpr bool mapbits_ok(uint64_t bits, int ws) {
    return ws >= 1 && ws <= 64 && (ws == 64 || (bits >> ws) == 0);
}

// the stream of byte position p under `bits`
constexpr uint32_t mapbits_at(uint64_t bits, int p) { return (uint32_t)((bits >> p) & 1u); }

// the complement of `bits` within the width (every position takes the other stream)
constexpr uint64_t mapbits_flip(uint64_t bits, int ws) {
    return ~bits & (ws >= 64 ? ~0ull : ((1ull << ws) - 1ull));
}

}  // namespace psy
