// tdt_entropy.h — the exact entropy chain of one byte position, shared by the kernels that decide a
// mapping from whole-message histograms on one wave (tdt_anyws.hip, tdt_enc_narrow.hip).
//
// Include it last: the mapping decision is bit-exact only if nothing below is contracted
// (tdt_log2.h), and the pragma holds to the end of the translation unit.
#pragma once
#include "tdt_encode.h"

#pragma clang fp contract(off)

namespace psy {

// The entropy of one byte position (calculate_entropy :470-480): the exact chain only.  Lane l of
// a wave holds the counts of bins l, l + 64, l + 128, l + 192 and computes their (-prob, log2 prob)
// (0, 0 for an empty bin: fma(0, 0, e) == e for the non-negative running sum), then every lane
// runs the chain over the bins in order 0..255.
__device__ __forceinline__ double any_entropy(const uint32_t (&c)[4], double total) {
    double np[4], L[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        np[k] = 0.0;
        L[k] = 0.0;
        if (c[k]) {
            const double prob = (double)c[k] / total;
            L[k] = psy_log2_glibc(prob, c_log2_tab, c_log2_tab2);
            np[k] = -prob;
        }
    }
    double e = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int l = 0; l < 64; ++l) e = __builtin_fma(readlane_f64(np[k], l), readlane_f64(L[k], l), e);
    return e;
}

}  // namespace psy
