// tdt_enc_sizes_ws.hip — the size-pass kernels (MODE_SIZES) of ONE word size (PSY_INST_WS),
// explicitly instantiated as tdt_enc_ws.hip does for the encode: psyne_amd/build.py compiles this
// file once per tuned word size, in parallel with the other translation units.
#define PSY_ENC_INST_TU 1
#include <hip/hip_runtime.h>

#include "tdt_encode.h"

#ifndef PSY_INST_WS
#error "PSY_INST_WS (the word size) must be defined"
#endif

#define PSY_ENC_SIZES_DEF(WS, T, G, TL, PS, PA) \
    template __global__ void psy::tdt_encode_kernel<WS, T, G, psy::MODE_SIZES, 0, TL, PS, PA, true>(psy::EncodeArgs);
PSY_ENC_SIZES_INSTANCES(PSY_ENC_SIZES_DEF, PSY_INST_WS)
template __global__ void psy::tdt_encode_lscan_sizes_kernel<PSY_INST_WS>(psy::EncodeArgs, const uint32_t *, uint32_t);
