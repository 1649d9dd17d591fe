// tdt_enc_mapped_ws.hip — the known-mapping encode kernels of the scattered batches (MODE_MAPPED,
// PAIR: tdt_encode_mapped_v / _vp) of ONE word size (PSY_INST_WS), explicitly instantiated as
// tdt_enc_ws.hip does for the encode: psyne_amd/build.py compiles this file once per tuned word
// size, in parallel with the other translation units.
#define PSY_ENC_INST_TU 1
#include <hip/hip_runtime.h>

#include "tdt_encode.h"

#ifndef PSY_INST_WS
#error "PSY_INST_WS (the word size) must be defined"
#endif

#define PSY_ENC_MAPPED_DEF(WS, T, G, TL, PS, PA) \
    template __global__ void psy::tdt_encode_kernel<WS, T, G, psy::MODE_MAPPED, 0, TL, PS, PA, true>(psy::EncodeArgs);
PSY_ENC_MAPPED_INSTANCES(PSY_ENC_MAPPED_DEF, PSY_INST_WS)
