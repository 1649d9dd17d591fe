// tdt_dec_acc.hip — the decode-accumulate kernels (tdt_decode_accumulate_v): the ACC instances of
// the scattered decode's kernels (tdt_decode.h), explicitly instantiated in a translation unit of
// their own so that psyne_amd/build.py compiles them in parallel with the others.
// (the headers' non-template kernels are defined once, in tdt_api.hip)
#define PSY_ENC_INST_TU 1
#define PSY_DEC_INST_TU 1
#include <hip/hip_runtime.h>

#include "tdt_decode.h"

#define PSY_DEC_ACC_DEF(...) template __global__ void __VA_ARGS__(psy::DecodeArgs);
PSY_DEC_ACC_INSTANCES(PSY_DEC_ACC_DEF)
