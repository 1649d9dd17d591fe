// tdt_dec_reduce.hip — the decode-reduce kernels (tdt_decode_reduce_v, tdt_dec_reduce.h): one instance
// per workgroup size, explicitly instantiated in a translation unit of their own so that
// psyne_amd/build.py compiles them in parallel with the others.
// (the headers' non-template kernels are defined once, in tdt_api.hip)
#define PSY_ENC_INST_TU 1
#define PSY_DEC_INST_TU 1
#define PSY_DEC_REDUCE_TU 1  // (tdt_decode_reduce_serial_kernel is defined here)
#include <hip/hip_runtime.h>

#include "tdt_dec_reduce.h"

#define PSY_DEC_REDUCE_DEF(...) template __global__ void __VA_ARGS__(psy::ReduceArgs);
PSY_DEC_REDUCE_INSTANCES(PSY_DEC_REDUCE_DEF)
