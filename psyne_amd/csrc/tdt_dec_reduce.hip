// tdt_dec_reduce.hip — the decode-reduce kernels (tdt_decode_reduce_v, tdt_dec_reduce.h) and their
// tiled form (tdt_dec_reduce_tiled.h): one instance per workgroup size, explicitly instantiated in a
// translation unit of their own so that psyne_amd/build.py compiles them in parallel with the others.
// (the headers' non-template kernels are defined once, in tdt_api.hip)
#define PSY_ENC_INST_TU 1
#define PSY_DEC_INST_TU 1
#define PSY_DEC_REDUCE_TU 1  // (the serial kernel and the tiled form's plan, block and scan kernels are defined here)
#include <hip/hip_runtime.h>

#include "tdt_dec_reduce_tiled.h"

#define PSY_DEC_REDUCE_DEF(...) template __global__ void __VA_ARGS__(psy::ReduceArgs);
PSY_DEC_REDUCE_INSTANCES(PSY_DEC_REDUCE_DEF)
#define PSY_DEC_REDUCE_TILED_DEF(...) template __global__ void __VA_ARGS__(psy::RedTiledArgs);
PSY_DEC_REDUCE_TILED_INSTANCES(PSY_DEC_REDUCE_TILED_DEF)
