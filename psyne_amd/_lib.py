"""ctypes binding of include/psyne_tdt.h (libpsyne_tdt.so, built in-tree).

There is no CPU fallback: if the HIP library is missing or no GPU is present, the codec
raises.  Pointers passed to the batch entry points are device pointers.
"""
from __future__ import annotations

import ctypes as C
import os
import pathlib

LIB_PATH = pathlib.Path(__file__).resolve().parent / "libpsyne_tdt.so"

TDT_OK, TDT_E_SHORT, TDT_E_MAGIC, TDT_E_TRUNCATED, TDT_E_BAD_MAPPING = 0, 1, 2, 3, 4
TDT_E_CAPACITY, TDT_E_UNSUPPORTED, TDT_E_BAD_HEADER, TDT_E_CONFIG = 5, 6, 7, 8
TDT_E_HIP, TDT_E_ARG, TDT_E_CAPTURE = 10, 11, 12
TDT_OPT_LARGE_MIN, TDT_OPT_TILE_CAP, TDT_OPT_NO_SIDE_STREAM = 1, 2, 3
TDT_OPT_SMALL_ON_CALLER_STREAM, TDT_OPT_NO_TWO_PHASE, TDT_OPT_COPY_THREADS = 4, 5, 6
TDT_OPT_PACK_SIZES_FIRST = 7
TDT_OPT_ANY_TILED = 8  # generic word sizes: long messages as tiles (default 1); 0: one workgroup per message
TDT_OPT_ANY_DEC_TILED = 9  # generic word sizes: long blobs decoded as 32 KiB tiles (default 1); 0: one workgroup per blob
TDT_OPT_RAW_FALLBACK = 10  # 1: a message whose TDT blob would exceed n + 4 bytes is stored as its UNCP blob (default 0)
TDT_OPT_HOST_RAW_FALLBACK = 11  # 1: the same rule for the host calls (tdt_encode_host / _v); independent of option 10
# tdt_ctx_get_stat: the generic-width decode plan's claims of the last call whose snapshot landed, and the budgets
TDT_STAT_ANY_DEC_LARGE, TDT_STAT_ANY_DEC_BLOCKS, TDT_STAT_ANY_DEC_TILES = 1, 2, 3
TDT_STAT_ANY_DEC_BUDGET_LARGE, TDT_STAT_ANY_DEC_BUDGET_TILES = 4, 5
TDT_STAT_RAW_FALLBACKS = 6  # messages the last device-batch encode stored raw by TDT_OPT_RAW_FALLBACK's rule
TDT_STAT_PACK_SCRATCH_BYTES = 7  # bytes of the context's two-phase scratch (sized exactly by the largest call so far)
TDT_STAT_HOST_RAW_FALLBACKS = 8  # messages the last host encode call stored raw by TDT_OPT_HOST_RAW_FALLBACK's rule
STATS = {"ANY_DEC_LARGE": TDT_STAT_ANY_DEC_LARGE, "ANY_DEC_BLOCKS": TDT_STAT_ANY_DEC_BLOCKS,
         "ANY_DEC_TILES": TDT_STAT_ANY_DEC_TILES, "ANY_DEC_BUDGET_LARGE": TDT_STAT_ANY_DEC_BUDGET_LARGE,
         "ANY_DEC_BUDGET_TILES": TDT_STAT_ANY_DEC_BUDGET_TILES, "RAW_FALLBACKS": TDT_STAT_RAW_FALLBACKS,
         "PACK_SCRATCH_BYTES": TDT_STAT_PACK_SCRATCH_BYTES, "HOST_RAW_FALLBACKS": TDT_STAT_HOST_RAW_FALLBACKS}


class TdtConfigC(C.Structure):
    _fields_ = [
        ("sample_fraction", C.c_float),
        ("word_size", C.c_int32),
        ("bandwidth_threshold_mbps", C.c_double),
        ("cpu_usage_threshold", C.c_double),
        ("min_tensor_size", C.c_uint64),
    ]


_vp = C.c_void_p
# name -> (restype, argtypes); every function declared in include/psyne_tdt.h
SIGNATURES = {
    "tdt_default_config": (None, [C.POINTER(TdtConfigC)]),
    "tdt_ctx_create": (C.c_int, [C.c_int, C.POINTER(TdtConfigC), C.POINTER(_vp)]),
    "tdt_ctx_destroy": (None, [_vp]),
    "tdt_ctx_set_metrics": (None, [_vp, C.c_double, C.c_double, C.c_double]),
    "tdt_ctx_get_metrics": (None, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "tdt_ctx_set_size_hint": (None, [_vp, C.c_uint64]),
    "tdt_should_transform": (C.c_int, [_vp, C.c_uint64]),
    "tdt_encode_bound": (C.c_uint64, [C.c_uint64, C.c_int32]),
    "tdt_ctx_encode_bound": (C.c_uint64, [_vp, C.c_uint64]),
    "tdt_ctx_host_encode_bound": (C.c_uint64, [_vp, C.c_uint64]),
    "tdt_encode_batch": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp, _vp]),
    "tdt_encode_with_mapping_batch": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, C.c_uint64, _vp, _vp, _vp]),
    "tdt_decode_batch": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp, _vp]),
    "tdt_decoded_sizes_batch": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "tdt_encode_batch_into": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "tdt_decode_batch_into": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "tdt_encode_batch_v": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "tdt_encode_batch_vw": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "tdt_pack_v": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp, _vp]),
    "tdt_encode_batch_vp": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, C.c_uint32, C.c_uint64, _vp, C.c_uint64, _vp, _vp,
                                      _vp]),
    "tdt_encoded_sizes_batch": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "tdt_encoded_sizes_v": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp]),
    "tdt_mappings_v": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp, _vp]),
    "tdt_encode_mapped_v": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tdt_encode_mapped_vp": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint64, _vp,
                                       _vp, _vp]),
    "tdt_decode_batch_v": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "tdt_decoded_sizes_v": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "tdt_encode_slots": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp]),
    "tdt_decode_slots": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "tdt_analyze_batch": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "tdt_encode_host": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp]),
    "tdt_decode_host": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp]),
    "tdt_encode_host_v": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp]),
    "tdt_host_alloc": (C.c_int, [C.c_uint64, C.POINTER(C.c_void_p)]),
    "tdt_host_free": (None, [_vp]),
    "tdt_host_copy": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "tdt_copy_device": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "tdt_analyze_host": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "tdt_ctx_error_flags": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint32)]),
    "tdt_ctx_set_option": (C.c_int, [_vp, C.c_int, C.c_uint64]),
    "tdt_ctx_get_stat": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64)]),
    "tdt_last_error": (C.c_char_p, []),
    "tdt_status_string": (C.c_char_p, [C.c_int]),
}

_lib = None


def load(path: pathlib.Path | None = None) -> C.CDLL:
    """Load libpsyne_tdt.so; raises (never falls back) if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # PSYNE_TDT_LIB: an alternative build of the same HIP library (diagnostic experiments)
    p = pathlib.Path(path or os.environ.get("PSYNE_TDT_LIB") or LIB_PATH)
    if not p.exists():
        raise RuntimeError(f"{p} not built: run `python -m psyne_amd.build` (hipcc --offload-arch=gfx950)")
    lib = C.CDLL(str(p))
    for name, (res, args) in SIGNATURES.items():
        f = getattr(lib, name, None)
        if f is None:
            # an older build chosen with PSYNE_TDT_LIB or `path` (A/B runs against a parent commit's
            # library) may lack newer entry points: calling one then raises AttributeError.  The
            # product library exports every one of them.
            if p == LIB_PATH:
                raise RuntimeError(f"{p} does not export {name}: rebuild it (`python -m psyne_amd.build`)")
            continue
        f.restype = res
        f.argtypes = args
    if path is None:
        _lib = lib
    return lib


class TdtError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        self.code = code
        super().__init__(f"TDT error {code}: {msg}")


def check(code: int):
    if code != TDT_OK:
        lib = load()
        raise TdtError(code, lib.tdt_last_error().decode() or lib.tdt_status_string(code).decode())
