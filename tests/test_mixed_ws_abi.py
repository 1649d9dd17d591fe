"""CPU-side check of the mixed-width scattered encode's entry point: include/psyne_tdt.h declares
tdt_encode_batch_vw with the documented parameter list, psyne_amd/_lib.py binds it with as many
arguments, and the built library exports it."""
import pathlib
import re

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

NAME = "tdt_encode_batch_vw"
EXPECTED = ["ctx", "d_msgs", "d_sizes", "d_word_size", "width_mask", "n_msgs", "d_blobs", "d_blob_cap", "d_out_len",
            "d_status", "hip_stream"]


def header():
    return (ROOT / "include" / "psyne_tdt.h").read_text()


def declaration():
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", src)
    assert m, NAME + " is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_mixed_call():
    params = declaration()
    assert [re.search(r"(\w+)$", p).group(1) for p in params] == EXPECTED
    assert params[0].startswith("tdt_ctx *") and params[-1].startswith("void *")
    assert "uint8_t *const *" in params[1] and "uint8_t *const *" in params[6]
    assert params[3].startswith("const int32_t *")
    assert params[4].startswith("uint64_t ") and params[5].startswith("uint32_t ")
    # the limit on the mask is written in the header
    assert re.search(r"#define\s+TDT_MIXED_MAX_WIDTHS\s+8\b", header())


def test_binding_lists_mixed_call():
    import ctypes as C
    from psyne_amd import _lib
    assert NAME in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == len(EXPECTED)
    assert args[4] is C.c_uint64 and args[5] is C.c_uint32


def test_protocol_header_forwards_mixed_call():
    src = (ROOT / "include" / "psyne_amd" / "hip_tdt_protocol.hpp").read_text()
    assert re.search(r"\bint\s+encode_batch_vw\s*\(", src) and NAME + "(ctx_," in src


def test_library_exports_mixed_call():
    from psyne_amd import _lib
    if not _lib.LIB_PATH.exists():
        pytest.skip("libpsyne_tdt.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    assert hasattr(lib, NAME)
    assert lib.tdt_encode_batch_vw(None, None, None, None, 0b1010, 0, None, None, None, None, None) != 0  # (null context)
    assert lib.tdt_encode_batch_vw(None, None, None, None, 0b1010, 4, None, None, None, None, None) != 0
