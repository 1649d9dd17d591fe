"""CPU-side check of the scattered-batch entry points: include/psyne_tdt.h declares them with the
documented parameter lists and psyne_amd/_lib.py binds them with as many arguments."""
import pathlib
import re

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

# name -> parameter names, in order
EXPECTED = {
    "tdt_encode_batch_v": ["ctx", "d_msgs", "d_sizes", "n_msgs", "d_blobs", "d_blob_cap", "d_out_len", "d_status",
                           "hip_stream"],
    "tdt_decode_batch_v": ["ctx", "d_blobs", "d_blob_len", "n_msgs", "d_outs", "d_out_cap", "d_out_len", "d_status",
                           "hip_stream"],
    "tdt_decoded_sizes_v": ["ctx", "d_blobs", "d_blob_len", "n_msgs", "d_sizes", "d_status", "hip_stream"],
}


def declaration(name):
    src = (ROOT / "include" / "psyne_tdt.h").read_text()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name + " is not declared"
    return [p.strip() for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_declares_scattered_call(name):
    params = declaration(name)
    assert [re.search(r"(\w+)$", p).group(1) for p in params] == EXPECTED[name]
    assert params[0].startswith("tdt_ctx *") and params[-1].startswith("void *")
    # the message / blob / output tables are arrays of pointers
    tables = [params[1]] if name == "tdt_decoded_sizes_v" else [params[1], params[4]]
    assert all("uint8_t *const *" in p for p in tables)
    assert "uint32_t" in params[3]


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_binding_lists_scattered_call(name):
    import ctypes as C
    from psyne_amd import _lib
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(EXPECTED[name])
    assert args[3] is C.c_uint32


def test_library_exports_scattered_calls():
    from psyne_amd import _lib
    if not _lib.LIB_PATH.exists():
        pytest.skip("libpsyne_tdt.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    for name in EXPECTED:
        assert hasattr(lib, name), name
    # a batch without messages touches nothing, not even the context
    assert lib.tdt_encode_batch_v(None, None, None, 0, None, None, None, None, None) != 0  # (null context)
