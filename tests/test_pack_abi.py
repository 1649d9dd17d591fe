"""CPU-side check of the packed wire buffer's entry points: include/psyne_tdt.h declares tdt_pack_v
and tdt_encode_batch_vp with the documented parameter lists, psyne_amd/_lib.py binds them with as
many arguments, and the built library exports them."""
import pathlib
import re

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

EXPECTED = {
    "tdt_pack_v": ["ctx", "d_blobs", "d_blob_len", "n_msgs", "d_out", "out_cap", "d_out_off", "d_status", "hip_stream"],
    "tdt_encode_batch_vp": ["ctx", "d_msgs", "d_sizes", "d_word_size", "width_mask", "n_msgs", "total_bytes", "d_out",
                            "out_cap", "d_out_off", "d_status", "hip_stream"],
}


def header():
    return (ROOT / "include" / "psyne_tdt.h").read_text()


def declaration(name):
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name + " is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_declares_packed_calls(name):
    params = declaration(name)
    assert [re.search(r"(\w+)$", p).group(1) for p in params] == EXPECTED[name]
    assert params[0].startswith("tdt_ctx *") and params[-1].startswith("void *")
    assert "const uint8_t *const *" in params[1] and params[2].startswith("const uint64_t *")
    by_name = dict(zip(EXPECTED[name], params))
    assert by_name["n_msgs"].startswith("uint32_t ") and by_name["out_cap"].startswith("uint64_t ")
    assert by_name["d_out"].startswith("uint8_t *") and by_name["d_out_off"].startswith("uint64_t *")
    assert by_name["d_status"].startswith("int32_t *")
    if name == "tdt_encode_batch_vp":
        assert by_name["d_word_size"].startswith("const int32_t *")
        assert by_name["width_mask"].startswith("uint64_t ") and by_name["total_bytes"].startswith("uint64_t ")


def test_header_names_the_reference_interface():
    # the "which reference interface" table has a row for the packed calls
    table = header().split("Wire format:")[0]
    assert "tdt_encode_batch_vp" in table and "tdt_pack_v" in table and "framed send" in table


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_binding_lists_packed_calls(name):
    import ctypes as C
    from psyne_amd import _lib
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(EXPECTED[name])
    for p, a in zip(EXPECTED[name], args):
        want = {"n_msgs": C.c_uint32, "out_cap": C.c_uint64, "width_mask": C.c_uint64, "total_bytes": C.c_uint64}
        assert a is want.get(p, C.c_void_p), p


def test_codec_has_the_python_layer():
    import inspect
    from psyne_amd import TdtCodec
    assert list(inspect.signature(TdtCodec.pack_v).parameters)[:4] == ["self", "ptrs", "lengths", "out"]
    assert list(inspect.signature(TdtCodec.encode_vp).parameters)[:5] == ["self", "ptrs", "sizes", "total_bytes", "out"]
    assert inspect.signature(TdtCodec.encode_tensors).parameters["packed"].default is False


def test_library_exports_packed_calls():
    from psyne_amd import _lib
    if not _lib.LIB_PATH.exists():
        pytest.skip("libpsyne_tdt.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    for name in EXPECTED:
        assert hasattr(lib, name), name
    # a null context is an argument error, with or without messages
    assert lib.tdt_pack_v(None, None, None, 0, None, 0, None, None, None) != 0
    assert lib.tdt_pack_v(None, None, None, 4, None, 0, None, None, None) != 0
    assert lib.tdt_encode_batch_vp(None, None, None, None, 0b1010, 0, 0, None, 0, None, None, None) != 0
    assert lib.tdt_encode_batch_vp(None, None, None, None, 0b1010, 4, 4096, None, 0, None, None, None) != 0
