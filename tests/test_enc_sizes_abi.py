"""CPU-side check of the exact-size entry points: include/psyne_tdt.h declares tdt_encoded_sizes_batch
and tdt_encoded_sizes_v with the documented parameter lists and TDT_OPT_PACK_SIZES_FIRST, psyne_amd/_lib.py
binds them with as many arguments, the built library exports them, and the Python layer has its side."""
import pathlib
import re

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

EXPECTED = {
    "tdt_encoded_sizes_batch": ["ctx", "d_in", "d_in_off", "n_msgs", "d_enc_sizes", "d_status", "hip_stream"],
    "tdt_encoded_sizes_v": ["ctx", "d_msgs", "d_sizes", "d_word_size", "width_mask", "n_msgs", "d_enc_sizes", "d_status",
                            "hip_stream"],
}


def header():
    return (ROOT / "include" / "psyne_tdt.h").read_text()


def declaration(name):
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name + " is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_declares_size_calls(name):
    params = declaration(name)
    assert [re.search(r"(\w+)$", p).group(1) for p in params] == EXPECTED[name]
    assert params[0].startswith("tdt_ctx *") and params[-1].startswith("void *")
    by_name = dict(zip(EXPECTED[name], params))
    assert by_name["n_msgs"].startswith("uint32_t ")
    assert by_name["d_enc_sizes"].startswith("uint64_t *") and by_name["d_status"].startswith("int32_t *")
    if name == "tdt_encoded_sizes_batch":
        assert by_name["d_in"].startswith("const uint8_t *") and by_name["d_in_off"].startswith("const uint64_t *")
    else:
        assert "const uint8_t *const *" in by_name["d_msgs"] and by_name["d_sizes"].startswith("const uint64_t *")
        assert by_name["d_word_size"].startswith("const int32_t *") and by_name["width_mask"].startswith("uint64_t ")


def test_header_defines_the_option_and_names_the_reference_interface():
    m = re.search(r"^#define\s+TDT_OPT_PACK_SIZES_FIRST\s+(\d+)\b", header(), re.M)
    assert m and int(m.group(1)) == 7
    table = header().split("Wire format:")[0]
    assert "tdt_encoded_sizes_batch" in table and "tdt_encoded_sizes_v" in table and "transformation_ratio" in table


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_binding_lists_size_calls(name):
    import ctypes as C
    from psyne_amd import _lib
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(EXPECTED[name])
    for p, a in zip(EXPECTED[name], args):
        want = {"n_msgs": C.c_uint32, "width_mask": C.c_uint64}
        assert a is want.get(p, C.c_void_p), p
    assert _lib.TDT_OPT_PACK_SIZES_FIRST == 7


def test_codec_has_the_python_layer():
    import inspect
    from psyne_amd import TdtCodec
    # (behind them: the optional result tensors of a captured call)
    assert list(inspect.signature(TdtCodec.encoded_sizes).parameters)[:4] == ["self", "data", "offsets", "stream"]
    sig = inspect.signature(TdtCodec.encoded_sizes_v).parameters
    assert list(sig)[:6] == ["self", "ptrs", "sizes", "word_sizes", "width_mask", "stream"]
    assert all(sig[k].default is None for k in list(sig)[6:])
    assert sig["word_sizes"].default is None and sig["width_mask"].default == 0
    et = inspect.signature(TdtCodec.encode_tensors).parameters
    assert et["exact"].default is False and et["packed"].default is False
    assert "synchronis" in TdtCodec.encode_tensors.__doc__  # exact=True reads the total back: the docstring says so


def test_library_exports_size_calls():
    from psyne_amd import _lib
    if not _lib.LIB_PATH.exists():
        pytest.skip("libpsyne_tdt.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    for name in EXPECTED:
        assert hasattr(lib, name), name
    # a null context is an argument error, with or without messages
    assert lib.tdt_encoded_sizes_batch(None, None, None, 0, None, None, None) != 0
    assert lib.tdt_encoded_sizes_batch(None, None, None, 4, None, None, None) != 0
    assert lib.tdt_encoded_sizes_v(None, None, None, None, 0b1010, 0, None, None, None) != 0
    assert lib.tdt_encoded_sizes_v(None, None, None, None, 0b1010, 4, None, None, None) != 0
    assert lib.tdt_ctx_set_option(None, _lib.TDT_OPT_PACK_SIZES_FIRST, 1) != 0
