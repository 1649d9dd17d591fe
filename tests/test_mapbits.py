"""The mapping bits of the known-mapping calls (tdt_mappings_v, tdt_encode_mapped_v / _vp), on the CPU:
psy::mapbits_ok and its neighbours (psyne_amd/csrc/tdt_mapbits.h) checked by tests/cpp/test_mapbits.cpp —
a program of its own, built with AddressSanitizer and UBSan and run directly — the Python helpers
mapbits_of / mapping_of, and the three entry points' presence in the header, the ctypes table and the
library, with a null context refused."""
import re

import pytest

from tests.support import CXX, ROOT, run_host_cpp

NEW = ("tdt_mappings_v", "tdt_encode_mapped_v", "tdt_encode_mapped_vp")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_mapbits_driver(tmp_path):
    run_host_cpp("test_mapbits.cpp", tmp_path, r"mapbits: 0 failures")


def test_helpers_round_trip_every_width():
    import numpy as np
    from psyne_amd import mapbits_of, mapping_of
    rng = np.random.default_rng(64)
    for ws in range(1, 65):
        for mapping in ([0] * ws, [1] * ws, [int(b) for b in rng.integers(0, 2, ws)],
                        [1 if p == ws - 1 else 0 for p in range(ws)]):
            bits = mapbits_of(mapping)
            assert 0 <= bits < (1 << ws)
            assert bits == sum(m << p for p, m in enumerate(mapping))
            assert mapping_of(bits, ws) == mapping
            # an int64 tensor's entry reads bit 63 as the sign
            signed = bits - (1 << 64) if bits >> 63 else bits
            assert mapping_of(signed, ws) == mapping
        if ws < 64:
            with pytest.raises(ValueError):
                mapping_of(1 << ws, ws)
            with pytest.raises(ValueError):
                mapping_of(-1, ws)  # bit 63
    assert mapbits_of([1, 1, 1, 0]) == 7 and mapping_of(7, 4) == [1, 1, 1, 0]
    for bad in ([], [0] * 65, [0, 2], [-1]):
        with pytest.raises(ValueError):
            mapbits_of(bad)
    for ws in (0, 65):
        with pytest.raises(ValueError):
            mapping_of(0, ws)


def test_header_and_signatures_name_the_three_calls():
    from psyne_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "psyne_tdt.h").read_text(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert "d_mapbits" in m.group(1), name
    assert re.search(r"#define\s+TDT_OPT_PACK_SIZES_FIRST\s+7\b", src)


def test_null_context_is_refused():
    from psyne_amd import _lib
    if not _lib.LIB_PATH.exists():
        pytest.skip("libpsyne_tdt.so not built")
    lib = _lib.load()
    assert lib.tdt_mappings_v(None, None, None, None, 0, 1, None, None, None, None) == _lib.TDT_E_ARG
    assert lib.tdt_encode_mapped_v(None, None, None, None, 0, 1, None, None, None, None, None, None) == _lib.TDT_E_ARG
    assert lib.tdt_encode_mapped_vp(None, None, None, None, 0, 1, 0, None, None, 0, None, None, None) == _lib.TDT_E_ARG
    assert b"null context" in lib.tdt_last_error()
