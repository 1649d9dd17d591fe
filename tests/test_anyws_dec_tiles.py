"""The tile arithmetic of the tiled generic-width decode (psyne_amd/csrc/tdt_anyws_dec_tiles.h: a
tile's words and stream range, the clamped block prefix, the search for a tile's first block, the
clip of a pair): plain host C++, checked by tests/cpp/test_anyws_dec_tiles.cpp — a program of its
own, built with AddressSanitizer and UBSan and run directly."""
import pytest

from tests.support import CXX, run_host_cpp


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_anyws_dec_tiles(tmp_path):
    run_host_cpp("test_anyws_dec_tiles.cpp", tmp_path, r"anyws dec tiles: \d+ blobs, 0 failures")
