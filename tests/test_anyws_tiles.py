"""The tile arithmetic of the tiled generic-width encode (psyne_amd/csrc/tdt_anyws_tiles.h: a tile's
stream range, its predecessor byte, the pairs of a run, the scan's combine): plain host C++, checked
by tests/cpp/test_anyws_tiles.cpp — a program of its own, built with AddressSanitizer and UBSan and
run directly."""
import pytest

from tests.support import CXX, run_host_cpp


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_anyws_tiles(tmp_path):
    run_host_cpp("test_anyws_tiles.cpp", tmp_path, r"anyws tiles: \d+ messages, 0 failures")
