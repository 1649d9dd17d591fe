"""The scan arithmetic of the tiled decode-reduce (psyne_amd/csrc/tdt_red_tiles.h: tile and block counts,
the tiles a block's range covers, a tile's carry block or "the stream ended before this tile"): plain
host C++, checked against a walk over pair lists by tests/cpp/test_red_tiles.cpp — a program of its own,
built with AddressSanitizer and UBSan and run directly."""
import pytest

from tests.support import CXX, run_host_cpp


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_red_tiles(tmp_path):
    run_host_cpp("test_red_tiles.cpp", tmp_path, r"red tiles: \d+ streams, 0 failures")
