"""The piece-to-segments arithmetic of the pack kernel (psyne_amd/csrc/tdt_pack.h: the 64-ary search
for a piece's first blob and the walk over its segments): plain host C++, checked by
tests/cpp/test_pack_segments.cpp — a program of its own, built with AddressSanitizer and UBSan and
run directly."""
import pytest

from tests.support import CXX, run_host_cpp


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_pack_segments(tmp_path):
    run_host_cpp("test_pack_segments.cpp", tmp_path, r"pack segments: 0 failures")
