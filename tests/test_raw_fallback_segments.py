"""The arithmetic of the raw fallback's copy, bound and decision (psyne_amd/csrc/tdt_rawfb.h): plain
host C++, checked by tests/cpp/test_raw_fallback_segments.cpp — a program of its own, built with
AddressSanitizer and UBSan and run directly."""
import pytest

from tests.support import CXX, run_host_cpp


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_raw_fallback_segments(tmp_path):
    run_host_cpp("test_raw_fallback_segments.cpp", tmp_path, r"raw fallback segments: 0 failures")
