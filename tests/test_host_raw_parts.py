"""The part arithmetic of the host pipeline's raw gather (TDT_OPT_HOST_RAW_FALLBACK; raw_span of
psyne_amd/csrc/tdt_rawfb.h): plain host C++, checked by tests/cpp/test_host_raw_parts.cpp — a program of
its own, built with AddressSanitizer and UBSan and run directly."""
import pytest

from tests.support import CXX, run_host_cpp


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_host_raw_parts(tmp_path):
    run_host_cpp("test_host_raw_parts.cpp", tmp_path, r"host raw parts: 0 failures")
