"""The funnel-shift copy shared by the passthrough, gather, host-output and pack kernels
(psyne_amd/csrc/tdt_copy.h: the split of a copy into head, 16-byte chunks and tail, the combine of
five aligned dwords, and the loop over them): plain host C++, checked by
tests/cpp/test_copy_shifted.cpp — a program of its own, built with AddressSanitizer and UBSan and
run directly."""
import pytest

from tests.support import CXX, run_host_cpp


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_copy_shifted(tmp_path):
    run_host_cpp("test_copy_shifted.cpp", tmp_path, r"copy shifted: 0 failures")
