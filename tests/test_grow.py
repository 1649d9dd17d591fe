"""The buffer grower of the host API (psyne_amd/csrc/tdt_grow.h: one function template and the three
capacity rules): plain host C++, checked by tests/cpp/test_grow.cpp over a fake allocator — a program
of its own, built with AddressSanitizer and UBSan and run directly."""
import pytest

from tests.support import CXX, run_host_cpp


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_grow(tmp_path):
    run_host_cpp("test_grow.cpp", tmp_path, r"grow: 0 failures")
