"""The slot arithmetic of the sizes-first packed encode (psyne_amd/csrc/tdt_pack.h: pack_exact_slot,
blob i's slot in the caller's buffer from the scanned exact sizes and out_cap): plain host C++,
checked by tests/cpp/test_sizes_first_slots.cpp — a program of its own, built with AddressSanitizer
and UBSan and run directly."""
import pytest

from tests.support import CXX, run_host_cpp


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_sizes_first_slots(tmp_path):
    run_host_cpp("test_sizes_first_slots.cpp", tmp_path, r"sizes-first slots: 0 failures")
