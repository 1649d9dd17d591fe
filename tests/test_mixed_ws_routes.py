"""The mask-to-routes mapping of tdt_encode_batch_vw (psy::mixed_routes, psyne_amd/csrc/tdt_plan.h):
plain host C++, checked by tests/cpp/test_mixed_routes.cpp — a program of its own, built with
AddressSanitizer and UBSan and run directly."""
import pytest

from tests.support import CXX, run_host_cpp


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_mixed_routes(tmp_path):
    run_host_cpp("test_mixed_routes.cpp", tmp_path, r"mixed routes: 0 failures", run_timeout=120)
