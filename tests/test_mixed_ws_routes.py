"""The mask-to-routes mapping of tdt_encode_batch_vw (psy::mixed_routes, psyne_amd/csrc/tdt_plan.h):
plain host C++, checked by tests/cpp/test_mixed_routes.cpp — a program of its own, built with
AddressSanitizer and UBSan and run directly."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_mixed_routes.cpp"
CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_mixed_routes(tmp_path):
    exe = tmp_path / "test_mixed_routes"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", str(SRC), "-o", str(exe)], timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"mixed routes: 0 failures", r.stdout), r.stdout
