"""The part arithmetic of the host pipeline's raw gather (TDT_OPT_HOST_RAW_FALLBACK; raw_span of
psyne_amd/csrc/tdt_rawfb.h): plain host C++, checked by tests/cpp/test_host_raw_parts.cpp — a program of
its own, built with AddressSanitizer and UBSan and run directly."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_host_raw_parts.cpp"
CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_host_raw_parts(tmp_path):
    exe = tmp_path / "test_host_raw_parts"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", str(SRC), "-o", str(exe)], timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"host raw parts: 0 failures", r.stdout), r.stdout
