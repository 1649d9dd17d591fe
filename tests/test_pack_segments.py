"""The piece-to-segments arithmetic of the pack kernel (psyne_amd/csrc/tdt_pack.h: the 64-ary search
for a piece's first blob and the walk over its segments): plain host C++, checked by
tests/cpp/test_pack_segments.cpp — a program of its own, built with AddressSanitizer and UBSan and
run directly."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_pack_segments.cpp"
CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_pack_segments(tmp_path):
    exe = tmp_path / "test_pack_segments"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", str(SRC), "-o", str(exe)], timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"pack segments: 0 failures", r.stdout), r.stdout
