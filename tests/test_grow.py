"""The buffer grower of the host API (psyne_amd/csrc/tdt_grow.h: one function template and the three
capacity rules): plain host C++, checked by tests/cpp/test_grow.cpp over a fake allocator — a program
of its own, built with AddressSanitizer and UBSan and run directly."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_grow.cpp"
CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_grow(tmp_path):
    exe = tmp_path / "test_grow"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", str(SRC), "-o", str(exe)], timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"grow: 0 failures", r.stdout), r.stdout
