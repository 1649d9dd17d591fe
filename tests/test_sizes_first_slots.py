"""The slot arithmetic of the sizes-first packed encode (psyne_amd/csrc/tdt_pack.h: pack_exact_slot,
blob i's slot in the caller's buffer from the scanned exact sizes and out_cap): plain host C++,
checked by tests/cpp/test_sizes_first_slots.cpp — a program of its own, built with AddressSanitizer
and UBSan and run directly."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_sizes_first_slots.cpp"
CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_sizes_first_slots(tmp_path):
    exe = tmp_path / "test_sizes_first_slots"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", str(SRC), "-o", str(exe)], timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"sizes-first slots: 0 failures", r.stdout), r.stdout
