"""What the test modules share and no GPU is needed for: the C ABI's status numbers, the canary byte,
the small input builders, and the runner of the stand-alone host C++ programs under tests/cpp.
Standard library and numpy only; tests/gpu_support.py holds what needs torch.

The module is no test module, so pytest does not rewrite its asserts: each carries its message."""
import hashlib
import pathlib
import re
import shutil
import subprocess

import numpy as np

# The library's status numbers (include/psyne_tdt.h), as literals: the tests pin the ABI's values
# on their own, not through psyne_amd._lib.
E_SHORT, E_MAGIC, E_TRUNCATED, E_BAD_MAPPING, E_CAPACITY, E_UNSUPPORTED, E_BAD_HEADER, E_CONFIG = 1, 2, 3, 4, 5, 6, 7, 8
E_HIP, E_ARG, E_CAPTURE = 10, 11, 12
CANARY = 0xA5

ROOT = pathlib.Path(__file__).resolve().parent.parent
CXX = shutil.which("g++") or shutil.which("clang++")


def digest(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()[:16]


def offsets_of(parts):
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return off


def offsets(lengths):
    off = np.zeros(len(lengths) + 1, np.int64)
    off[1:] = np.cumsum(np.asarray(lengths, dtype=np.int64))
    return off


def gradient(rng, nbytes):
    """bench.py's payload: float32, 70 % exact zeros, else N(0, 0.01)."""
    x = rng.normal(0, 0.01, nbytes // 4).astype(np.float32)
    x[rng.random(x.size) < 0.7] = 0
    return x.view(np.uint8)


def bits_of(mapping):
    return sum(int(m) << p for p, m in enumerate(mapping))


def mask_of(widths):
    m = 0
    for w in set(widths):
        m |= 1 << (w - 1)
    return m


def phased_slots(sizes, lead=0, step=5):
    """Slot i of sizes[i] bytes starting (lead + step i) mod 16 bytes past a 16-byte boundary (step is
    odd: sixteen consecutive slots take sixteen residues), 16 or more bytes after the slot before:
    (slot table of n + 1 entries, its end).  The table's slots reach up to the next one's start, so
    the gap belongs to the slot and must stay untouched all the same."""
    at, table = 64, []
    for i, s in enumerate(sizes):
        at += (lead + step * i - at) % 16
        table.append(at)
        at += s + 16
    return np.asarray(table + [at], np.int64), at + 64


def address_order(tensors, order):
    idx = sorted(range(len(tensors)), key=lambda i: tensors[i].data_ptr())
    if order == "descending":
        idx.reverse()
    elif order == "shuffled":
        np.random.default_rng(7).shuffle(idx)
    return idx


def run_host_cpp(src, tmp_path, pattern, run_timeout=300):
    """Build `src` (a name under tests/cpp, or an absolute path) as a program of its own with
    AddressSanitizer and UBSan, run it directly, and require exit status 0 and `pattern` in its output."""
    exe = tmp_path / pathlib.Path(src).stem
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", str(ROOT / "tests" / "cpp" / src), "-o", str(exe)],
                          timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=run_timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(pattern, r.stdout), r.stdout


def report(bad):
    assert not bad, "%d mismatches, the first: %s" % (len(bad), "; ".join(bad[:8]))
