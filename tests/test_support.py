"""The shared test helpers (tests/support.py, tests/mixed_ws_cases.py): the random inputs they build
are pinned to what the copies they replaced built, and the small arithmetic helpers to literals."""
import numpy as np
import pytest

from tests.mixed_ws_cases import SIZES, records
from tests.support import CXX, digest, gradient, mask_of, offsets, offsets_of, phased_slots, run_host_cpp


def test_gradient_is_the_replaced_copy():
    # at the parent commit:
    # python -c "import hashlib, numpy as np, tests.test_gpu_copy_routes as m; \
    #   print(hashlib.sha256(m.gradient(np.random.default_rng(1), 4096).tobytes()).hexdigest()[:16])"
    assert digest(gradient(np.random.default_rng(1), 4096).tobytes()) == "e2f3bcecc6cd64c0"


def test_records_is_the_replaced_copy():
    # at the parent commit:
    # python -c "import hashlib, numpy as np, tests.test_gpu_mixed_ws as m; \
    #   print(hashlib.sha256(m.records(np.random.default_rng(1), 12, 4104).tobytes()).hexdigest()[:16])"
    assert 4104 in SIZES
    assert digest(records(np.random.default_rng(1), 12, 4104).tobytes()) == "4ffcbe02a472173c"


def test_offsets_by_parts_and_by_lengths_agree():
    parts = [b"abc", b"", np.zeros(5, np.uint8), b"x"]
    want = [0, 3, 3, 8, 9]
    assert offsets_of(parts).tolist() == want and offsets([len(p) for p in parts]).tolist() == want
    assert offsets_of(parts).dtype == offsets([3, 0]).dtype == np.int64
    assert offsets_of([]).tolist() == offsets([]).tolist() == [0]


def test_phased_slots_take_every_residue():
    table, end = phased_slots([1] * 16)
    assert table.size == 17
    assert sorted(int(t) % 16 for t in table[:16]) == list(range(16))
    assert (np.diff(table[:16]) >= 1 + 16).all()
    assert end > table[15] + 1 and end >= table[16]


def test_mask_of_sets_bit_width_minus_one():
    assert mask_of([1, 2, 4, 8, 16, 3, 12]) == 0x888F


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_run_host_cpp_reports_a_missing_pattern(tmp_path):
    src = tmp_path / "hello.cpp"
    src.write_text('#include <cstdio>\nint main() { std::puts("hello: 1 failures"); }\n')
    with pytest.raises(AssertionError) as ei:
        run_host_cpp(src, tmp_path, r"hello: 0 failures")
    assert "hello: 1 failures" in str(ei.value)
