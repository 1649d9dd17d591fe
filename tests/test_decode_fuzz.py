"""The crafted decode cases (tests/decode_cases.py) against their pinned record
(tests/golden/decode_fuzz.json, written by tests/golden/make_decode_fuzz.py where the compiled
reference exists): the generator still builds the recorded blobs, the CPU oracle still gives the
recorded statuses and bytes, and a plain numpy decoder agrees with it.  Pins the yardstick the
GPU tests of those blobs (tests/test_gpu_decode_fuzz.py) compare with."""
import json

import pytest

from oracle.oracle import Oracle, Reference
from tests import decode_cases as dc
from tests.golden_cases import GOLDEN
from tests.support import E_UNSUPPORTED, digest


@pytest.fixture(scope="module")
def record():
    return json.loads((GOLDEN / "decode_fuzz.json").read_text())["cases"]


@pytest.fixture(scope="module")
def decoded():
    """name → (status, bytes) from the oracle, computed once."""
    orc = Oracle()
    return {c.name: orc.decode(c.blob) for c in dc.all_cases()}


def test_generator_reproduces_every_blob(record):
    cases = dc.all_cases()
    assert [c.name for c in cases] == [r["name"] for r in record]
    for c, r in zip(cases, record):
        assert (c.ws, c.family, digest(c.blob)) == (r["ws"], r["family"], r["blob"]), c.name


def test_oracle_reproduces_every_status_and_output(record, decoded):
    for r in record:
        st, out = decoded[r["name"]]
        assert st == r["status"], (r["name"], st)
        if st == 0:
            assert digest(out) == r["out"], r["name"]
        else:
            assert "out" not in r and r["ref"] == "ub", r["name"]
    # every documented header status occurs at every width; mapping_size = ws - 1 gives TRUNCATED or
    # BAD_MAPPING depending on what the shifted stream table then holds
    for ws in dc.WIDTHS:
        st = {r["name"].split("_bad_")[1]: r["status"] for r in record if r["family"] == "malformed" and r["ws"] == ws}
        assert {1, 2, 3, 4, 7} <= set(st.values()), ws
        assert (st["cut0"], st["cut3"], st["cut4"], st["cut19"], st["cut20"]) == (1, 1, 3, 3, 3), ws
        assert (st["magic"], st["ws0"], st["map_eq_ns"], st["map_negative"]) == (2, 7, 4, 4), ws
        assert st["msize_short"] in (3, 4) and st["len0_past_end"] == 3 and st["cut_last_byte"] == 3, ws
        assert st["ws65"] == 0, ws
    assert all(r.get("lib_status") == E_UNSUPPORTED for r in record if r["name"].endswith("_ws65"))


def test_numpy_decoder_equals_oracle(decoded):
    n = 0
    for c in dc.valid_cases():
        st, out = decoded[c.name]
        assert st == 0, c.name
        assert dc.numpy_decode(c.blob) == out, c.name
        n += 1
    assert n >= 270


def test_coverage():
    cases = dc.all_cases()
    dc.check_coverage(cases)
    # takes_fast_path restates parse_fast: the shapes the encoder writes are fast, three streams,
    # odd ws-8 shares and ws-16 shares that are no multiple of 4 are not, nor is any generic width
    assert dc.takes_fast_path(4, [1, 1, 0, 0]) and dc.takes_fast_path(4, [0, 1, 1, 1])
    assert dc.takes_fast_path(8, [0, 0, 1, 1, 1, 1, 1, 1]) and not dc.takes_fast_path(8, [0, 0, 0, 1, 1, 1, 1, 1])
    assert dc.takes_fast_path(16, [0] * 4 + [1] * 12) and not dc.takes_fast_path(16, [0] * 6 + [1] * 10)
    assert not dc.takes_fast_path(4, [0, 1, 2, 0]) and not dc.takes_fast_path(12, [0] * 12)
    assert dc.takes_fast_path(2, [0, 1], 16) and not dc.takes_fast_path(2, [0, 1], 17)


@pytest.mark.skipif(not Reference.available(), reason="oracle/_ref not built (needs the reference at build time)")
def test_reference_equals_oracle(decoded):
    ref = Reference()
    for c in dc.valid_cases():
        st, out, err = ref.decode(c.blob, cap=1 << 18)
        assert st == 0, (c.name, err)
        assert out == decoded[c.name][1], c.name
