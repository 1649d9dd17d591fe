"""The routing cases (tests/policy_cases.py) against their pinned record (tests/golden/policy_matrix.json,
written by tests/golden/make_policy_matrix.py where the compiled reference exists): the cases cover
every term on both sides in every message class, the CPU oracle answers and encodes what the reference
did, and the record's verdicts are the formula, restated once below.  Pins the yardstick the GPU routes
(tests/test_gpu_policy_matrix.py) compare with."""
import json

import pytest

from oracle.oracle import Oracle, Reference
from tests import policy_cases as pc
from tests.golden_cases import GOLDEN
from tests.support import digest


@pytest.fixture(scope="module")
def record():
    meta = json.loads((GOLDEN / "policy_matrix.json").read_text())
    assert meta["seed"] == pc.SEED
    return meta["cases"]


@pytest.fixture(scope="module")
def cases():
    return pc.all_cases()


def oracle_config(orc, c):
    return orc.config(word_size=c.ws, sample_fraction=1.0, bandwidth_threshold_mbps=c.bandwidth_threshold,
                      cpu_usage_threshold=c.cpu_threshold, min_tensor_size=c.min_tensor)


def test_coverage(cases):
    pc.check_coverage(cases)
    assert 600 <= len(cases) <= 1100
    assert max(c.n for c in cases) <= 262144
    # every `off` case fails exactly its term, every `on` case none
    for c in cases:
        assert pc.flipped_terms(c) == ([c.term] if c.side == "off" else []), c.name


def test_oracle_equals_the_record(cases, record):
    orc = Oracle()
    assert [c.name for c in cases] == [r["name"] for r in record]
    lengths = {}
    for c, r in zip(cases, record):
        cfg = oracle_config(orc, c)
        assert int(orc.should_transform(c.n, cfg=cfg, bandwidth=c.bandwidth, cpu=c.cpu)) == r["st"], c.name
        blob = orc.encode(c.message, cfg=cfg, bandwidth=c.bandwidth, cpu=c.cpu)
        assert (int(blob[:4] == b"DTDT"), len(blob), digest(blob)) == (r["tdt"], r["len"], r["sha"]), c.name
        assert blob[:4] == b"DTDT" or (blob[:4] == b"PCNU" and blob[4:] == c.message.tobytes()), c.name
        lengths[c.name] = len(blob)
    # the premises about the content: no TDT blob of n + 4 bytes, none longer unless its frame alone is
    pc.check_blob_lengths(cases, lengths)
    exceed = [c.name for c in cases if c.side == "on" and lengths[c.name] > c.n + 4]
    assert all(c.n <= 120 and c.ws >= 16 for c in cases if c.name in exceed) and len(exceed) == 10


def test_record_equals_the_formula(cases, record):
    """The decision, written out once more: the record, the oracle and the documentation cannot drift
    apart silently."""
    for c, r in zip(cases, record):
        n = c.n
        policy_on = c.cpu <= c.cpu_threshold and c.bandwidth < c.bandwidth_threshold
        tdt = policy_on and n >= c.min_tensor and n % 4 == 0 and n >= 64 and n % c.ws == 0
        assert r["tdt"] == int(tdt) == int(c.side == "on"), c.name
        # should_transform itself has no word-size guard (it lives in compress_tdt): on the `modws`
        # cases it says yes and the blob is raw all the same
        assert r["st"] == int(policy_on and n >= c.min_tensor and n % 4 == 0 and n >= 64), c.name
        assert (r["st"] != r["tdt"]) == (c.term == "modws" and c.side == "off"), c.name
        assert r["tdt"] or r["len"] == n + 4, c.name


@pytest.mark.skipif(not (Reference.available() and Reference().has_policy),
                    reason="oracle/_ref not built (needs the reference at build time)")
def test_reference_equals_the_record(cases, record):
    ref = Reference()
    for c, r in zip(cases, record):
        st, blob = ref.policy(c.message, word_size=c.ws, bandwidth=c.bandwidth, cpu=c.cpu, min_tensor_size=c.min_tensor,
                              bandwidth_threshold_mbps=c.bandwidth_threshold, cpu_usage_threshold=c.cpu_threshold)
        assert (int(st), int(blob[:4] == b"DTDT"), len(blob), digest(blob)) == (r["st"], r["tdt"], r["len"], r["sha"]), c.name
