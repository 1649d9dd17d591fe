"""The raw-fallback fixtures (tests/raw_fallback_cases.py) on the CPU: every fixture lies on its
intended side of the rule "E > n + 4", its expected blob decodes to the message, and inputs and
expected blobs match the digests pinned in tests/golden/raw_fallback.json."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import raw_fallback_cases as rc

# kind -> True: the rule stores it raw; False: the blob stays as it is; None: the side is the oracle's (pinned)
SIDE = {"uniform": True, "thr+2": True, "one+2": True, "grad70": False, "thr-2": False, "thr0": False, "one-2": False,
        "one+0": False, "odd": False, "short": False, "ragged": False, "empty": False, "dense": None}
GAP = {"thr-2": -2, "thr0": 0, "thr+2": 2, "one-2": -2, "one+0": 0, "one+2": 2}
ROUTED = ("odd", "short", "ragged", "empty")


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def golden():
    return rc.load_golden()


def check(c, golden, orc, seen):
    n = c["x"].size
    seen.add(c["name"])
    assert rc.case_digest(c) == golden[c["name"]], c["name"]
    side = SIDE[c["kind"]]
    if c["kind"] == "dense" and c["ws"] == 4:
        side = True  # a dense fp32 gradient at its own width expands
    if side is not None:
        assert c["falls"] == side, c["name"]
    assert c["falls"] == (len(c["plain"]) > n + 4), c["name"]
    if c["kind"] in GAP:
        assert len(c["plain"]) - (n + 4) == GAP[c["kind"]] and c["plain"][:4] == b"DTDT", c["name"]
    if c["kind"] in ROUTED:
        assert c["plain"] == rc.UNCP + c["x"].tobytes() == c["want"], c["name"]
    assert c["want"] == (rc.UNCP + c["x"].tobytes() if c["falls"] else c["plain"]), c["name"]
    assert len(c["want"]) == min(len(c["plain"]), n + 4), c["name"]
    st, back = orc.decode(c["want"])
    assert st == 0 and back == c["x"].tobytes(), c["name"]


def test_fixtures_lie_on_their_sides_and_decode(orc, golden):
    seen = set()
    for ws, n, _ in rc.all_configs():
        batch = rc.batch(orc, ws, n, rc.seed_of(ws, n))
        kinds = [c["kind"] for c in batch]
        assert {"uniform", "dense", "grad70", "odd", "short", "empty", "thr-2", "thr0", "thr+2"} <= set(kinds)
        # interleaved: no fallback beside another
        assert not any(a["falls"] and b["falls"] for a, b in zip(batch, batch[1:])), (ws, n)
        for c in batch:
            check(c, golden, orc, seen)
    for ws, n in rc.MAPPED_TRIOS:
        for c in rc.mapped_trio(orc, ws, n):
            assert c["mapping"] == [0] * ws
            check(c, golden, orc, seen)
    assert seen == set(golden)


# The blob lengths the feature was motivated with: (generator, n, ws, length, relative spread).  The
# lengths are those of one random draw each, so the fixtures' generators are held to them within the
# spread of such draws: a blob is 2 bytes per run, the run count of n random bytes scatters by about
# sqrt(n) / n around its mean (a few times that is allowed), and the 1 KiB gradient, whose run count
# hangs on where its ~77 non-zero values fall, by far more.
ISSUE_TABLE = [(rc.dense, 1024, 4, 1976, 0.03), (rc.dense, 65536, 4, 123940, 0.005), (rc.uniform, 65536, 4, 130684, 0.002),
               (rc.uniform, 65520, 12, 130562, 0.002), (rc.grad70, 1024, 4, 886, 0.2), (rc.grad70, 65536, 4, 52338, 0.04)]


def test_the_issue_table(orc):
    for gen, n, ws, length, spread in ISSUE_TABLE:
        cfg = orc.config(sample_fraction=1.0, word_size=ws)
        for seed in range(4):
            got = len(orc.encode(gen(n, seed), cfg=cfg))
            assert abs(got - length) <= spread * length, (gen.__name__, n, ws, seed, got, length)
            assert (got > n + 4) == (gen is not rc.grad70)


def test_mapping_zero_can_beat_the_analysed_split(orc):
    """Why tdt_mappings_v keeps the analysed bits of a message that falls back: mapping 0 is a valid
    single-stream mapping whose blob can be shorter than n + 4 where the analysed split's is longer
    (16 KiB of words (k, k, k, k), varied), so zeroed bits would encode to other bytes."""
    k = np.arange(4096, dtype=np.int64)
    w = np.repeat((k % 251 + 1)[:, None], 4, axis=1).astype(np.uint8)
    w[::2, 3] = 0  # position 3 is half zeros: less entropy than the others, a stream of its own
    x = w.reshape(-1)
    mp = [int(v) for v in orc.analyze(x, 4)[2]]
    assert 0 < sum(mp) < 4
    cfg = orc.config(sample_fraction=1.0, word_size=4)
    split, single = orc.encode(x, cfg=cfg), orc.encode(x, cfg=cfg, mapping=[0, 0, 0, 0])
    assert len(split) != len(single)
