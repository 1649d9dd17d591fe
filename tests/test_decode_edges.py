"""The decode edge cases (tests/decode_edge_cases.py) against their pinned record
(tests/golden/decode_edges.json, written by tests/golden/make_decode_edges.py where the compiled
reference exists): the generator still builds the recorded blobs, the CPU oracle still gives the
recorded bytes with status 0, and a plain numpy decoder agrees with it.  Pins the yardstick the GPU
tests of those blobs (tests/test_gpu_decode_edges.py) compare with."""
import json

import pytest

from oracle.oracle import Oracle, Reference
from tests import decode_edge_cases as ec
from tests.golden_cases import GOLDEN
from tests.support import digest


@pytest.fixture(scope="module")
def record():
    return json.loads((GOLDEN / "decode_edges.json").read_text())


@pytest.fixture(scope="module")
def decoded():
    """name → (status, bytes) from the oracle, computed once."""
    orc = Oracle()
    return {c.name: orc.decode(c.blob) for c in ec.all_cases()}


def test_generator_reproduces_every_blob(record):
    cases = ec.all_cases()
    assert record["dropped"] == []
    assert record["geometry"] == ec.geometry()  # (new kernel sizes move the edges: make the record again)
    assert [c.name for c in cases] == [r["name"] for r in record["cases"]]
    for c, r in zip(cases, record["cases"]):
        assert (c.ws, c.family, digest(c.blob)) == (r["ws"], r["family"], r["blob"]), c.name


def test_oracle_reproduces_every_output(record, decoded):
    for r in record["cases"]:
        st, out = decoded[r["name"]]
        assert st == 0, (r["name"], st)
        assert digest(out) == r["out"], r["name"]


def test_numpy_decoder_equals_oracle(decoded):
    for c in ec.all_cases():
        assert ec.numpy_decode(c.blob) == decoded[c.name][1], c.name


def test_coverage():
    cases = ec.all_cases()
    ec.check_coverage(cases)
    assert len(cases) <= ec.MAX_CASES and {c.family for c in cases} == set(ec.FAMILIES)
    # the geometry read from the source, and what follows from it for one known shape
    g = ec.geometry()
    assert set(g) == {"tile_groups", "wr", "one_waves", "blobc", "any_pairs", "dsmall_max", "dbig_min", "one_max"}
    k = ec.stream_kinds("fast", 4, 3, 65552)
    seg, groups = 12, 4097
    tg = -(-(-(-groups // g["one_waves"])) // 64) * 64
    assert k == dict(share=16388 * 3, lane8=8, block=512, lane=16, round=64 * seg, window=g["wr"] * 64 * seg,
                     gen=8 * g["wr"] * 64 * seg, tile=g["tile_groups"] * seg, onetile=tg * seg)
    assert ec.stream_kinds("fast", 4, 3, g["dsmall_max"])["window"] == 64 * seg
    assert ec.referenced(4, [1, 1, 1, 0]) == [(1, 3), (0, 1)]


def test_locate_names_the_nearest_edge():
    mapping = (1, 1, 1, 0)
    c = next(c for c in ec.all_cases() if c.name == "w4_1110_edge_65552_d+0")
    sid, kind, d, what, pos, pi = next(e for e in c.edges if e[1] == "tile" and not e[3].startswith("cross"))
    k = mapping.count(sid)
    column = [b for b in range(4) if mapping[b] == sid][pos % k]  # the output byte of stream position pos
    said = ec.locate(c, (pos // k) * 4 + column)
    assert said.startswith("stream %d position %d, nearest edge: tile d=+0" % (sid, pos)), said
    assert said.endswith(" at %d, pair %d" % (pos, pi)), said


@pytest.mark.skipif(not Reference.available(), reason="oracle/_ref not built (needs the reference at build time)")
def test_reference_equals_oracle(decoded):
    ref = Reference()
    for c in ec.all_cases():
        st, out, err = ref.decode(c.blob, cap=1 << 18)
        assert st == 0, (c.name, err)
        assert out == decoded[c.name][1], c.name
