"""The cases of the tiled generic-width decode and the numpy model of its arithmetic
(tests/anyws_dec_tiled_cases.py), on the CPU: the model gives the oracle's bytes at the kernels' tile
size and at a smaller one, every case holds what its name says, and blobs and outputs match the
digests pinned in tests/golden/anyws_dec_tiled.json (tests/golden/make_anyws_dec_tiled.py)."""
import hashlib
import json
import pathlib

import pytest

from oracle.oracle import Oracle
from tests import anyws_dec_tiled_cases as tc
from tests.decode_cases import numpy_decode

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "anyws_dec_tiled.json"
SMALL_TILE = 4096


@pytest.fixture(scope="module")
def expected():
    orc = Oracle()
    out = {}
    for c in tc.all_cases(with_big=True):
        st, o = orc.decode(c.blob)
        assert st == 0, c.name
        out[c.name] = o
    return out


def test_geometry_read_from_the_sources():
    assert tc.kernel_tile() == 32768 and tc.block_pairs() == 2048
    assert tc.tile_words(64, tc.kernel_tile()) == 512 and tc.tile_words(3, tc.kernel_tile()) == 10922


@pytest.mark.parametrize("tile", [None, SMALL_TILE])
def test_model_matches_oracle(expected, tile):
    tile = tile or tc.kernel_tile()
    bad = [c.name for c in tc.all_cases(with_big=True) if tc.model_decode(c.blob, tile) != expected[c.name]]
    assert not bad, bad[:8]


def test_oracle_matches_numpy_decode(expected):
    bad = [c.name for c in tc.all_cases() if numpy_decode(c.blob) != expected[c.name]]
    assert not bad, bad[:8]


def test_cases_hold_what_they_name():
    tile = tc.kernel_tile()
    cases = tc.all_cases(with_big=True)
    for c in cases:
        tc.holds(c, tile)
    kinds = {k for c in cases for _, k, _, _ in c.claims}
    assert kinds >= set(tc.BOUNDARY_KINDS) | {"block_at", "np_mod", "zero_blocks", "total"}
    # both streams meet every boundary feature, every block offset and every np remainder
    for r in (0, 1):
        assert {k for c in cases for s, k, _, _ in c.claims if s == r} >= set(tc.BOUNDARY_KINDS)
    assert {a for c in cases for _, k, _, a in c.claims if k == "block_at"} == {0, 1, tc.block_pairs() - 1}
    assert {a for c in cases for _, k, _, a in c.claims if k == "np_mod"} == {m % tc.block_pairs() for m in tc.NP_MODS}
    assert {a for c in cases for _, k, _, a in c.claims if k == "zero_blocks"} == {1, 2}
    shapes = [tc.parse(c.blob) for c in cases]
    assert {o % ws for o, _, ws, _, _, _ in shapes if ws > 2} >= {0, 1}
    assert any(o % ws == ws - 1 for o, _, ws, _, _, _ in shapes)
    assert any(ms == ws + 2 for _, _, ws, ms, _, _ in shapes)
    assert any(len(set(mp)) == 1 for _, _, _, _, mp, _ in shapes) and any(len(set(mp)) == 3 for _, _, _, _, mp, _ in shapes)
    assert any(ns > len(set(mp)) for _, ns, _, _, mp, _ in shapes)
    tw = lambda ws: tc.tile_words(ws, tile)  # noqa: E731
    assert any((o // ws) % tw(ws) == 1 for o, _, ws, _, _, _ in shapes)
    assert any((o // ws) % tw(ws) == 0 and o % ws == 0 for o, _, ws, _, _, _ in shapes)
    big = cases[-1]
    assert big.oracle_only and sum(q for _, k, q, _ in big.claims if k == "total") > 2 ** 32


def test_digests_are_pinned(expected):
    gold = json.loads(GOLDEN.read_text())
    assert gold["tile"] == tc.kernel_tile() and gold["block_pairs"] == tc.block_pairs() and gold["seed"] == tc.SEED
    dig = lambda b: hashlib.sha256(b).hexdigest()[:16]  # noqa: E731
    cases = tc.all_cases(with_big=True)
    assert [r["name"] for r in gold["cases"]] == [c.name for c in cases]
    for r, c in zip(gold["cases"], cases):
        assert r["blob"] == dig(c.blob) and r["out"] == dig(expected[c.name]), c.name
        assert r["oracle_only"] == bool(c.oracle_only)
