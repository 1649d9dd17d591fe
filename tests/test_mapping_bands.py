"""The mapping-decision fixtures (tests/golden/mapping_bands.json) on the CPU: the cases cover what
they claim to cover, judged from the oracle's own entropies; the oracle decides every one of them as
the reference codec did when the fixture was made; and, where the compiled reference is present, the
oracle's blob is the reference's byte for byte."""
import zlib

import numpy as np
import pytest

from oracle.oracle import Oracle, Reference
from tests import mapping_band_cases as mb


@pytest.fixture(scope="module")
def cases():
    return mb.load_cases()


@pytest.fixture(scope="module")
def analysed(cases):
    orc = Oracle()
    return [orc.analyze(c["input"], word_size=c["ws"]) for c in cases]


def test_margin_is_the_sources():
    """The bands were laid around the margin the encoder is compiled with."""
    assert mb.load_meta()["margin"] == mb.fast_margin()


def test_rebuilding_is_deterministic(cases):
    """Twice the same bytes here, and the bytes the maker saw (one checksum over every message's)."""
    crcs = []
    for c in cases:
        again = mb.build(c)
        assert again.tobytes() == c["input"].tobytes() and again.size == c["size"], c["name"]
        crcs.append(zlib.crc32(again.tobytes()).to_bytes(4, "little"))
    assert zlib.crc32(b"".join(crcs)) == mb.load_meta()["crc32"]


def test_coverage_table(cases, analysed):
    M = mb.fast_margin()
    assert mb.FIXTURE.stat().st_size < 512 * 1024
    assert sum(len(c["syms"]) > 64 for c in cases) <= 32 and all(len(c["syms"]) <= 256 for c in cases)
    cells = {}
    for c, (hist, ent, mp) in zip(cases, analysed):
        cells.setdefault((c["ws"], c["size"]), []).append((c, ent, [int(x) for x in mp]))
        assert len(c["moves"]) <= 3 and len(c["mul"]) == c["ws"], c["name"]
    assert set(cells) == {(ws, size) for ws in mb.WIDTHS for size in mb.sizes_for(ws)}
    for (ws, size), rows in cells.items():
        n = size // ws
        near = [r for r in rows if r[0]["kind"] == "near"]
        indep = [r for r in rows if r[0]["kind"] == "indep"]
        ties = [r for r in rows if r[0]["kind"] == "tie"]
        assert len(near) + len(indep) + len(ties) == len(rows)
        # ---- every band in both signs, confirmed from the oracle's entropies with an exact mean
        got = sorted(mb.classify(c, ent, M) for c, ent, _ in near)
        want = sorted((b, s) for b in range(4) for s in mb.SIGNS) if ws > 1 else []
        assert got == want, (ws, size, got)
        for c, ent, mp in near:
            assert (c["band"], c["sign"]) == mb.classify(c, ent, M), c["name"]
            assert len(c["perturbed"]) == c["j"] and 1 <= len(c["moves"]), c["name"]
            assert mp == [int((b in c["perturbed"]) == (c["sign"] == "+")) for b in range(ws)], c["name"]
        # ---- near ties between unrelated histograms: deepest inside the margin and just outside it
        got = sorted(mb.classify(c, ent, M) for c, ent, _ in indep)
        assert got == (sorted((b, s) for b in mb.INDEP_BANDS for s in mb.SIGNS) if ws > 1 else []), (ws, size, got)
        for c, ent, mp in indep:
            assert (c["band"], c["sign"]) == mb.classify(c, ent, M) and len(c["perturbed"]) == c["j"], c["name"]
            assert mp == [int((b in c["perturbed"]) == (c["sign"] == "+")) for b in range(ws)], c["name"]
            h = np.zeros((2, 256), np.int64)
            h[0, c["syms"]], h[1, c["alt_syms"]] = c["counts"], c["alt_counts"]
            assert int((h[0] != h[1]).sum()) > 6, c["name"]  # (kind `near` differs in at most six bins)
        if ws > 1:
            assert {c["j"] for c, _, _ in near} >= set(mb.j_values(ws)), (ws, size)
            assert len({tuple(c["perturbed"]) for c, _, _ in near}) >= min(4, ws), (ws, size)
        # ---- the exact ties
        assert {c["tie"] for c, _, _ in ties} >= set(mb.tie_kinds(n)), (ws, size)
        for c, ent, mp in ties:
            assert len({float(e) for e in ent}) == 1 and len(set(mp)) == 1, c["name"]
            counts = np.asarray(c["counts"])
            if c["tie"] == "const":
                assert counts.tolist() == [n]
            elif c["tie"] == "le64":
                assert counts.size > 1 and counts.max() <= 64
            elif c["tie"] == "gt64":
                assert counts.size > 1 and counts.min() > 64
            elif c["tie"] == "mixed":
                assert counts.min() <= 64 < counts.max()
        if ws in (3, 8, 12, 16):  # all zeros, and all ones (an empty stream 0)
            assert {mp[0] for _, _, mp in ties} == {0, 1}, (ws, size)
        # ---- above 64 KiB: the speculated mapping and another one in the bands next to the margin
        spec = mb.SPECULATED.get(ws)
        if spec is not None and size > 65536:
            for band in (1, 2):
                mps = [mp for c, _, mp in near if c["band"] == band]
                assert spec in mps and any(m != spec for m in mps), (ws, size, band)


def test_oracle_mapping_is_the_references(cases, analysed):
    for c, (_, _, mp) in zip(cases, analysed):
        assert "ref_mapping" in c, c["name"]
        assert [int(x) for x in mp] == c["ref_mapping"], c["name"]


@pytest.mark.skipif(not Reference.available(), reason="oracle/_ref not built (the reference sources were absent at build time)")
def test_oracle_blob_is_the_references(cases):
    orc, ref = Oracle(), Reference()
    for c in cases:
        want = ref.encode(c["input"], sample_fraction=1.0, word_size=c["ws"], bandwidth=10.0)
        got = orc.encode(c["input"], cfg=orc.config(word_size=c["ws"]), bandwidth=10.0)
        assert got == want, c["name"]
