"""Cases of the tiled generic-width decode (psyne_amd/csrc/tdt_anyws.h: long blobs as 32 KiB output
tiles) and a numpy model of its arithmetic (psyne_amd/csrc/tdt_anyws_dec_tiles.h: block sums, the
clamped prefix, the per-tile block search, the clip, the placement), shared by
tests/test_anyws_dec_tiled_model.py (CPU: the model against the oracle, so the cases are right
before a GPU sees them) and tests/test_gpu_anyws_dec_tiled.py.

A case is a blob serialised (tests/decode_cases.serialize) from explicit per-stream (count, value)
arrays, so that pair, block and stream ends fall where the case says; `claims` lists what it says —
(stream, kind, stream position, argument) — and holds() checks each claim against the blob itself.
Deterministic, no fixture file: the digests are pinned in tests/golden/anyws_dec_tiled.json."""
from __future__ import annotations

import re
from collections import namedtuple

import numpy as np

from tests.anyws_cases import CSRC
from tests.anyws_tiled_cases import mapping_of
from tests.decode_cases import parse, serialize

WIDTHS = (3, 5, 12, 40, 64)
MAPPINGS = ("low", "high", "interleaved")
SEED = 0xDEC7113
BOUNDARY_KINDS = ("on", "before1", "after1", "straddle1", "straddle127", "straddle254", "zeros_before", "zeros_on",
                  "zeros_after")
NP_MODS = (1, 7, 8, 9, 2047, 2048, 2049)

Case = namedtuple("Case", "name ws blob claims oracle_only")


def _source_int(name: str) -> int:
    m = re.search(r"constexpr uint32_t %s = (\d+);" % name, (CSRC / "tdt_anyws_dec_tiles.h").read_text())
    return int(m.group(1))


def kernel_tile() -> int:
    """Output bytes per tile (kAnyDecTile)."""
    return _source_int("kAnyDecTile")


def block_pairs() -> int:
    """Pairs per block (kAnyDecBlockPairs)."""
    return _source_int("kAnyDecBlockPairs")


def tile_words(ws: int, tile: int) -> int:
    return tile // ws


def ntiles_of(orig: int, ws: int, tile: int) -> int:
    tw = tile_words(ws, tile)
    return (orig // ws + tw - 1) // tw


# --------------------------------------------------------------------------- building streams
class Pairs:
    """(count, value) pairs appended one run at a time; `pos` = the counts so far."""

    def __init__(self, rng):
        self.rng, self.c, self.pos, self.v = rng, [], 0, int(rng.integers(0, 256))

    def add(self, counts):
        counts = np.asarray(counts, np.int64).reshape(-1)
        self.c.append(counts)
        self.pos += int(counts.sum())

    def n(self):
        return sum(x.size for x in self.c)

    def fill_to(self, goal, maxrun):
        """Random counts in 1..maxrun up to position `goal` exactly."""
        while self.pos < goal:
            need = goal - self.pos
            c = self.rng.integers(1, maxrun + 1, max(8, 2 * need // (maxrun + 1) + 8))
            cs = np.cumsum(c)
            if cs[-1] >= need:
                i = int(np.searchsorted(cs, need))
                c = c[: i + 1]
                c[i] -= cs[i] - need
            self.add(c)

    def bytes(self, odd=False) -> bytes:
        c = np.concatenate(self.c) if self.c else np.zeros(0, np.int64)
        s = np.empty(2 * c.size + (1 if odd else 0), np.uint8)
        s[0:2 * c.size:2] = c
        # neighbouring pairs differ in value, so a misplaced pair shows
        s[1:2 * c.size:2] = (self.v + 1 + 5 * np.arange(c.size)) & 0xFF
        if odd:
            s[-1] = 0xEE
        return s.tobytes()


def boundary_feature(p: Pairs, q: int, kind: str, S: int, maxrun: int):
    """Bring the stream to tile boundary position q with feature `kind` there."""
    if kind == "on":
        p.fill_to(q, maxrun)
    elif kind == "before1":
        p.fill_to(q - 1, maxrun)
        p.add([min(5, S - p.pos)])
    elif kind == "after1":
        p.fill_to(q - 3, maxrun)
        p.add([min(4, S - p.pos)])
    elif kind.startswith("straddle"):
        near = int(kind[8:])
        p.fill_to(q - near, maxrun)
        p.add([min(255, S - p.pos)])
    elif kind == "zeros_before":
        p.fill_to(q - 2, maxrun)
        p.add([0] * 5 + [2])
    elif kind == "zeros_on":
        p.fill_to(q, maxrun)
        p.add([0] * 5)
    elif kind == "zeros_after":
        p.fill_to(q, maxrun)
        p.add([1] + [0] * 5)
    else:
        raise ValueError(kind)


def pad_pairs_to(p: Pairs, mod: int, want: int):
    """Count-0 pairs until the pair count is `want` modulo `mod`."""
    p.add([0] * ((want - p.n()) % mod))


# --------------------------------------------------------------------------- blobs
def layout_ids(layout: str):
    """Stored stream ids of the two referenced streams among unused ones: 'plain' none, 'before',
    'between', 'after', 'all' (an unused stream before, between and after)."""
    return {"plain": (0, 1, 2), "before": (1, 2, 3), "between": (0, 2, 3), "after": (0, 1, 3), "all": (1, 3, 5)}[layout]


def make_blob(rng, ws, orig, mapping, streams, layout="plain", wide=False):
    """mapping: position -> referenced stream index (0, 1, ...); streams: their bytes."""
    if len(streams) > 2:
        ids, ns = list(range(len(streams))), len(streams)
    else:
        a, b, ns = layout_ids(layout)
        ids = [a, b]
    stored = [Pairs(rng) for _ in range(ns)]
    for s in stored:  # unused streams: a few pairs nothing may read as data
        s.fill_to(int(rng.integers(0, 40)), 7)
    stored = [s.bytes(odd=bool(i & 1)) for i, s in enumerate(stored)]
    for r, sb in enumerate(streams):
        stored[ids[r]] = sb
    full = [ids[m] for m in mapping]
    if wide:
        full += [int(rng.integers(-2 ** 31, 2 ** 31)) for _ in range(2)]
    return serialize(orig, ws, full, stored)


def _k(mapping, r):
    return sum(1 for m in mapping if m == r)


def build_cases(tile: int):
    rng = np.random.default_rng(SEED)
    bp = block_pairs()
    cases, combos = [], [(ws, mk) for ws in WIDTHS for mk in MAPPINGS]
    feat = [0]

    def geometry(ws, tiles, extra_words=0, tail=0):
        tw = tile_words(ws, tile)
        wc = tiles * tw + extra_words
        return wc, wc * ws + tail

    def add(name, ws, mkind, orig, streams, claims, layout="plain", wide=False, mapping=None, oracle_only=False):
        mapping = mapping_of(ws, mkind) if mapping is None else mapping
        blob = make_blob(rng, ws, orig, mapping, streams, layout, wide)
        assert 66000 <= orig <= 174000 or oracle_only, (name, orig)
        cases.append(Case("ws%d_%s_%s" % (ws, mkind, name), ws, blob, tuple(claims), oracle_only))

    # ---- tile boundaries: every feature at boundaries of both streams, cycling over widths and mappings
    for rep in range(2):
        for ci, (ws, mk) in enumerate(combos):
            tiles = 2 + (ci + rep) % 3  # two to four whole tiles and a partial one
            wc, orig = geometry(ws, tiles, extra_words=tile_words(ws, tile) // 3 + 1, tail=(0, 1, ws - 1)[ci % 3])
            mapping, streams, claims = mapping_of(ws, mk), [], []
            for r in (0, 1):
                k, p = _k(mapping, r), Pairs(rng)
                S = wc * k
                for t in range(1, tiles + 1):
                    kind = BOUNDARY_KINDS[feat[0] % len(BOUNDARY_KINDS)]
                    feat[0] += 1
                    q = t * tile_words(ws, tile) * k
                    boundary_feature(p, q, kind, S, (255, 3, 40)[(ci + r) % 3])
                    claims.append((r, kind, q, 0))
                p.fill_to(S, 255)
                streams.append(p.bytes())
            add("bound%d" % rep, ws, mk, orig, streams, claims, wide=(ci % 5 == 0))

    # ---- block boundaries: maxrun 1..3 (a tile spans many blocks); a block boundary on a tile
    # boundary, one pair before and one pair after it
    for ci, (ws, mk) in enumerate(combos):
        wc, orig = geometry(ws, 2, extra_words=200, tail=(1, ws - 1, 0)[ci % 3])
        mapping, streams, claims = mapping_of(ws, mk), [], []
        for r in (0, 1):
            k, p = _k(mapping, r), Pairs(rng)
            q, delta = tile_words(ws, tile) * k, (0, -1, 1)[(ci + r) % 3]
            p.fill_to(q - 1, 1 + (ci + r) % 3)
            pad_pairs_to(p, bp, (delta - 1) % bp)
            p.add([1])  # the pair that reaches q: `delta` pairs past a block boundary
            claims.append((r, "block_at", q, delta % bp))
            p.fill_to(wc * k, 1 + (ci + r + 1) % 3)
            pad_pairs_to(p, bp, NP_MODS[(ci + r) % len(NP_MODS)] % bp)
            claims.append((r, "np_mod", 0, NP_MODS[(ci + r) % len(NP_MODS)] % bp))
            streams.append(p.bytes())
        add("blocks", ws, mk, orig, streams, claims)

    # ---- whole blocks of count-0 pairs: one and two in a row, at a tile's first byte and mid-tile
    for ci, (ws, mk) in enumerate(combos[::2]):
        wc, orig = geometry(ws, 3)
        mapping, streams, claims = mapping_of(ws, mk), [], []
        for r in (0, 1):
            k, p = _k(mapping, r), Pairs(rng)
            tq = tile_words(ws, tile) * k
            q = tq if (ci + r) % 2 == 0 else tq + tq // 2
            nz = 1 + (ci // 2 + r) % 2
            p.fill_to(q - 1, 3)
            pad_pairs_to(p, bp, bp - 1)
            p.add([1])
            p.add([0] * (nz * bp))
            claims.append((r, "zero_blocks", q, nz))
            p.fill_to(wc * k, 200)
            streams.append(p.bytes())
        add("zeroblk", ws, mk, orig, streams, claims)

    # ---- short streams
    short = ("mid_tile", "on_boundary", "one_into_last", "empty", "zeros_only", "odd_byte")
    for ci, (ws, mk) in enumerate(combos):
        kind = short[ci % len(short)]
        wc, orig = geometry(ws, 2, extra_words=200, tail=ws - 1)
        mapping, streams, claims = mapping_of(ws, mk), [], []
        for r in (0, 1):
            k, p = _k(mapping, r), Pairs(rng)
            tq, odd = tile_words(ws, tile) * k, False
            if r == ci % 2:  # the short one; the other stream is exact
                end = {"mid_tile": tq + tq // 2, "on_boundary": 2 * tq, "one_into_last": 2 * tq + 1, "empty": 0,
                       "zeros_only": 0, "odd_byte": 0}[kind]
                p.fill_to(end, 3 if end else 1)
                if kind == "zeros_only":
                    p.add([0] * 3000)
                odd = kind == "odd_byte"
                claims.append((r, "total", end, 0))
            else:
                p.fill_to(wc * k, 255)
            streams.append(p.bytes(odd=odd))
        add("short_" + kind, ws, mk, orig, streams, claims)

    # ---- long streams: an excess of 1 byte and of several tiles, an odd trailing byte
    for ci, (ws, mk) in enumerate(combos[1::2]):
        wc, orig = geometry(ws, 3, extra_words=1)  # wc = 1 (mod Tw): the last tile is one word
        mapping, streams, claims = mapping_of(ws, mk), [], []
        for r in (0, 1):
            k, p = _k(mapping, r), Pairs(rng)
            excess = 1 if (ci + r) % 2 == 0 else 3 * tile_words(ws, tile) * k + 11
            p.fill_to(wc * k + excess, (255, 2)[(ci + r) % 2])
            claims.append((r, "total", wc * k + excess, 0))
            streams.append(p.bytes(odd=True))
        add("long", ws, mk, orig, streams, claims, layout=("before", "between", "after", "all")[ci % 4], wide=(ci % 2 == 1))

    # ---- shape: wc = ntiles * Tw exactly; one referenced stream only; three referenced streams
    for ci, (ws, mk) in enumerate(combos[::3]):
        wc, orig = geometry(ws, 3)
        mapping = mapping_of(ws, mk)
        streams = []
        for r in (0, 1):
            p = Pairs(rng)
            p.fill_to(wc * _k(mapping, r), (1, 255)[r])
            streams.append(p.bytes())
        add("whole_tiles", ws, mk, orig, streams, [], layout="all")
    for ws in WIDTHS:
        wc, orig = geometry(ws, 2, extra_words=200, tail=1)
        p = Pairs(rng)
        p.fill_to(wc * ws - 1000, 40)  # (a little short)
        add("one_stream", ws, "single", orig, [p.bytes()], [], layout="between", mapping=[0] * ws)
        m3 = [p % 3 for p in range(ws)]
        streams = []
        for r in range(3):
            p = Pairs(rng)
            p.fill_to(wc * _k(m3, r), 9)
            streams.append(p.bytes())
        add("three_streams", ws, "three", orig, streams, [], mapping=m3)
    return cases


def past_2_32_case(tile: int) -> Case:
    """One stream of 16,843,010 pairs of count 255 (4,294,967,550 bytes decoded) in a 33.7 MB blob
    whose output is three tiles.  Oracle only: a full expansion would take 4 GiB."""
    rng = np.random.default_rng(SEED + 1)
    ws, mapping = 12, mapping_of(12, "low")
    orig = 3 * tile_words(ws, tile) * ws
    n = 16843010
    s0 = np.empty(2 * n, np.uint8)
    s0[0::2] = 255
    s0[1::2] = (np.arange(n) // 3) & 0xFF
    p = Pairs(rng)
    p.fill_to((orig // ws) * _k(mapping, 1), 255)
    blob = make_blob(rng, ws, orig, mapping, [s0.tobytes(), p.bytes()])
    return Case("ws12_low_past_2_32", ws, blob, ((0, "total", 255 * n, 0),), True)


_CACHE = {}


def all_cases(with_big=False):
    """Every case in a fixed order (built once per process); with_big: the 2^32 case last."""
    if "cases" not in _CACHE:
        _CACHE["cases"] = build_cases(kernel_tile())
        assert len({c.name for c in _CACHE["cases"]}) == len(_CACHE["cases"])
    if with_big and "big" not in _CACHE:
        _CACHE["big"] = past_2_32_case(kernel_tile())
    return _CACHE["cases"] + ([_CACHE["big"]] if with_big else [])


# --------------------------------------------------------------------------- what a case claims
def referenced(blob):
    """(orig, ws, [(stream id, positions P, counts, values)]) of a blob, the streams in the order of
    their first position."""
    orig, _, ws, _, mapping, streams = parse(blob)
    out, seen = [], []
    for m in mapping:
        if m not in seen:
            seen.append(m)
    for s in seen:
        raw = np.frombuffer(streams[s], np.uint8)
        n = raw.size // 2
        out.append((s, [p for p in range(ws) if mapping[p] == s], raw[0:2 * n:2].astype(np.int64), raw[1:2 * n:2]))
    return orig, ws, out


def holds(case: Case, tile: int):
    """Assert every claim of the case against its blob."""
    orig, ws, refs = referenced(case.blob)
    bp = block_pairs()
    by_logical = {}
    mapping = parse(case.blob)[4]
    for r, m in enumerate(sorted(set(mapping))):  # logical stream r = the r-th smallest stored id
        by_logical[r] = next(x for x in refs if x[0] == m)
    for r, kind, q, arg in case.claims:
        _, P, counts, _ = by_logical[r]
        ends = np.cumsum(counts)
        starts = ends - counts
        if kind in ("on", "zeros_on", "zeros_after"):
            assert q in ends, (case.name, kind)
        if kind == "before1":
            assert q - 1 in ends and q not in ends, case.name
        if kind == "after1":
            assert q + 1 in ends and q not in ends, case.name
        if kind.startswith("straddle"):
            i = int(np.searchsorted(ends, q, "right"))
            assert starts[i] == q - int(kind[8:]) and ends[i] > q, case.name
        if kind == "zeros_before":
            i = int(np.flatnonzero(ends == q)[0])
            assert counts[i] == 2 and (counts[i - 5:i] == 0).all(), case.name
        if kind == "zeros_on":
            i = int(np.flatnonzero(ends == q)[0])
            assert (counts[i + 1:i + 6] == 0).all(), case.name
        if kind == "zeros_after":
            i = int(np.flatnonzero(ends == q)[-1])
            assert counts[i - 5:i].sum() == 0 or (counts[np.flatnonzero(ends == q + 1)[0] + 1:][:5] == 0).all(), case.name
        if kind == "block_at":  # the first pair that starts at q is `arg` pairs past a block boundary
            i = int(np.flatnonzero((starts == q) & (counts > 0))[0])
            assert i % bp == arg, (case.name, i % bp, arg)
        if kind == "np_mod":
            assert counts.size % bp == arg, case.name
        if kind == "zero_blocks":
            i = int(np.flatnonzero((starts == q) & (counts == 0))[0])
            assert i % bp == 0 and (counts[i:i + arg * bp] == 0).all() and counts[i + arg * bp] > 0, case.name
        if kind == "total":
            assert int(counts.sum()) == q, case.name
    assert 2 <= ntiles_of(orig, ws, tile) or case.oracle_only


# --------------------------------------------------------------------------- the model
def model_decode(blob: bytes, tile: int) -> bytes:
    """The output of the tile pipeline, computed the way it computes it: per stream the block sums
    and their exclusive prefix clamped at the stream's share; per tile and stream the largest block
    whose prefix is at most the range's start, the blocks walked from there with every pair cut to
    the range and expanded into the stream's plane (zero first); the planes scattered to the
    positions of the tile's words; zeros past the last whole word."""
    orig, ws, refs = referenced(blob)
    bp = block_pairs()
    wc = orig // ws
    tw = tile_words(ws, tile)
    out = np.full(orig, 0xEE, np.uint8)
    prefix = []
    for _, P, counts, _ in refs:
        S = wc * len(P)
        sums = np.add.reduceat(counts, np.arange(0, counts.size, bp)) if counts.size else np.zeros(0, np.int64)
        assert (sums <= bp * 255).all()
        prefix.append(np.minimum(np.concatenate([[0], np.cumsum(sums)[:-1]]), S) if sums.size else sums)
    for t in range((wc + tw - 1) // tw):
        w0, w1 = t * tw, min((t + 1) * tw, wc)
        words = np.zeros((w1 - w0, ws), np.uint8)
        for (_, P, counts, values), E in zip(refs, prefix):
            k = len(P)
            q0, q1 = w0 * k, w1 * k
            plane = np.zeros(q1 - q0, np.uint8)
            if counts.size:
                b = int(np.searchsorted(E, q0, "right")) - 1  # the largest b with E[b] <= q0
                sbase = int(E[b])
                pc = b * bp
                while pc < counts.size and sbase < q1:
                    c, v = counts[pc:pc + bp], values[pc:pc + bp]
                    ends = sbase + np.cumsum(c)
                    lo, hi = np.clip(ends - c, q0, q1), np.clip(ends, q0, q1)
                    n = hi - lo
                    idx = np.repeat(lo - q0 - (np.cumsum(n) - n), n) + np.arange(int(n.sum()))
                    plane[idx] = np.repeat(v, n)
                    sbase = int(ends[-1])
                    pc += bp
            words[:, P] = plane.reshape(w1 - w0, k)
        out[w0 * ws:w1 * ws] = words.reshape(-1)
    out[wc * ws:] = 0
    return out.tobytes()
