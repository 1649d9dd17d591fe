"""Run-structured encode cases: runs whose starts, ends and 255-cap chunk starts sit on, one byte
before and one byte behind every boundary of the encode kernels, at every tuned width and stream
split.  No GPU and no fixture bytes: everything follows from SEED.  The record of what the compiled
reference makes of them is tests/golden/encode_runs.json (tests/golden/make_encode_runs.py); the CPU
test is tests/test_encode_runs.py, the GPU routes tests/test_gpu_encode_runs.py.

A message is built from its streams, not from words: stream 0 (the positions mapped to 0) holds two
values in geometric runs of mean 3, stream 1 bytes that differ from their predecessor (every slot a
run start), so the analysed mapping is the intended one by a wide entropy gap.  Edges then overwrite
stream bytes around a boundary, in both streams independently:

    end    a run of L bytes whose successor starts at s_b + d
    start  a run of L bytes that starts at s_b + d
    cap    a run of L > 255 j bytes that starts at s_b + d - 255 j, j = 1..3: its j-th cap chunk
           starts at s_b + d

with L from LENGTHS and d from DS.  The bytes before and behind a run are patched so that it has
exactly its length; edges neither touch nor overlap, and those of a stream take at most half of it.
In two of every three variants the first and last 16 message bytes are BOOKEND, so that in a
contiguous batch a message ends on the byte its successor starts with.

Families: `edge` (the above at the tuned widths), `span` (the same at SIZE_SPAN), `capex_clean`,
`capex_dirty`, `capex_256` (runs around the cap-exclusion rule of pass A1) and `generic` (widths
3, 12 and 40 at the boundaries of tdt_anyws.hip)."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests.anyws_cases import intended_mapping, kernel_chunk

SEED = 0xE2C0DE
TUNED = (1, 2, 4, 8, 16)
GENERIC = (3, 12, 40)
# the class edges of tdt_api.hip (kSmallMax = 4096, kMidMax = 32768, kBigMin = 65536) and the smallest
# shapes behind them: 8192 gives RW = 2, 100024 is n % 16 = 8, 196640 three tiles and a partial one
SIZES = (1024, 4096, 4112, 8192, 32768, 32784, 65536, 65552, 100016, 100024, 196640)
SIZE_PARTIAL = 100024  # no multiple of 16: widths up to 8
SIZE_SPAN = 589840     # crosses a 512 KiB span: widths 2..16, SPAN_CASES messages each
SPAN_CASES = 3
SIZE_CAPEX = 65536
SIZES_GENERIC = (4200, 20520, 65640)  # multiples of 120 near 4 KiB, 20 KiB and 64 KiB
VARIANTS = 3
BOOKEND = 0x5A
LENGTHS = (1, 2, 254, 255, 256, 257, 509, 510, 511, 765, 766, 1020, 1021)
CAP_LENGTHS = tuple(L for L in LENGTHS if L > 255)
DS = (-1, 0, 1)
PLACEMENTS = ("end", "start", "cap")
KINDS = ("start", "end", "group", "block", "round", "wave", "tile", "span")
GENERIC_KINDS = ("start", "end", "lane", "chunk")
COMBOS = tuple((p, d) for p in PLACEMENTS for d in DS)
SPAN_COMBOS = tuple((p, 0) for p in PLACEMENTS)
# what fits at a stream's two ends: nothing lies before byte 0, no slot at the stream's length
FEASIBLE = {"start": (("start", 0), ("start", 1), ("end", 1)),
            "end": (("end", 0), ("end", -1), ("start", -1), ("cap", -1))}
CAPEX_OUTCOMES = ("clean", "dirty", "256")

GROUP = 16          # bytes per group
ROUND_GROUPS = 64   # one group per lane
TILE_GROUPS = 4096  # kTileGroups
SPAN_GROUPS = 8 * TILE_GROUPS  # kSpanTiles tiles


class Case(NamedTuple):
    name: str
    ws: int
    mapping: tuple
    n: int
    family: str
    message: np.ndarray


EDGES: dict = {}  # case name -> [(stream, kind, placement, d, L, the run's first stream byte)], filled by all_cases()


def mappings(ws: int) -> list:
    """k1 = 1, ws/2 and ws - 1 positions in stream 1, each with stream 1 on the low positions, on the
    high ones (the float-like layout) and interleaved; width 1 has the one mapping [0]."""
    if ws == 1:
        return [(0,)]

    def inter(k1):
        if 2 * k1 > ws:
            return tuple(1 - m for m in inter(ws - k1))
        pos = {(1 + (i * ws) // k1) % ws for i in range(k1)}
        return tuple(1 if b in pos else 0 for b in range(ws))

    out = []
    for k1 in sorted({1, ws // 2, ws - 1}):
        for m in (tuple(1 if b < k1 else 0 for b in range(ws)), tuple(1 if b >= ws - k1 else 0 for b in range(ws)),
                  inter(k1)):
            if m not in out:
                out.append(m)
    return out


def shares(ws: int, mapping) -> list:
    """k_c: the positions of stream c (one entry for a one-stream mapping)."""
    k1 = sum(mapping)
    return [ws - k1, k1] if k1 else [ws]


def geometry(ws: int, mapping, n: int) -> dict:
    """The encode kernels' decomposition of an n-byte message, restated from
    psyne_amd/csrc/tdt_encode.h and tdt_api.hip:

    * groups of 16 bytes, wave w owns groups [w RW 64, (w + 1) RW 64), a round is 64 groups
      (tdt_encode.h:14-18; `gw0 = tg0 + wv * RW * 64`, :522; `RW = (tgn + TEAM - 1) / TEAM`, :517);
    * TEAM = 64 up to kSmallMax = 4096 bytes, 256 up to kMidMax = 32768, 512 above
      (tdt_api.hip:452-459, DESIGN.md §4 "message classes");
    * Ls_c = (16 / ws) k_c slots of stream c per group (EncLayout::WPG, :139);
    * pass A1's cap-exclusion block: 8 groups, 4 where Ls = 16 (:1382-1398);
    * a tile is kTileGroups = 4096 groups (:65), a span kSpanTiles = 8 tiles (:66); inside a tile
      the 512-lane team gives each wave 8 rounds (`RW = kTileGroups / 64`, :517)."""
    ngroups = (n + GROUP - 1) // GROUP
    team = 64 if n <= 4096 else 256 if n <= 32768 else 512
    ks = shares(ws, mapping)
    ls = [(GROUP // ws) * k for k in ks]
    return dict(ngroups=ngroups, team=team, rw=(ngroups + team - 1) // team, ls=ls,
                block=[4 if x == 16 else 8 for x in ls], lens=[(n // ws) * k for k in ks])


def boundaries(ws: int, mapping, n: int, rng) -> list:
    """[(kind, group or None)] per stream: every wave, tile and span boundary of the message, two
    wave boundaries of its tiles, and seeded picks of the group, block and round kinds."""
    g = geometry(ws, mapping, n)
    ng = g["ngroups"]
    out = []
    for c in range(len(g["ls"])):
        b = [("start", 0), ("end", None)]
        if n > 65536:  # (the rarest kinds first: a neighbour's long run may not take their place)
            b += sorted((("span" if t % SPAN_GROUPS == 0 else "tile", t) for t in range(TILE_GROUPS, ng, TILE_GROUPS)))
        b += [("wave", w * g["rw"] * ROUND_GROUPS) for w in range(1, g["team"] // 64) if w * g["rw"] * ROUND_GROUPS < ng]
        if n > 65536:
            inner = [x for x in range(512, ng, 512) if x % TILE_GROUPS]
            b += [("wave", int(x)) for x in rng.choice(inner, 2, replace=False)]
        b += [("group", int(x)) for x in rng.integers(1, ng, 3)]
        blk = g["block"][c]
        b += [("block", blk * int(x)) for x in rng.integers(1, (ng + blk - 1) // blk, 2)]
        if ng > ROUND_GROUPS:
            b += [("round", ROUND_GROUPS * int(x)) for x in rng.integers(1, (ng + 63) // 64, 2)]
        out.append(b)
    return out


class _Cycles:
    """Round-robin counters of the lengths per width, and per width, stream and kind how often each
    (placement, d) was placed: the rarest is tried first, so coverage comes by construction."""

    def __init__(self):
        self.at = {}

    def next(self, key, seq):
        i = self.at.get(key, 0)
        self.at[key] = i + 1
        return seq[i % len(seq)]


def background(c: int, length: int, rng, dense: bool = False) -> tuple:
    """(stream bytes, the two values of stream 0 or None).  dense: stream 0's runs are 1 or 2 bytes."""
    if c == 1:
        return np.cumsum(rng.integers(1, 256, length)).astype(np.uint8), None
    a, b = (int(x) for x in rng.choice(256, 2, replace=False))
    m = length // 2 + 64 if not dense else length + 1
    runs = rng.geometric(1.0 / 3.0, m) if not dense else rng.integers(1, 3, m)
    idx = np.repeat(np.arange(m) & 1, runs)[:length]
    assert idx.size == length
    return np.where(idx == 0, a, b).astype(np.uint8), (a, b)


def put_run(s: np.ndarray, a: int, L: int, vals, rng, turn: int):
    """A run of exactly L bytes at s[a:a + L]: its value, and other values on either side."""
    v = vals[turn & 1] if vals else int(rng.integers(0, 256))
    other = (vals[1 - (turn & 1)]) if vals else (v ^ 0x80)
    s[a:a + L] = v
    if a > 0 and s[a - 1] == v:
        s[a - 1] = other
    if a + L < s.size and s[a + L] == v:
        s[a + L] = other


def place_edges(s, vals, key, c, bounds, lo, hi, cyc, rng) -> list:
    """One edge per boundary (kind, stream byte) where one fits in s[lo:hi]."""
    taken, out = [], []
    budget = s.size // 2
    for kind, sb in bounds:
        combos = SPAN_COMBOS if kind == "span" else tuple(FEASIBLE[kind]) if kind in FEASIBLE else COMBOS
        placed = cyc.at.setdefault((key, c, kind), {})
        for placement, d in sorted(combos, key=lambda pd: (placed.get(pd, 0), combos.index(pd))):  # the rarest first
            j = 0
            if placement == "cap":
                L = cyc.next((key, "capL"), CAP_LENGTHS)
                j = 1 + cyc.next((key, "j"), (0, 1, 2)) % ((L - 1) // 255)
                if kind == "end":
                    L = 255 * j - d
                a = sb + d - 255 * j
            else:
                L = cyc.next((key, "L"), LENGTHS)
                if kind in FEASIBLE and placement != kind:  # the one-byte run at a stream's end
                    L = abs(d)
                a = sb + d - L if placement == "end" else sb + d
            if a < lo or a + L > hi or L > budget or any(x < a + L + 1 and a - 1 < y for x, y in taken):
                continue
            put_run(s, a, L, vals, rng, len(out))
            taken.append((a - 1, a + L + 1))
            budget -= L
            out.append((c, kind, placement, d, L, a))
            placed[(placement, d)] = placed.get((placement, d), 0) + 1
            break
    return out


def assemble(ws, mapping, streams) -> np.ndarray:
    wc = streams[0].size // shares(ws, mapping)[0]
    msg = np.empty((wc, ws), np.uint8)
    for c, s in enumerate(streams):
        pos = [b for b in range(ws) if mapping[b] == c]
        msg[:, pos] = s.reshape(wc, len(pos))
    return msg.reshape(-1)


def _name(ws, mapping, n, tag):
    return "ws%d_m%s_n%d_%s" % (ws, "".join(str(m) for m in mapping), n, tag)


def edge_case(ws, mapping, n, variant, family, cyc) -> Case:
    rng = np.random.default_rng([SEED, ws, sum(m << b for b, m in enumerate(mapping)), n, variant])
    geo = geometry(ws, mapping, n)
    bookend = variant % 3 != 2
    streams, edges = [], []
    for c, bounds in enumerate(boundaries(ws, mapping, n, rng)):
        s, vals = background(c, geo["lens"][c], rng)
        ls = geo["ls"][c]
        be = ls + 1 if bookend else 0  # the bookend's bytes of this stream, and the patched neighbour
        sb = [(k, s.size if g is None else g * ls) for k, g in bounds if not (bookend and k in FEASIBLE)]
        edges += place_edges(s, vals, ws, c, sb, be, s.size - be, cyc, rng)
        streams.append(s)
    msg = assemble(ws, mapping, streams)
    if bookend:
        msg[:16] = BOOKEND
        msg[-16:] = BOOKEND
    name = _name(ws, mapping, n, "v%d" % variant)
    EDGES[name] = edges
    return Case(name, ws, tuple(mapping), n, family, msg)


# ------------------------------------------------------------------ cap-exclusion family
def capex_case(ws, mapping, c, outcome) -> Case:
    """Runs of (B - 1) Ls .. 256 + Ls bytes in stream c, one per phase of an aligned B-group block,
    kept when they give the wanted outcome: `clean` (every aligned block keeps a run start), `dirty`
    (a block without one, every run below 256) or `256` (runs of exactly 256 at every phase, then
    257 .. 256 + Ls)."""
    n = SIZE_CAPEX
    rng = np.random.default_rng([SEED, 0xCA9, ws, sum(m << b for b, m in enumerate(mapping)), c, CAPEX_OUTCOMES.index(outcome)])
    geo = geometry(ws, mapping, n)
    streams = [background(x, geo["lens"][x], rng, dense=True) for x in range(len(geo["ls"]))]
    s, vals = streams[c]
    ls, blk = geo["ls"][c], geo["block"][c] * geo["ls"][c]
    low = blk - ls
    at, placed = blk, 0
    for i in range(8 * blk):
        phase = i % blk
        if outcome == "256":
            L = 256 if i < blk else 257 + (i - blk) % ls
        elif outcome == "clean":  # (B - 1) Ls .. 2 B Ls: clean or not by the phase
            L = min(low + i % (blk + ls), 255)
        else:
            L = blk + 1 + (i * 37) % (255 - blk)
        a = at + phase
        if a + L + 2 * blk > s.size:
            break
        x0 = (a // blk + 1) * blk  # the first aligned block that starts behind the run's start
        dirty = a + L >= x0 + blk
        if outcome != "256" and dirty != (outcome == "dirty"):
            continue
        put_run(s, a, L, vals, rng, placed)
        placed += 1
        at = ((a + L) // blk + 2) * blk
    assert placed >= 8, (ws, mapping, c, outcome, placed)
    name = _name(ws, mapping, n, "capex_s%d_%s" % (c, outcome))
    EDGES[name] = []
    return Case(name, ws, tuple(mapping), n, "capex_" + outcome, assemble(ws, mapping, [x for x, _ in streams]))


# ------------------------------------------------------------------ generic widths
def stream_index(ws, mapping, c, j: int) -> int:
    """How many bytes of stream c lie before message byte j (generic word sizes:
    (j / ws) k_c + the positions below j mod ws in stream c)."""
    return (j // ws) * sum(1 for m in mapping if m == c) + sum(1 for b in range(j % ws) if mapping[b] == c)


def generic_case(ws, n, variant, cyc) -> Case:
    """The edges at the boundaries of tdt_encode_any_kernel: the stream byte where each chunk of
    kAnyChunk message bytes ends, and a lane's 16 stream bytes inside a chunk."""
    mapping = tuple(intended_mapping(ws))
    chunk = kernel_chunk()
    rng = np.random.default_rng([SEED, 0x6E, ws, n, variant])
    bookend = variant % 3 != 2
    streams, edges = [], []
    for c in (0, 1):
        k = sum(1 for m in mapping if m == c)
        s, vals = background(c, (n // ws) * k, rng)
        starts = [stream_index(ws, mapping, c, j) for j in range(0, n, chunk)] + [s.size]
        sb = [] if bookend else [("start", 0), ("end", s.size)]
        sb += [("chunk", x) for x in starts[1:-1]]
        for ch in rng.integers(0, len(starts) - 1, 8):
            lanes = (starts[ch + 1] - starts[ch]) // 16
            if lanes > 1:
                sb.append(("lane", starts[ch] + 16 * int(rng.integers(1, lanes))))
        sb = [sb[i] for i in rng.permutation(len(sb))]  # (a short stream's budget goes to no kind first)
        be = (16 // ws + 2) * k + 1 if bookend else 0
        edges += place_edges(s, vals, ws, c, sb, be, s.size - be, cyc, rng)
        streams.append(s)
    msg = assemble(ws, mapping, streams)
    if bookend:
        msg[:16] = BOOKEND
        msg[-16:] = BOOKEND
    name = _name(ws, mapping, n, "g%d" % variant)
    EDGES[name] = edges
    return Case(name, ws, mapping, n, "generic", msg)


# ------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=1)
def _all() -> tuple:
    EDGES.clear()
    cyc = _Cycles()
    out = []
    for ws in TUNED:
        maps = mappings(ws)
        for mapping in maps:
            for n in SIZES:
                if n == SIZE_PARTIAL and ws > 8:
                    continue
                out += [edge_case(ws, mapping, n, v, "edge", cyc) for v in range(VARIANTS)]
        if ws > 1:
            # (the variants 2, 3, 4: the first has no bookends, so the span edges meet both kinds of ends)
            out += [edge_case(ws, maps[(i * 7) % len(maps)], SIZE_SPAN, 2 + i, "span", cyc) for i in range(SPAN_CASES)]
        for i, k1 in enumerate(sorted({sum(m) for m in maps})):
            mapping = [m for m in maps if sum(m) == k1][i % 3 if ws > 2 else 0]
            for c in range(len(shares(ws, mapping))):
                out += [capex_case(ws, mapping, c, o) for o in CAPEX_OUTCOMES]
    for ws in GENERIC:
        out += [generic_case(ws, n, v, cyc) for n in SIZES_GENERIC for v in range(VARIANTS)]
    assert len({c.name for c in out}) == len(out)
    for c in out:
        c.message.setflags(write=False)
    return tuple(out)


def all_cases() -> list:
    """Every case as (name, ws, mapping, n, family, message); built once, the messages read-only."""
    return list(_all())


def check_coverage(cases):
    """At every tuned width and in each stream that exists: every kind but span with every placement
    and every d that fits (FEASIBLE at a stream's two ends), span (widths 2..16) with the three
    placements at d = 0; every L at every width; the three cap-exclusion outcomes at every width; at
    the generic widths every placement and d at lane and chunk boundaries and an edge at either end."""
    seen, lengths, outcomes = {}, {}, {}
    for c in cases:
        for s, kind, placement, d, L, _ in EDGES[c.name]:
            seen.setdefault((c.ws, s, kind), set()).add((placement, d))
            lengths.setdefault(c.ws, set()).add(L)
        if c.family.startswith("capex_"):
            outcomes.setdefault(c.ws, set()).add(c.family[6:])
    for ws in TUNED:
        for s in range(1 if ws == 1 else 2):
            for kind in KINDS:
                if kind == "span":
                    want = set(SPAN_COMBOS) if ws > 1 else set()
                else:
                    want = set(FEASIBLE.get(kind, COMBOS))
                missing = want - seen.get((ws, s, kind), set())
                assert not missing, "width %d stream %d kind %s lacks %s" % (ws, s, kind, sorted(missing))
        assert lengths[ws] >= set(LENGTHS), "width %d lacks lengths %s" % (ws, sorted(set(LENGTHS) - lengths[ws]))
        assert outcomes.get(ws) == set(CAPEX_OUTCOMES), "width %d: cap-exclusion outcomes %s" % (ws, outcomes.get(ws))
    for ws in GENERIC:
        for s in (0, 1):
            for kind in GENERIC_KINDS:
                got = seen.get((ws, s, kind), set())
                if kind in FEASIBLE:  # (three messages without bookends per width: some edge at either end)
                    assert got, "width %d stream %d has no edge at its %s" % (ws, s, kind)
                    continue
                assert not set(COMBOS) - got, "width %d stream %d kind %s lacks %s" % (ws, s, kind, sorted(set(COMBOS) - got))
