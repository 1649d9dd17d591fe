"""Cases of the tiled generic-width encode (psyne_amd/csrc/tdt_anyws.h: long messages as 64 KiB
tiles) and a numpy model of its tile arithmetic, shared by tests/test_anyws_tiled_model.py (CPU: the
model against the oracle, so the cases are right before a GPU sees them) and
tests/test_gpu_anyws_tiled.py.

A case is a message built from two byte streams and a mapping (bit p of a word -> stream), so both
streams' run structure is chosen freely: the tests encode it with that mapping (the known-mapping
routes; Oracle.encode(mapping=...)) and again analysed (whatever mapping the entropies give)."""
import math
import re

import numpy as np

from tests.anyws_cases import CSRC

WIDTHS = (3, 5, 12, 40, 64)
MAPPINGS = ("low", "high", "interleaved")
CROSSING = (254, 255, 256, 510, 511, 765)


def kernel_tile() -> int:
    """The tiled encode's tile size in message bytes (kAnyTile, psyne_amd/csrc/tdt_anyws.h)."""
    m = re.search(r"constexpr uint32_t kAnyTile = (\d+);", (CSRC / "tdt_anyws.h").read_text())
    return int(m.group(1))


def mapping_of(ws: int, kind: str) -> list[int]:
    """Stream 1 at the low positions, the high ones, or every other one."""
    if kind == "low":
        return [1 if p < ws // 2 else 0 for p in range(ws)]
    if kind == "high":
        return [0 if p < ws // 2 else 1 for p in range(ws)]
    if kind == "interleaved":
        return [p & 1 for p in range(ws)]
    raise ValueError(kind)


def unit(ws: int) -> int:
    """Message sizes that compress are multiples of the word size and of 4."""
    return ws * 4 // math.gcd(ws, 4)


def round_up(n: int, ws: int) -> int:
    u = unit(ws)
    return (n + u - 1) // u * u


def stream_pos(j, ws, mapping, s):
    """Bytes of stream s before message byte j (the closed form the kernels use)."""
    before = np.concatenate([[0], np.cumsum([1 if m == s else 0 for m in mapping])])
    return (j // ws) * int(before[ws]) + int(before[j % ws])


def pred_pos(jb, ws, mapping, s):
    """The message byte holding the stream byte before stream position stream_pos(jb)."""
    for d in range(1, ws + 1):
        if mapping[(jb - d) % ws] == s:
            return jb - d
    raise ValueError("stream %d is empty" % s)


def stream_of(S: int, starts, seed: int) -> np.ndarray:
    """S bytes whose run starts are exactly `starts` (0 is always one): neighbouring runs differ."""
    st = np.unique(np.concatenate([[0], np.asarray([q for q in starts if 0 < q < S], np.int64)])).astype(np.int64)
    vals = np.empty(st.size, np.uint8)
    v = seed & 0xFF
    for i in range(st.size):
        v = (v * 5 + 3) & 0xFF  # (odd multiplier and step: never the same value twice in a row)
        vals[i] = v
    return np.repeat(vals, np.diff(np.concatenate([st, [S]])))


def message_of(ws: int, mapping, streams) -> np.ndarray:
    """The message whose stream s is streams[s] (len = words * positions mapped to s)."""
    pos = [[p for p in range(ws) if mapping[p] == s] for s in (0, 1)]
    wc = len(streams[0]) // len(pos[0]) if pos[0] else len(streams[1]) // len(pos[1])
    msg = np.zeros((wc, ws), np.uint8)
    for s in (0, 1):
        if pos[s]:
            msg[:, pos[s]] = np.asarray(streams[s], np.uint8).reshape(wc, len(pos[s]))
    return msg.reshape(-1)


def edges_of(n, ws, mapping, s, tile):
    """The tile boundaries' stream positions."""
    return [stream_pos(jb, ws, mapping, s) for jb in range(tile, n, tile)]


def start_sets(kind: str, S: int, edges):
    """Run starts of one stream for a structure `kind`."""
    out = []
    if kind == "edges":  # runs ending at, starting at, and 255-caps landing on each boundary and beside it
        for e in edges:
            for d in (-1, 0, 1):
                out += [e + d, e + d - 255, e + d - 510, e + d + 255, e + d + 510]
    elif kind == "span1":  # a run over one whole tile: no start between the first two boundaries
        out += [7, edges[0] - 5, edges[1] + 5, edges[1] + 6, S - 3]
    elif kind == "span3":  # a run over three whole tiles
        out += [1, edges[0] - 300, edges[3] + 5, S - 1]
    elif kind == "constant":  # one run, which is also the final run
        pass
    elif kind == "dense":
        out += list(range(1, S, 3))
    else:
        raise ValueError(kind)
    return [q for q in out if 0 < q < S]


def structured(ws, mkind, tiles, extra_words, kinds, tile, seed=1):
    """A message of `tiles` whole tiles (rounded up to compress) plus extra_words words, stream s
    built with structure kinds[s]."""
    mapping = mapping_of(ws, mkind)
    n = round_up(tiles * tile, ws) + extra_words * unit(ws)
    wc = n // ws
    streams = []
    for s in (0, 1):
        S = wc * sum(1 for m in mapping if m == s)
        streams.append(stream_of(S, start_sets(kinds[s], S, edges_of(n, ws, mapping, s, tile)), seed + 17 * s))
    return message_of(ws, mapping, streams)


def crossing_message(ws, mkind, tile, lengths, seed=3):
    """Three tiles and a partial one; across boundary k, in each stream, one run of lengths[k] bytes
    (its first byte well before the boundary, or the very byte before it)."""
    mapping = mapping_of(ws, mkind)
    n = round_up(3 * tile, ws) + 401 * unit(ws)
    wc = n // ws
    streams = []
    for s in (0, 1):
        S = wc * sum(1 for m in mapping if m == s)
        edges = edges_of(n, ws, mapping, s, tile)
        starts = []
        for k, L in enumerate(lengths):
            a = edges[k] - (L // 2 if (k + s) % 2 == 0 else 1)
            starts += [a - 3, a, a + L, a + L + 2]
        streams.append(stream_of(S, starts, seed + 5 * s))
    return message_of(ws, mapping, streams)


def cases_for(ws: int, mkind: str, tile: int):
    """(name, message) of every structure at one width and mapping: two to five tiles, partial last tiles."""
    small = 1 if ws <= 12 else 0  # a last tile of one unit: fewer stream bytes than one lane's 16 at widths 3, 5, 12
    return [
        ("just_above", structured(ws, mkind, 1, -(-64 // unit(ws)), ("edges", "edges"), tile)),
        ("edges2", structured(ws, mkind, 2, max(small, 1), ("edges", "edges"), tile)),
        ("crossing_a", crossing_message(ws, mkind, tile, CROSSING[:3])),
        ("crossing_b", crossing_message(ws, mkind, tile, CROSSING[3:], seed=5)),
        ("span1", structured(ws, mkind, 2, 700, ("span1", "span1"), tile, seed=9)),
        ("span3", structured(ws, mkind, 4, 311, ("span3", "span3"), tile, seed=11)),
        ("constant", structured(ws, mkind, 2, 5, ("constant", "constant"), tile, seed=13)),
        ("const_dense", structured(ws, mkind, 1, 450, ("constant", "dense"), tile, seed=15)),
        ("dense_const", structured(ws, mkind, 1, 450, ("dense", "constant"), tile, seed=19)),
    ]


def rle_pairs(lengths: np.ndarray, values: np.ndarray) -> np.ndarray:
    """(count, value) pairs of runs: 255, ..., 255, remainder each, as bytes."""
    lengths = np.asarray(lengths, np.int64)
    per = (lengths + 254) // 255
    total = int(per.sum())
    counts = np.full(total, 255, np.int64)
    last = np.cumsum(per) - 1
    counts[last] = lengths - 255 * (per - 1)
    out = np.empty(2 * total, np.uint8)
    out[0::2] = counts
    out[1::2] = np.repeat(np.asarray(values, np.uint8), per)
    return out


def tile_model(msg: np.ndarray, ws: int, mapping, tile: int) -> bytes:
    """The blob of `msg` under `mapping`, assembled the way the tile pipeline assembles it: per
    (tile, stream) the run starts of the tile alone (its predecessor byte read from the message), the
    scan of first / last / inner over the tiles, and every tile's pairs written at its pair base."""
    msg = np.asarray(msg, np.uint8)
    n = msg.size
    assert n % ws == 0 and n > 0
    wc = n // ws
    ns = 2 if any(mapping) else 1
    head = np.array([0x54445444, n, ns, ws, ws] + [int(m) for m in mapping], "<u4").tobytes()  # magic "TDTD"
    body = b""
    words = msg.reshape(wc, ws)
    for s in range(ns):
        pos = [p for p in range(ws) if mapping[p] == s]
        if not pos:
            body += np.array([0], "<u4").tobytes()
            continue
        x = words[:, pos].reshape(-1)
        S = x.size
        recs, per_tile = [], []
        for jb in range(0, n, tile):
            je = min(n, jb + tile)
            b, e = stream_pos(jb, ws, mapping, s), stream_pos(je, ws, mapping, s)
            prev = int(msg[pred_pos(jb, ws, mapping, s)]) if b else -1
            seg = x[b:e].astype(np.int64)
            st = b + np.flatnonzero(seg != np.concatenate([[prev], seg[:-1]])) if e > b else np.zeros(0, np.int64)
            first = int(st[0]) + 1 if st.size else 0
            last = int(st[-1]) + 1 if st.size else 0
            inner = int(((np.diff(st) + 254) // 255).sum()) if st.size > 1 else 0
            recs.append((first, last, inner))
            per_tile.append(st)
        # the scan: carried run start + 1 and pair base of every tile
        carry, base, scan = 0, 0, []
        for first, last, inner in recs:
            scan.append((carry, base))
            cross = (first - carry + 254) // 255 if first and carry else 0
            base += cross + inner
            carry = max(carry, last)
        total = base + (S - (carry - 1) + 254) // 255
        out = np.zeros(2 * total, np.uint8)
        for t, st in enumerate(per_tile):
            c, pb = scan[t]
            begins = np.concatenate([[c - 1], st[:-1]])[st > 0]  # every start closes the run of the start before it,
            st = st[st > 0]                                      # the tile's first one the carried run; byte 0 closes nothing
            if st.size:
                pairs = rle_pairs(st - begins, x[st - 1])
                out[2 * pb:2 * pb + pairs.size] = pairs
                pb += pairs.size // 2
            if t == len(per_tile) - 1:
                fin = rle_pairs([S - (carry - 1)], [x[S - 1]])
                out[2 * pb:2 * pb + fin.size] = fin
                assert pb + fin.size // 2 == total
        body += np.array([2 * total], "<u4").tobytes() + out.tobytes()
    return head + body
