"""Decode-only blobs whose pairs sit on, one before and one behind every boundary of the decode
kernels (tests/test_decode_edges.py on the CPU, tests/test_gpu_decode_edges.py on the GPU; digests
pinned in tests/golden/decode_edges.json by tests/golden/make_decode_edges.py).  Deterministic from
SEED, no GPU, no message bytes stored: the blobs are rebuilt on every run.  Conventions, serialize,
parse, takes_fast_path and numpy_decode are those of tests/decode_cases.py.

A case is (name, ws, family, blob, edges).  `edges` lists every deliberate placement as
(stream, kind, d, what, position, pair_index): in stored stream `stream` the counted pair number
`pair_index` starts at stream position `position`, which is `d` behind a multiple of `kind` (for the
pair-index kinds lane8 / block / chunk it is `pair_index` that is `d` behind the multiple); `what`
says what stands in front of it.  check_coverage() verifies every entry against the blob.

The geometry is read from psyne_amd/csrc (geometry()); a line that is not found raises.

Edge kinds, in stream positions of a referenced stream with k byte positions per word and
seg = (16 / ws) * k positions per 16-byte group:
    lane 16 | round 64 seg | window WR 64 seg (WR = 1 up to dsmall_max decoded bytes) | gen 8 windows |
    tile kDecTileGroups seg | onetile TG seg, TG = roundup64(ceil(ngroups / kOneWaves)) | share (orig / ws) k
and in pair indices: lane8 8 | block 512 | chunk kAnyDecPairs (generic widths).
decode_one's generic path has one-round windows (lane, round, share); tdt_decode_any_kernel has
share and the pair-index kinds.

Families: edge (a counted pair at B + d behind a random run, a 255-run, a 1-run or 1 / 8 / 600
count-0 pairs, and `cross`: a 255-run from B - j over B), dense (z count-0 pairs, then pairs of one
count c: pair index = position / c + z), cap (255-runs only, three phases), zeros (blocks of count-0
pairs at the start, in front of a tile edge, behind the data, alone, and one per other block), ends
(stream lengths around every boundary, empty / one-pair / straddling / surplus streams, pair counts
around the block size, odd trailing bytes), tails (message sizes around groups, rounds and tiles).

Not covered: decode_fast's rebase of the held pair starts (PSY_DEC_REBASE_LOG2, every 2^28 positions
inside one call) needs a blob that decodes to 256 MiB on the one-wave path.
"""
from __future__ import annotations

import pathlib
import re
from collections import namedtuple

import numpy as np

from tests.decode_cases import numpy_decode, parse, serialize, takes_fast_path  # noqa: F401

SEED = 0xED6E5
CSRC = pathlib.Path(__file__).resolve().parents[1] / "psyne_amd" / "csrc"
FAMILIES = ("edge", "dense", "cap", "zeros", "ends", "tails")
SIZES = (1024, 8192, 8208, 24592, 49168, 65552, 98416)
BIG = 140000
MAX_CASES, MAX_BYTES = 2000, 100 * 1000 * 1000
DS = (-1, 0, 1)
MODES = ("rand", "r255", "r1", "z1", "z8", "z600", "cross1", "cross128", "cross254")
GAP = 520  # positions between two placements of one stream: a 255-run in front and one across

Case = namedtuple("Case", "name ws family blob edges")
Shape = namedtuple("Shape", "name ws mapping ns path")  # path: fast | one | any

SHAPES = (
    Shape("w1", 1, (0,), 1, "fast"),
    Shape("w2_01", 2, (0, 1), 2, "fast"),
    Shape("w2_00", 2, (0, 0), 1, "fast"),
    Shape("w4_1110", 4, (1, 1, 1, 0), 2, "fast"),
    Shape("w4_0111", 4, (0, 1, 1, 1), 2, "fast"),
    Shape("w4_0101", 4, (0, 1, 0, 1), 2, "fast"),
    Shape("w4_0000", 4, (0, 0, 0, 0), 1, "fast"),
    Shape("w4_1111", 4, (1, 1, 1, 1), 2, "fast"),  # stream 0 stored and empty
    Shape("w8_62", 8, (1,) * 6 + (0,) * 2, 2, "fast"),
    Shape("w8_44", 8, (0,) * 4 + (1,) * 4, 2, "fast"),
    Shape("w16_4c", 16, (0,) * 4 + (1,) * 12, 2, "fast"),
    Shape("w16_0", 16, (0,) * 16, 1, "fast"),
    Shape("w4_0120", 4, (0, 1, 2, 0), 3, "one"),
    Shape("w4_0123", 4, (0, 1, 2, 3), 4, "one"),
    Shape("w8_35", 8, (0,) * 3 + (1,) * 5, 2, "one"),
    Shape("w16_r16", 16, tuple(range(16)), 16, "one"),
    Shape("w2_17", 2, (0, 1), 17, "one"),
    Shape("w3", 3, (0, 1, 1), 2, "any"),
    Shape("w5", 5, (0,) * 5, 1, "any"),
    Shape("w12", 12, (0, 1) * 6, 2, "any"),
    Shape("w40", 40, (0,) * 39 + (1,), 2, "any"),
    Shape("w64", 64, tuple(i % 3 for i in range(64)), 3, "any"),
)
SHAPE16 = "w16_r16"
POS_KINDS = {"fast": ("lane", "round", "window", "gen", "tile", "onetile", "share"),
             "one": ("lane", "round", "share"), "any": ("share",)}
KIND_RANK = ("note", "lane", "lane8", "round", "window", "onetile", "gen", "tile", "block", "chunk", "share")
PAIR_KINDS = {"fast": ("lane8", "block"), "one": ("lane8", "block"), "any": ("lane8", "block", "chunk")}


# --------------------------------------------------------------------------- geometry from the source
_GEO = {}


def _source_int(fname, pattern):
    m = re.search(pattern, (CSRC / fname).read_text(), re.M)
    if not m:
        raise RuntimeError("no line matching %r in %s" % (pattern, CSRC / fname))
    v = 1
    for f in m.group(1).split("*"):
        v *= int(f.strip())
    return v


def geometry() -> dict:
    """The decode kernels' sizes as their source states them."""
    if not _GEO:
        num = r"([0-9][0-9 *]*)"
        _GEO.update(
            tile_groups=_source_int("tdt_decode.h", r"^constexpr\s+uint32_t\s+kDecTileGroups\s*=\s*" + num + ";"),
            wr=_source_int("tdt_decode.h", r"^#define\s+PSY_DEC_WR\s+" + num + r"\s*$"),
            one_waves=_source_int("tdt_decode.h", r"^constexpr\s+int\s+kOneWaves\s*=\s*" + num + ";"),
            blobc=_source_int("tdt_decode.h", r"^#define\s+PSY_DEC_BLOBC\s+" + num + r"\s*$"),
            any_pairs=_source_int("tdt_anyws.h", r"^constexpr\s+uint32_t\s+kAnyDecPairs\s*=\s*" + num + ";"),
            dsmall_max=_source_int("tdt_api.hip", r"^\s*uint64_t\s+dsmall_max\s*=\s*" + num + ";"),
            dbig_min=_source_int("tdt_api.hip", r"^\s*uint64_t\s+dbig_min\s*=\s*" + num + ";"),
            one_max=_source_int("tdt_api.hip", r"^constexpr\s+uint64_t\s+kOneMax\s*=\s*" + num + ";"),
        )
        g = _GEO
        if not (g["tile_groups"] % 64 == 0 and 1 <= g["wr"] <= 8 and g["dsmall_max"] < g["dbig_min"] <= g["one_max"]):
            raise RuntimeError("implausible decode geometry %r" % g)
    return _GEO


def referenced(ws, mapping):
    """[(stored stream id, k)] in the order of first use (the kernels' r = 0, 1, ...)."""
    ids = []
    for s in mapping[:ws]:
        if s not in ids:
            ids.append(s)
    return [(s, list(mapping[:ws]).count(s)) for s in ids]


def stream_kinds(path, ws, k, orig) -> dict:
    """kind → size in stream positions (pair-index kinds in pairs) for a stream with k byte positions
    per word in a message of orig bytes on `path`."""
    g = geometry()
    wc = orig // ws
    out = {"share": wc * k, "lane8": 8, "block": 512}
    if path == "any":
        out["chunk"] = g["any_pairs"]
        return out
    seg = (16 // ws) * k
    out.update(lane=16, round=64 * seg)
    if path == "fast":
        wr = 1 if orig <= g["dsmall_max"] else g["wr"]
        ngroups = (wc * ws + 15) // 16
        tg = ((ngroups + g["one_waves"] - 1) // g["one_waves"] + 63) // 64 * 64
        out.update(window=wr * 64 * seg, gen=8 * wr * 64 * seg, tile=g["tile_groups"] * seg, onetile=tg * seg)
    return out


# --------------------------------------------------------------------------- building one stream
class Stream:
    """Pairs of one stored stream, appended in numpy chunks; `pos` is the decoded length so far."""

    def __init__(self, rng, sid):
        self.rng, self.sid = rng, sid
        self.cc, self.vv = [], []
        self.pos = self.npairs = 0
        self.last = int(rng.integers(0, 256))
        self.zvals = ()
        self.edges = []
        self.odd = False

    def _append(self, counts):
        """Counted pairs; every value differs from the value before it (and from the count-0 pairs
        just written)."""
        counts = np.asarray(counts, np.int64)
        if counts.size == 0:
            return
        delta = self.rng.integers(1, 256, counts.size)
        first = (self.last + int(delta[0])) % 256
        while first == self.last or first in self.zvals:
            first = (first + 1) % 256
        delta[0] = (first - self.last) % 256
        vals = (self.last + np.cumsum(delta)) % 256
        self.cc.append(counts)
        self.vv.append(vals)
        self.pos += int(counts.sum())
        self.npairs += counts.size
        self.last, self.zvals = int(vals[-1]), ()

    def run(self, count):
        assert 1 <= count <= 255
        self._append([count])

    def zeros(self, z):
        """z count-0 pairs whose values differ from the counted pairs on both sides."""
        if z == 0:
            return
        a = (self.last + 1 + int(self.rng.integers(0, 100))) % 256
        b = (self.last + 120 + int(self.rng.integers(0, 100))) % 256
        self.cc.append(np.zeros(z, np.int64))
        self.vv.append(np.where(np.arange(z) % 2 == 0, a, b))
        self.npairs += z
        self.zvals = (a, b)

    def const(self, c, total):
        """Pairs of count c up to `total` more positions (the last one shorter)."""
        n, rem = divmod(total, c)
        self._append([c] * n + ([rem] if rem else []))

    def fill_to(self, target, maxrun=8):
        """Random runs of 1..maxrun up to position `target` exactly."""
        need = target - self.pos
        assert need >= 0, (target, self.pos)
        while need > 0:
            c = self.rng.integers(1, maxrun + 1, max(16, 3 * need // (maxrun + 1) + 16))
            cs = np.cumsum(c)
            if cs[-1] >= need:
                i = int(np.searchsorted(cs, need))
                c = c[: i + 1]
                c[i] -= cs[i] - need
            self._append(c)
            need = target - self.pos

    def fill_pairs(self, target, maxrun=3):
        """Random runs up to pair index `target` exactly."""
        assert target >= self.npairs
        self._append(self.rng.integers(1, maxrun + 1, target - self.npairs))

    def fill_both(self, target, residue, mod=512):
        """Up to position `target` with a pair count of `residue` modulo `mod`."""
        assert target - self.pos >= 1400
        self.fill_to(target - 1300)
        need = target - self.pos
        n = (residue - self.npairs) % mod
        while n * 255 < need:
            n += mod
        assert 0 < n <= need
        c = np.full(n, need // n, np.int64)
        c[: need % n] += 1
        self._append(self.rng.permutation(c))
        assert self.pos == target and self.npairs % mod == residue

    def mark(self, kinds, d, what):
        """Record the counted pair about to be appended (no boundary kind: as a `note`)."""
        for kind in kinds or ["note"]:
            self.edges.append((self.sid, kind, d, what, self.pos, self.npairs))

    def bytes(self):
        c = np.concatenate(self.cc) if self.cc else np.zeros(0, np.int64)
        v = np.concatenate(self.vv) if self.vv else np.zeros(0, np.int64)
        s = np.empty(2 * c.size + (1 if self.odd else 0), np.uint8)
        s[0:2 * c.size:2] = c
        s[1:2 * c.size:2] = v
        if self.odd:
            s[-1] = 0xEE
        return s.tobytes()


def kinds_at(kinds, names, b):
    return [n for n in names if n in kinds and kinds[n] > 0 and b > 0 and b % kinds[n] == 0]


def candidates(kinds, names, limit, thin):
    """Boundaries of every kind up to `limit`, the rarest kinds first; lane and round thinned."""
    out = []
    for n in sorted((n for n in names if n in kinds and kinds[n] > 0), key=lambda n: -kinds[n]):
        if n == "share":
            mult = [kinds[n]]
        else:
            mult = list(range(kinds[n], limit + 1, kinds[n]))
            if n in ("lane", "lane8"):
                mult = mult[thin % 37::37]
            elif n == "round" and len(mult) > 24:
                step = len(mult) // 24 + 1
                mult = mult[thin % step::step]
        out += [b for b in mult if b <= limit]
    return out


def choose(cands, gap):
    got = []
    for b in cands:
        if all(abs(b - a) >= gap for a in got):
            got.append(b)
    return sorted(got)


def edge_stream(rng, sid, kinds, names, d, rot, maxrun):
    """Position space: for every chosen boundary B a counted pair at B + d, or a 255-run over B."""
    st = Stream(rng, sid)
    S = kinds["share"]
    for i, b in enumerate(choose(candidates(kinds, names, S, rot), GAP)):
        mode = MODES[(rot + i) % len(MODES)]
        here = kinds_at(kinds, names, b)
        x = b + d
        if mode.startswith("cross"):
            j = int(mode[5:])
            if b - j < st.pos:
                mode = "z1"
            else:
                st.fill_to(b - j, maxrun)
                st.mark(here, -j, mode)
                st.run(255)
                continue
        if x < st.pos:
            continue
        if mode == "r255" and x - 255 >= st.pos:
            st.fill_to(x - 255, maxrun)
            st.run(255)
        elif mode == "r1" and x - 1 >= st.pos:
            st.fill_to(x - 1, maxrun)
            st.run(1)
        else:
            st.fill_to(x, maxrun)
            if mode[0] == "z":
                st.zeros(int(mode[1:]))
            elif mode != "rand":
                mode = "rand"
        st.mark(here, d, mode)
        st.run(int(rng.integers(1, 4)))
    if st.pos < S:
        st.fill_to(S, maxrun)
    return st


def pair_edge_stream(rng, sid, kinds, names, d, rot):
    """Pair-index space: the pair with index I + d is a counted pair behind a 255-run, a 1-run or
    count-0 pairs."""
    st = Stream(rng, sid)
    S = kinds["share"]
    for i, b in enumerate(choose(candidates(kinds, names, S // 2, rot), 8)):
        mode = MODES[(rot + i) % 6]
        x = b + d
        if st.pos >= S - 300:
            break
        room = x - st.npairs
        if room < 0:
            continue
        if mode in ("r255", "r1") and room >= 1:
            st.fill_pairs(x - 1)
            st.run(255 if mode == "r255" else 1)
        elif mode[0] == "z" and room >= int(mode[1:]):
            st.fill_pairs(x - int(mode[1:]))
            st.zeros(int(mode[1:]))
        else:
            mode = "rand"
            st.fill_pairs(x)
        st.mark(kinds_at(kinds, names, b), d, mode)
        st.run(int(rng.integers(1, 4)))
    if st.pos < S:
        st.fill_to(S, 3)
    return st


# --------------------------------------------------------------------------- assembling a blob
def orig_for(size, ws):
    return (size + ws - 1) // ws * ws


def assemble(rng, shape, orig, make):
    """make(sid, r, kinds) → Stream for every referenced stream; the other stored streams hold a few
    pairs that nothing may read (w4_1111's stream 0: empty)."""
    ref = referenced(shape.ws, shape.mapping)
    built, edges = {}, []
    for r, (sid, k) in enumerate(ref):
        st = make(sid, r, stream_kinds(shape.path, shape.ws, k, orig))
        built[sid] = st.bytes()
        edges += st.edges
    streams = []
    for s in range(shape.ns):
        if s in built:
            streams.append(built[s])
        elif shape.name == "w4_1111":
            streams.append(b"")
        else:
            junk = Stream(rng, s)
            junk.fill_to(int(rng.integers(0, 40)), 7)
            junk.odd = bool(s & 1)
            streams.append(junk.bytes())
    return serialize(orig, shape.ws, list(shape.mapping), streams), tuple(edges)


def names_for(shape):
    return POS_KINDS[shape.path]


def _edge_cases(rng, shape, out):
    fast = shape.path == "fast"
    # (not every size with every d: the case count is capped; every (kind, d) stays, check_coverage)
    if fast:
        grid = [(s, d) for s in (1024, 8208, 24592, 65552, 98416) for d in DS] + [(8192, 0)] + [(49168, d) for d in DS]
    else:
        grid = [(1024, 0)] + [(s, d) for s in (8208, 65552) for d in DS]
    n = 0
    for size, d in grid:
        if True:
            orig = orig_for(size, shape.ws)
            rot, maxrun = n, (8, 3, 40, 255)[n % 4]
            blob, edges = assemble(rng, shape, orig, lambda sid, r, kinds: edge_stream(
                rng, sid, kinds, names_for(shape), d, rot + r, maxrun))
            out.append(Case("%s_edge_%d_d%+d" % (shape.name, size, d), shape.ws, "edge", blob, edges))
            n += 1
    for size in (65552,):
        for d in DS:
            orig = orig_for(size, shape.ws)
            rot = n
            blob, edges = assemble(rng, shape, orig, lambda sid, r, kinds: pair_edge_stream(
                rng, sid, kinds, PAIR_KINDS[shape.path], d, rot + r))
            out.append(Case("%s_edge_pairs_%d_d%+d" % (shape.name, size, d), shape.ws, "edge", blob, edges))
            n += 1


DENSE_Z = (0, 512, 1, 511, 7, 8, 9, 513)
DENSE_Z_ANY = (2047, 2048, 2049)


def dense_stream(rng, sid, kinds, z, c):
    st = Stream(rng, sid)
    st.zeros(z)
    st.mark(["block"] if z % 512 == 0 and z else [], 0, "dense z=%d c=%d" % (z, c))
    st.const(c, kinds["share"])
    return st


def _dense_cases(rng, shape, out):
    cycle = (8192, 24592, 1024, 49168, 8208, 65552, 98416)
    zs = DENSE_Z + (DENSE_Z_ANY if shape.path == "any" else ())
    for iz, z in enumerate(zs):
        for c in (1, 2, 3):
            size = cycle[(iz + 3 * c) % len(cycle)]
            if c <= 2 and z in (0, 512):  # a block ends where a tile begins: sizes with tiles
                size = 65552 if z == 0 else 98416
            orig = orig_for(size, shape.ws)
            blob, edges = assemble(rng, shape, orig, lambda sid, r, kinds: dense_stream(rng, sid, kinds, z, c))
            out.append(Case("%s_dense_%d_z%d_c%d" % (shape.name, size, z, c), shape.ws, "dense", blob, edges))


def cap_stream(rng, sid, kinds, o):
    st = Stream(rng, sid)
    S = kinds["share"]
    if S:
        st.mark([], 0, "cap o=%d" % o)
        st.run(min(o, S))
        st.const(255, S - st.pos)
    return st


def _cap_cases(rng, shape, out):
    for size in (8192, 24592):
        for o in (255, 1, 254):
            orig = orig_for(size, shape.ws)
            blob, edges = assemble(rng, shape, orig, lambda sid, r, kinds: cap_stream(rng, sid, kinds, o))
            out.append(Case("%s_cap_%d_o%d" % (shape.name, size, o), shape.ws, "cap", blob, edges))


def _zeros_cases(rng, shape, out):
    fast = shape.path == "fast"
    size = 65552 if fast else 24592
    orig = orig_for(size, shape.ws)

    def add(tag, make):
        blob, edges = assemble(rng, shape, orig, make)
        out.append(Case("%s_zeros_%d_%s" % (shape.name, size, tag), shape.ws, "zeros", blob, edges))

    def at_start(m, shift):
        def make(sid, r, kinds):
            st = Stream(rng, sid)
            if shift:
                st.run(2)
            st.zeros(512 * m)
            st.mark(["block"] if not shift else [], 0, "behind %d count-0 pairs" % (512 * m))
            st.fill_to(kinds["share"], 8)
            return st
        return make

    def before(kind, m, shift):
        def make(sid, r, kinds):
            st = Stream(rng, sid)
            S, size_k = kinds["share"], kinds[kind]
            b = size_k * max(1, (S // size_k) // 2)  # a boundary in the middle of the stream
            if b >= S or b < 1400:
                st.fill_to(S, 8)
                return st
            st.fill_both(b, 1 if shift else 0)
            st.zeros(512 * m)
            st.mark(kinds_at(kinds, names_for(shape), b) + (["block"] if not shift else []), 0,
                    "behind %d count-0 pairs%s" % (512 * m, " + 1 pair" if shift else ""))
            st.fill_to(S, 8)
            return st
        return make

    def behind(m):
        def make(sid, r, kinds):
            st = Stream(rng, sid)
            st.fill_to(kinds["share"], 8)
            st.zeros(512 * m)
            return st
        return make

    def only(sid, r, kinds):
        st = Stream(rng, sid)
        st.zeros(700)
        return st

    def alternate(slot):
        def make(sid, r, kinds):
            st = Stream(rng, sid)
            S, b = kinds["share"], 0
            while st.pos + 4 * 512 < S:
                if b % 2:
                    st.fill_pairs(512 * b + slot, 3)
                    st.zeros(1)
                    st.mark(["block"] if slot == 0 else [], 1 if slot == 0 else 0, "behind the count-0 pair at slot %d of block %d" % (slot, b))
                st.fill_pairs(512 * (b + 1), 3)
                b += 1
            st.fill_to(S, 3)
            return st
        return make

    for m in (1, 2):
        for shift in (0, 1):
            add("start_m%d_s%d" % (m, shift), at_start(m, shift))
    if fast:
        for m, shift in ((1, 0), (2, 1), (1, 1), (2, 0)):
            add("tile_m%d_s%d" % (m, shift), before("tile", m, shift))
        for m, shift in ((1, 0), (2, 1)):
            add("onetile_m%d_s%d" % (m, shift), before("onetile", m, shift))
    for m in (1, 2):
        add("behind_m%d" % m, behind(m))
    add("only", only)
    for slot in (0, 7, 8, 511):
        add("alt_slot%d" % slot, alternate(slot))


def _ends_cases(rng, shape, out):
    fast = shape.path == "fast"
    size = 65552 if fast else 24592
    orig = orig_for(size, shape.ws)
    n = [0]

    def add(tag, make):
        blob, edges = assemble(rng, shape, orig, make)
        out.append(Case("%s_ends_%d_%s" % (shape.name, size, tag), shape.ws, "ends", blob, edges))
        n[0] += 1

    def length(kind, d, which):
        def make(sid, r, kinds):
            st = Stream(rng, sid)
            S, size_k = kinds["share"], kinds[kind]
            mult = max(1, S // size_k)
            b = S if kind == "share" else size_k * (1, max(1, mult // 2), mult)[which]
            st.fill_to(max(b + d - 1, 0), (8, 255, 3)[which])
            if b + d > st.pos:  # the last pair, ending at B + d
                st.mark([kind], d, "stream ends here")
                st.run(1)
            return st
        return make

    for kind in (k for k in ("round", "window", "tile", "onetile", "share") if k in POS_KINDS[shape.path]):
        for d in DS:
            add("%s_d%+d" % (kind, d), length(kind, d, n[0] % 3))

    def simple(f):
        def make(sid, r, kinds):
            st = Stream(rng, sid)
            f(st, kinds["share"])
            return st
        return make

    def straddle(st, S):
        st.fill_to(S - 1, 8)
        st.mark(["share"], -1, "a 255-run over the share's end")
        st.run(255)

    def surplus(st, S):
        st.fill_to(S, 8)
        st.fill_pairs(st.npairs + 700, 3)

    def npmod(res):
        def f(st, S):
            st.fill_to(S, 8)
            st.fill_pairs(st.npairs + (res - st.npairs) % 512, 3)
            assert st.npairs % 512 == res
        return f

    def odd(parity):
        def f(st, S):
            st.fill_to(S, 8)
            if st.npairs % 2 != parity:
                st.run(1)
            st.odd = True
        return f

    add("empty", simple(lambda st, S: None))
    add("one_pair", simple(lambda st, S: st.run(200)))
    add("straddle", simple(straddle))
    add("surplus", simple(surplus))
    for res in (0, 1, 8, 511):
        add("np%d" % res, simple(npmod(res)))
    for parity in (0, 1):
        add("odd_behind_%s" % ("even", "odd")[parity], simple(odd(parity)))


def _tails_cases(rng, shape, out):
    ws, tg = shape.ws, geometry()["tile_groups"]

    def words_with(test, lo):
        for wc in range((lo + ws - 1) // ws, (lo + ws - 1) // ws + 4096):
            if test((wc * ws + 15) // 16, wc * ws):
                return wc
        return None

    wanted = [("g0", lambda g, w: g % 64 == 0 and w % 16 == 0, 5000), ("g1", lambda g, w: g % 64 == 1, 5000),
              ("g63", lambda g, w: g % 64 == 63, 5000), ("w16", lambda g, w: w % 16 != 0, 9000),
              ("tile1g", lambda g, w: g == tg + 1, 16 * tg), ("tile2", lambda g, w: g == 2 * tg, 32 * tg - 64)]
    for i, (tag, test, lo) in enumerate(wanted):
        wc = words_with(test, lo)
        if wc is None:
            continue  # (no such word count at this width: check_coverage says which tags a path needs)
        for rest in ((0, ws - 1) if ws > 1 and i == 0 else (0,)):
            orig = wc * ws + rest
            blob, edges = assemble(rng, shape, orig, lambda sid, r, kinds: edge_stream(
                rng, sid, kinds, names_for(shape), (0, -1, 1)[i % 3], i + r, 8))
            out.append(Case("%s_tails_%d_%s" % (shape.name, orig, tag), ws, "tails", blob, edges))


def _big_cases(rng, out):
    fast = [s for s in SHAPES if s.path == "fast"]
    for i, shape in enumerate(fast[::2]):
        orig = orig_for(BIG, shape.ws)
        blob, edges = assemble(rng, shape, orig, lambda sid, r, kinds: edge_stream(
            rng, sid, kinds, names_for(shape), DS[i % 3], i + r, (8, 255)[i % 2]))
        out.append(Case("%s_edge_%d_d%+d" % (shape.name, BIG, DS[i % 3]), shape.ws, "edge", blob, edges))
    for shape in (fast[0], fast[3], fast[10]):
        orig = orig_for(BIG, shape.ws)
        blob, edges = assemble(rng, shape, orig, lambda sid, r, kinds: dense_stream(rng, sid, kinds, 0, 1))
        out.append(Case("%s_dense_%d_z0_c1" % (shape.name, BIG), shape.ws, "dense", blob, edges))


_CACHE = {}


def all_cases():
    """Every case, in a fixed order (built once per process)."""
    if "cases" not in _CACHE:
        rng = np.random.default_rng(SEED)
        cases = []
        for shape in SHAPES:
            assert takes_fast_path(shape.ws, list(shape.mapping), shape.ns) == (shape.path == "fast"), shape.name
            for fam in (_edge_cases, _dense_cases, _cap_cases, _zeros_cases, _ends_cases, _tails_cases):
                fam(rng, shape, cases)
        _big_cases(rng, cases)
        assert len({c.name for c in cases}) == len(cases)
        check_coverage(cases)
        _CACHE["cases"] = cases
    return _CACHE["cases"]


def shape_of(case) -> Shape:
    return next(s for s in SHAPES if case.name.startswith(s.name + "_"))


# --------------------------------------------------------------------------- reading a blob's streams
View = namedtuple("View", "sid r k kinds counts starts soff")


def views(case):
    """Per referenced stream of the case's blob: its geometry, the pairs' counts, their start
    positions and the stream's offset in the blob."""
    orig, ns, ws, msize, mapping, streams = parse(case.blob)
    shape = shape_of(case)
    offs, off = [], 20 + 4 * msize
    for s in streams:
        offs.append(off + 4)
        off += 4 + len(s)
    out = []
    for r, (sid, k) in enumerate(referenced(ws, mapping)):
        raw = np.frombuffer(streams[sid], np.uint8)
        counts = raw[0:raw.size // 2 * 2:2].astype(np.int64)
        starts = np.cumsum(counts) - counts
        out.append(View(sid, r, k, stream_kinds(shape.path, ws, k, orig), counts, starts, offs[sid]))
    return out


def locate(case, at) -> str:
    """Where output byte `at` lies — its stream and stream position — and the case's nearest edge."""
    orig, _, ws, _, mapping, _ = parse(case.blob)
    if at >= orig // ws * ws:
        return "behind the last whole word"
    b = at % ws
    sid = mapping[b]
    k = list(mapping).count(sid)
    pos = (at // ws) * k + sum(1 for x in mapping[:b] if x == sid)
    near = [e for e in case.edges if e[0] == sid]
    if not near:
        return "stream %d position %d" % (sid, pos)
    # (one placement is listed under every kind its boundary is a multiple of: name the rarest)
    _, kind, d, what, p, pi = min(near, key=lambda e: (abs(e[4] - pos), -KIND_RANK.index(e[1])))
    return "stream %d position %d, nearest edge: %s d=%+d (%s) at %d, pair %d" % (sid, pos, kind, d, what, p, pi)


# --------------------------------------------------------------------------- what the tests rely on
def check_coverage(cases):
    """Every line computed from the blobs; a later edit of the generator cannot quietly lose one."""
    g = geometry()
    assert len(cases) <= MAX_CASES, len(cases)
    total = sum(parse(c.blob)[0] for c in cases)
    assert total <= MAX_BYTES, total
    assert sum(parse(c.blob)[0] > g["dbig_min"] for c in cases) <= 10

    seen = {}       # shape → {(kind, d)}
    fams = {}       # shape → families
    coincide = set()  # (kind, r): pair 512 b starts exactly at a multiple of kind
    zero_front = set()  # kinds with an all-zero block directly in front of such a boundary
    arms = {}       # fast shape → {"cached", "cached_full", "small_uncached", "full", "checked"}
    mixed_blocks = many_blocks = headless16 = zero_chunk = cut_inside = False
    tails = {}      # shape → {what its tails cases' sizes are}
    for c in cases:
        shape = shape_of(c)
        orig = parse(c.blob)[0]
        fams.setdefault(shape.name, set()).add(c.family)
        vs = {v.sid: v for v in views(c)}
        if c.family == "tails":
            whole = orig // c.ws * c.ws
            groups = (whole + 15) // 16
            tails.setdefault(shape.name, set()).update(
                ["g%d" % (groups % 64), "w16" if whole % 16 else "w0", "rest" if orig % c.ws else "norest"] +
                (["tile+1"] if groups == g["tile_groups"] + 1 else []) + (["2tiles"] if groups == 2 * g["tile_groups"] else []))
        for sid, kind, d, what, pos, pi in c.edges:  # every recorded placement is in the blob
            v = vs[sid]
            assert v.counts[pi] > 0 and v.starts[pi] == pos, (c.name, sid, kind, d, pos, pi)
            if kind == "note":
                continue
            size = v.kinds[kind]
            if what.startswith("cross"):
                assert d == -int(what[5:]) and v.counts[pi] == 255 and (pos - d) % size == 0, (c.name, kind, what)
                assert not ((v.starts > pos) & (v.starts < pos + 255) & (v.counts > 0)).any(), (c.name, kind, what)
                seen.setdefault(shape.name, set()).add((kind, "cross"))
            elif what == "stream ends here":
                assert pos + 1 == v.starts[-1] + v.counts[-1] and (pos + 1 - d) % size == 0, (c.name, kind, d)
                seen.setdefault(shape.name, set()).add((kind, "end", d))
            else:
                at = pi if kind in ("lane8", "block", "chunk") else pos
                assert at - d > 0 and (at - d) % size == 0, (c.name, kind, d, at)
                seen.setdefault(shape.name, set()).add((kind, d))
        for v in vs.values():
            nblocks = (v.counts.size + 511) // 512
            S = v.kinds["share"]
            if shape.path == "fast":
                a = arms.setdefault(shape.name, set())
                inside = v.soff + 2 * v.counts.size <= g["blobc"]
                if orig <= g["dsmall_max"] and v.counts.size:
                    a.add("cached" if inside else "small_uncached")
                    if inside and nblocks > 1:
                        a.add("cached_full")
                if orig > g["dsmall_max"] and nblocks > 1:
                    a.add("full")
                if orig > g["dsmall_max"] and v.counts.size:
                    a.add("checked")
                bstart = v.starts[512::512]  # where blocks 1, 2, ... begin
                for kind in ("tile", "onetile"):
                    size = v.kinds[kind]
                    if kind == "tile" and orig < 16384 + 16 * g["tile_groups"]:
                        continue
                    if kind == "onetile" and not (4096 < orig <= g["one_max"]):
                        continue
                    hit = np.flatnonzero((bstart % size == 0) & (bstart > 0) & (bstart < S) & (v.counts[512::512] > 0))
                    if hit.size:
                        coincide.add((kind, v.r))
                    for b in hit:  # block b (0-based, in front of block b + 1) sums to 0
                        if v.counts[512 * b:512 * (b + 1)].sum() == 0 and v.starts[512 * b] > 0:
                            zero_front.add(kind)
                if bstart.size and np.bincount(bstart[bstart < S] // v.kinds["window"]).max(initial=0) >= 4:
                    many_blocks = True
            full = [v.counts[512 * b:512 * (b + 1)] for b in range(nblocks - 1)]
            if shape.path == "fast" and any((f > 0).all() for f in full) and any((f == 0).any() for f in full):
                mixed_blocks = True
            if shape.name == SHAPE16 and S >= 4 * v.kinds["round"]:
                rounds = np.zeros(S // v.kinds["round"], bool)
                live = v.starts[(v.counts > 0) & (v.starts < rounds.size * v.kinds["round"])]
                rounds[live // v.kinds["round"]] = True
                run = best = 0
                for x in rounds:
                    run = 0 if x else run + 1
                    best = max(best, run)
                headless16 |= best >= 3
            if shape.path == "any":
                ch = v.kinds["chunk"]
                zero_chunk |= any(v.counts[i:i + ch].sum() == 0 and v.starts[i] < S
                                  for i in range(0, v.counts.size - ch + 1, ch))
                inside = (v.starts < S) & (v.starts + v.counts > S)
                cut_inside |= bool(inside.any())

    for shape in SHAPES:
        assert fams[shape.name] == set(FAMILIES), (shape.name, fams[shape.name])
        for kind in POS_KINDS[shape.path] + PAIR_KINDS[shape.path]:
            for d in DS:
                assert (kind, d) in seen[shape.name], (shape.name, kind, d)
        for kind in POS_KINDS[shape.path]:
            assert (kind, "cross") in seen[shape.name], (shape.name, kind)
        for kind in (k for k in ("round", "window", "tile", "onetile", "share") if k in POS_KINDS[shape.path]):
            for d in DS:
                assert (kind, "end", d) in seen[shape.name], (shape.name, kind, d)
        need = {"g0", "g1", "g63", "w0", "norest"} | ({"rest"} if shape.ws > 1 else set()) | (
            {"w16"} if shape.ws % 16 else set()) | ({"tile+1", "2tiles"} if shape.path != "any" else set())
        if shape.ws % 64 == 0:  # whole words of 64 bytes: the group count is a multiple of 4
            need -= {"g1", "g63"}
        assert tails[shape.name] >= need, (shape.name, need - tails[shape.name])
        if shape.path == "fast":
            assert arms[shape.name] >= {"cached", "small_uncached", "full", "checked"}, (shape.name, arms[shape.name])
    assert any("cached_full" in a for a in arms.values())
    assert coincide >= {("tile", 0), ("tile", 1), ("onetile", 0), ("onetile", 1)}, coincide
    assert zero_front >= {"tile", "onetile"}, zero_front
    assert mixed_blocks and many_blocks and headless16 and zero_chunk and cut_inside, (
        mixed_blocks, many_blocks, headless16, zero_chunk, cut_inside)
