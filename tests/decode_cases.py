"""Crafted decode-only blobs for the differential decode tests (tests/test_decode_fuzz.py on the
CPU, tests/test_gpu_decode_fuzz.py on the GPU; digests pinned in tests/golden/decode_fuzz.json by
tests/golden/make_decode_fuzz.py).  Deterministic from SEED, no GPU, no fixture file: the blobs
are rebuilt on every run and checked against the pinned digests.

A case is (name, ws, family, blob bytes).  The valid families hold what the TDT format allows and
this project's encoder never writes — any number of streams (unused ones too), mappings of any
shape, mapping_size > word_size, streams shorter or longer than their share of the words, count-0
pairs, an odd trailing byte, an original_size that is no multiple of word_size — at the decoded
sizes where the decode kernels change path:

    1,024 / 1,040   one 1 KiB window of decode_one's generic path, and one window plus a group
    5,000           a tail past the last whole word at most widths
    8,192 / 8,208   the two sides of dsmall_max (one-round windows with the blob cache / main list)
    20,000, 65,536, 70,001   many windows; one, two and three 32 KiB tiles once TDT_OPT_LARGE_MIN
                    sends them to the large-blob passes
    140,000         above dbig_min (the list dispatched first); a handful of cases only

The family "malformed" derives, per width, cut and patched copies of one valid 5,000-byte blob;
their expected statuses are the oracle's (the reference itself has no bounds checks there).
"""
from __future__ import annotations

import struct
from collections import namedtuple

import numpy as np

SEED = 0xDEC0DE5
MAGIC_TDT = 0x54445444
TUNED = (1, 2, 4, 8, 16)
GENERIC = (3, 5, 12, 24, 40, 64)
WIDTHS = TUNED + GENERIC
SIZES = (1024, 1040, 5000, 8192, 8208, 20000, 65536, 70001)
BIG = 140000
FAMILIES = ("exact", "short", "long", "zero_odd", "half_odd", "alt_empty")
MAXRUNS = (1, 2, 3, 8, 255)

Case = namedtuple("Case", "name ws family blob")


# --------------------------------------------------------------------------- blob construction
def serialize(orig, ws, mapping, streams, msize=None):
    """TDTEncodedData::serialize's layout: magic, original_size, num_streams, word_size,
    mapping_size, the mapping (int32), then per stream a length word and its bytes."""
    msize = len(mapping) if msize is None else msize
    out = [struct.pack("<5I", MAGIC_TDT, orig, len(streams), ws & 0xFFFFFFFF, msize),
           struct.pack("<%di" % len(mapping), *mapping)]
    for s in streams:
        out.append(struct.pack("<I", len(s)))
        out.append(bytes(s))
    return b"".join(out)


def pairs(rng, total, maxrun=255, zero_frac=0.0, odd=False) -> bytes:
    """(count, value) pairs whose counts sum to `total` (the vectorised form of _pairs in
    tests/test_gpu_parity.py): counts uniform in 1..maxrun, a fraction zero_frac of count-0 pairs
    in between, `odd`: one trailing byte that no decoder may read as a pair."""
    chunks, have = [], 0
    while have < total:
        n = max(64, int(2.5 * (total - have) / (maxrun + 1) / (1.0 - zero_frac)) + 64)
        c = rng.integers(1, maxrun + 1, n)
        if zero_frac:
            c[rng.random(n) < zero_frac] = 0
        cs = np.cumsum(c) + have
        if cs[-1] >= total:
            i = int(np.searchsorted(cs, total))  # the first pair that reaches `total`
            c = c[: i + 1]
            c[i] -= cs[i] - total
            have = total
        else:
            have = int(cs[-1])
        chunks.append(c)
    counts = np.concatenate(chunks) if chunks else np.zeros(0, np.int64)
    assert int(counts.sum()) == total
    s = np.empty(2 * counts.size + (1 if odd else 0), np.uint8)
    s[0:2 * counts.size:2] = counts
    s[1:2 * counts.size:2] = rng.integers(0, 256, counts.size)
    if odd:
        s[-1] = rng.integers(1, 256)
    return s.tobytes()


def make_mapping(rng, ws, nref, unused):
    """ws positions onto nref referenced streams (every one used, in a shuffled position order),
    the referenced ids scattered among nref + unused stream ids."""
    ns = nref + unused
    ids = [int(x) for x in rng.permutation(ns)[:nref]]
    pos = [r % nref for r in range(ws)]
    if ws > nref:  # uneven shares: every stream once, the rest at random
        pos = list(range(nref)) + [int(x) for x in rng.integers(0, nref, ws - nref)]
    pos = [pos[int(i)] for i in rng.permutation(ws)]
    return [ids[p] for p in pos], ns


def fill_streams(rng, family, mapping, ns, wc, maxrun):
    """Stream bytes of every stored stream: the referenced ones by `family`, the unused ones a few
    pairs that nothing may read as data."""
    streams = []
    for s in range(ns):
        need = wc * mapping.count(s)
        if need == 0:
            streams.append(pairs(rng, int(rng.integers(0, 40)), maxrun=7, odd=bool(s & 1)))
        elif family == "exact":
            streams.append(pairs(rng, need, maxrun))
        elif family == "short":  # leaves zeros
            streams.append(pairs(rng, int(need * rng.random()), maxrun))
        elif family == "long":  # the excess is ignored
            streams.append(pairs(rng, need + int(rng.integers(1, 3001)), maxrun))
        elif family == "zero_odd":
            streams.append(pairs(rng, need, maxrun, zero_frac=0.2, odd=True))
        elif family == "half_odd":
            streams.append(pairs(rng, need // 2, maxrun, odd=True))
        elif family == "alt_empty":  # every other stream empty
            streams.append(b"" if s % 2 == 0 else pairs(rng, need, maxrun))
        else:
            raise ValueError(family)
    return streams


def craft(rng, orig, ws, family, nref, unused, maxrun, wide_mapping, mapping=None):
    if mapping is None:
        mapping, ns = make_mapping(rng, ws, nref, unused)
    else:
        ns = max(mapping) + 1 + unused
    streams = fill_streams(rng, family, mapping, ns, orig // ws, maxrun)
    full = list(mapping)
    if wide_mapping:  # mapping_size = ws + 2: the extra entries are never read
        full += [int(rng.integers(-2 ** 31, 2 ** 31)) for _ in range(2)]
    return serialize(orig, ws, full, streams)


# --------------------------------------------------------------------------- reading a blob back
def parse(blob: bytes):
    """(orig, ns, ws, msize, mapping[:ws], [stream bytes]) of a well-formed blob."""
    _, orig, ns, ws, msize = struct.unpack_from("<5I", blob, 0)
    mapping = list(struct.unpack_from("<%di" % msize, blob, 20))[:ws]
    off = 20 + 4 * msize
    streams = []
    for _ in range(ns):
        (n,) = struct.unpack_from("<I", blob, off)
        streams.append(blob[off + 4:off + 4 + n])
        off += 4 + n
    return orig, ns, ws, msize, mapping, streams


def takes_fast_path(ws, mapping, num_streams=None) -> bool:
    """parse_fast's rule (psyne_amd/csrc/tdt_decode.h) for a valid blob with at least one whole
    word: a tuned width, at most two referenced streams, each with a per-group segment
    (16 / ws) * k_r of whole dwords — and, where num_streams is given, at most 16 stored streams.
    Every other shape is decoded by decode_one's generic path (tuned widths) or by
    tdt_decode_any_kernel (the other widths)."""
    if ws not in TUNED:
        return False
    if num_streams is not None and num_streams > 16:
        return False
    ref = sorted(set(mapping[:ws]))
    if len(ref) > 2:
        return False
    return all(((16 // ws) * mapping[:ws].count(s)) % 4 == 0 for s in ref)


# --------------------------------------------------------------------------- the cases
def _valid_cases(rng):
    out = []
    for ws in WIDTHS:
        nrefs = sorted({n for n in (1, 2, 3, 4, min(ws, 16)) if n <= ws})
        # ws 1 and 2 leave the fast path only through num_streams > 16: more such cases there
        unused_cycle = (0, 17, 1, 17) if ws <= 2 else (0, 1, 17)
        for i in range(3 * len(SIZES)):  # (i % 8, i % 6): 24 different size / family pairs
            orig, family = SIZES[i % len(SIZES)], FAMILIES[i % len(FAMILIES)]
            nref = nrefs[(i + i // len(nrefs)) % len(nrefs)]
            unused = unused_cycle[i % len(unused_cycle)]
            maxrun = MAXRUNS[(i + i // len(MAXRUNS)) % len(MAXRUNS)]
            wide = i % 4 == 3
            name = "ws%d_%d_%s_r%d_u%d_m%d%s" % (ws, orig, family, nref, unused, maxrun, "_wide" if wide else "")
            out.append(Case(name, ws, family, craft(rng, orig, ws, family, nref, unused, maxrun, wide)))
    # one or two streams that leave the fast path only by their segment shape
    shapes = {8: ([0, 1, 0, 0, 1, 1, 1, 1], [0] * 3 + [1] * 5), 16: ([0, 1] * 3 + [1] * 10, [1] * 5 + [0] * 11)}
    for ws, maps in shapes.items():
        for j, mp in enumerate(maps):
            for orig, family, maxrun in ((5000, "long", 1), (20000, "zero_odd", 3)):
                name = "ws%d_%d_%s_seg%d_m%d" % (ws, orig, family, j, maxrun)
                out.append(Case(name, ws, family, craft(rng, orig, ws, family, 2, 0, maxrun, False, mapping=mp)))
    # above dbig_min
    for ws, family, nref, unused, maxrun, mp in ((4, "long", 3, 0, 3, None), (8, "zero_odd", 2, 0, 255, shapes[8][1]),
                                                 (16, "short", 2, 1, 8, shapes[16][0]), (12, "exact", 4, 0, 2, None),
                                                 (2, "half_odd", 2, 0, 1, None)):
        name = "ws%d_%d_%s_r%d_u%d_m%d" % (ws, BIG, family, nref, unused, maxrun)
        out.append(Case(name, ws, family, craft(rng, BIG, ws, family, nref, unused, maxrun, False, mapping=mp)))
    return out


def _malformed_cases(rng):
    out = []
    for ws in WIDTHS:
        mapping = [b % 2 for b in range(ws)]  # two stored streams at every width (ws 1: one unused)
        streams = fill_streams(rng, "exact", mapping, 2, 5000 // ws, 3)
        if ws == 1:
            streams[1] = pairs(rng, 20, maxrun=7)
        base = serialize(5000, ws, mapping, streams)
        table = 20 + 4 * ws
        (l0,) = struct.unpack_from("<I", base, table)
        end0 = table + 4 + l0
        assert l0 > 8 and end0 + 4 < len(base) - 1

        def add(tag, blob):
            out.append(Case("ws%d_bad_%s" % (ws, tag), ws, "malformed", bytes(blob)))

        def patched(off, value):
            b = bytearray(base)
            struct.pack_into("<i" if value < 0 else "<I", b, off, value)
            return b

        for cut in (0, 3, 4, 19, 20):
            add("cut%d" % cut, base[:cut])
        add("cut_before_table", base[:table - 1])
        add("cut_at_table", base[:table])
        add("cut_in_len0", base[:table + 2])
        add("cut_in_stream0", base[:end0 - 1])
        add("cut_in_len1", base[:end0 + 2])
        add("cut_last_byte", base[:-1])
        add("map_eq_ns", patched(20 + 4 * (ws - 1), 2))
        add("map_negative", patched(20, -1))
        add("msize_short", patched(16, ws - 1))
        add("ws0", patched(12, 0))
        add("magic", patched(0, 0x54445445))
        add("len0_past_end", patched(table, len(base)))
        # a valid blob of word size 65: the oracle decodes it, the library reports TDT_E_UNSUPPORTED
        mp65 = [int(x) for x in rng.integers(0, 2, 65)]
        out.append(Case("ws%d_bad_ws65" % ws, ws, "malformed",
                        serialize(5000, 65, mp65, fill_streams(rng, "exact", mp65, 2, 5000 // 65, 3))))
    return out


_CACHE = {}


def all_cases():
    """Every case, in a fixed order (built once per process)."""
    if "cases" not in _CACHE:
        rng = np.random.default_rng(SEED)
        cases = _valid_cases(rng) + _malformed_cases(rng)
        assert len({c.name for c in cases}) == len(cases)
        check_coverage(cases)
        _CACHE["cases"] = cases
    return _CACHE["cases"]


def valid_cases():
    return [c for c in all_cases() if c.family != "malformed"]


def malformed_cases():
    return [c for c in all_cases() if c.family == "malformed"]


def check_coverage(cases):
    """What the tests rely on; a later edit of the generator cannot quietly lose it.  (Status 0 of
    every valid case is asserted where an oracle runs: make_decode_fuzz.py, test_decode_fuzz.py.)"""
    valid = [c for c in cases if c.family != "malformed"]
    for ws in WIDTHS:
        mine = [c for c in valid if c.ws == ws]
        assert {c.family for c in mine} == set(FAMILIES), ws
        assert {parse(c.blob)[0] for c in mine} >= set(SIZES), ws
        assert any(parse(c.blob)[1] - len(set(parse(c.blob)[4])) == 17 for c in mine), ws
        assert any(parse(c.blob)[3] == ws + 2 for c in mine), ws
    for ws in TUNED:
        # every tuned width reaches the generic path: 4, 8 and 16 by the mapping's shape, 1 and 2
        # only by more than 16 stored streams.  >= 5,000 bytes: five or more 1 KiB windows.
        n = 0
        for c in valid:
            orig, ns, w, _, mp, _ = parse(c.blob)
            n += w == ws and orig >= 5000 and not takes_fast_path(w, mp, ns)
        assert n >= 8, (ws, n)
        assert any(c.ws == ws and takes_fast_path(ws, parse(c.blob)[4], parse(c.blob)[1]) for c in valid), ws
    for ws in (8, 16):  # non-fast by the segment shape alone
        assert any(c.ws == ws and parse(c.blob)[1] <= 2 and len(set(parse(c.blob)[4])) <= 2 and
                   not takes_fast_path(ws, parse(c.blob)[4], parse(c.blob)[1]) for c in valid), ws
    assert sum(parse(c.blob)[0] == BIG for c in valid) <= 6
    bad = [c for c in cases if c.family == "malformed"]
    assert all(sum(c.ws == ws for c in bad) == 18 for ws in WIDTHS)


# --------------------------------------------------------------------------- the plain decoder
def numpy_decode(blob: bytes) -> bytes:
    """decode of a well-formed TDT blob in plain numpy, independent of the oracle: every stream
    run-length expanded (np.repeat), cut or zero-padded to its share of the words, and scattered
    into the columns of a (words, ws) view; bytes past the last whole word stay zero."""
    orig, _, ws, _, mapping, streams = parse(blob)
    wc = orig // ws
    out = np.zeros(orig, np.uint8)
    words = out[: wc * ws].reshape(wc, ws)
    for s in sorted(set(mapping)):
        cols = [b for b in range(ws) if mapping[b] == s]
        raw = np.frombuffer(streams[s], np.uint8)
        n = raw.size // 2  # an odd trailing byte is no pair
        dec = np.repeat(raw[1:2 * n:2], raw[0:2 * n:2])[: wc * len(cols)]
        share = np.zeros(wc * len(cols), np.uint8)
        share[: dec.size] = dec
        words[:, cols] = share.reshape(wc, len(cols))
    return out.tobytes()
