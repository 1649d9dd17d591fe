"""Routing cases: every term of the decision that stands in front of each encode — TDT blob or "UNCP"
plus the raw bytes — flipped alone, at every tuned and three generic widths and in every message class.
No GPU and no fixture bytes: everything follows from SEED.  The record of what the compiled reference
makes of them is tests/golden/policy_matrix.json (tests/golden/make_policy_matrix.py); the CPU test is
tests/test_policy_matrix.py, the GPU routes tests/test_gpu_policy_matrix.py.

The decision is the reference's should_transform (tdt_compression.hpp:186-201) plus compress_tdt's size
guard (:364-367, whose exception encode turns into the passthrough, :256-265):

    cpu <= cpu_threshold && bandwidth < bandwidth_threshold
    && n >= min_tensor_size && n % 4 == 0 && n >= 64 && n % word_size == 0      (&& n < 2^32)

A case is (name, ws, n, min_tensor, bandwidth, cpu, bandwidth_threshold, cpu_threshold, term, side,
message).  Exactly one term decides it: every other term holds, and the term named by `term` sits on
its last value on the failing side (side "off": the blob is raw) or its first value on the holding side
(side "on": a TDT blob), so that a wrong operator or a dropped term fails a named case.  "Legal" sizes
are the multiples of lcm(4, ws).

    mt     min_tensor_size in MT_VALUES: the largest legal n below it (off), n equal to it where that is
           legal and the first legal n above (on); at 200000 also 98304, 131072 (off) and 262144 (on).  The
           values 0 and 64 give "on" cases only: below them n >= 64 fails as well, which is `n64`'s case.
    mod4   widths 1, 2, 3: n = k lcm + ws (no multiple of 4, a whole number of words) beside k lcm
    modws  widths 8, 16, 3, 12, 40: n = k lcm + 4 (a multiple of 4, no whole number of words) beside k lcm;
           both at three k around each of CLASS_SIZES, with min_tensor_size = MOD_MIN_TENSOR
    n64    min_tensor_size 0: the last legal n below 64, 64 where legal, the first legal n above; also at
           width 32, which has this term's cases alone: the one generic width below 64 that divides 64,
           where `n >= 64` and `n > 64` part (at 3, 12 and 40 a 64-byte message fails n % word_size too)
    bw     thresholds (100, 0.8): bandwidth 100 off, nextafter(100, 0) on, 1000 off; thresholds
           (50, 0.8): 49.9 on, 50 and 75 off (75 is below the default 100: a literal fails here)
    cpu    thresholds (100, 0.8): cpu 0.8 on (the reference tests `>`), nextafter(0.8, 1) off;
           thresholds (100, 0.25): 0.25 on, 0.3 off (0.3 is below the default 0.8)
           — `bw` and `cpu` at the legal sizes at or below each of METRIC_SIZES

`modws` is the one term the reference's should_transform does not hold (the guard lives in
compress_tdt): there the predicate says yes and the blob is raw all the same (`predicate()`, `compresses()`).

The `n < 2^32` term cannot be reached with small shapes and is out of scope here.  Two restatements
differ in it: psyne_amd/csrc/tdt_anyws.hip:261 (the whole-message kernel of the generic widths) has
it, tdt_anyws.hip:497 (their tiled scan) does not.

Content: a sparse float32 gradient (nine zeros in ten) at the tuned widths, and at the generic ones
words whose positions b % 3 == 0 are random where the others change slowly; every message is a prefix
of its width's one buffer, whose first bytes are nearly constant so that the shortest messages
compress too.  The module asserts nothing about blobs itself (it has no codec); `check_blob_lengths`
is called with the oracle's lengths by the CPU test and the pin script: a TDT blob is never n + 4
bytes long, so a route that takes the wrong branch shows in the length as well as in the bytes, and it
is longer than n + 4 only where the frame alone is (`frame_exceeds`), which no content can mend."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

SEED = 0x901C7
TUNED = (1, 2, 4, 8, 16)
GENERIC = (3, 12, 40)
N64_ONLY = (32,)  # a generic width that divides 64: at 3, 12 and 40 no message of 64 bytes holds whole words
WIDTHS = TUNED + GENERIC + N64_ONLY
MT_VALUES = (0, 64, 1024, 4112, 32784, 65552, 200000)
MT_EXTRA = ((98304, "off"), (131072, "off"), (262144, "on"))  # at min_tensor_size 200000: big and raw, tiled and raw, tiled and TDT
CLASS_SIZES = (1024, 4096, 32768, 65536, 131072)
METRIC_SIZES = (4096, 65536, 131072)
MOD_MIN_TENSOR = 512
MAX_N = 262144
CLASSES = ("small", "mid", "medium", "big", "tiled")
DEFAULTS = dict(min_tensor=1024, bandwidth=10.0, cpu=0.5, bandwidth_threshold=100.0, cpu_threshold=0.8)
BW_ROWS = ((100.0, 0.8, 100.0, "off"), (100.0, 0.8, float(np.nextafter(100.0, 0.0)), "on"), (100.0, 0.8, 1000.0, "off"),
           (50.0, 0.8, 49.9, "on"), (50.0, 0.8, 50.0, "off"), (50.0, 0.8, 75.0, "off"))
CPU_ROWS = ((100.0, 0.8, 0.8, "on"), (100.0, 0.8, float(np.nextafter(0.8, 1.0)), "off"),
            (100.0, 0.25, 0.25, "on"), (100.0, 0.25, 0.3, "off"))


class Case(NamedTuple):
    name: str
    ws: int
    n: int
    min_tensor: int
    bandwidth: float
    cpu: float
    bandwidth_threshold: float
    cpu_threshold: float
    term: str
    side: str
    message: np.ndarray


def lcm4(ws: int) -> int:
    return 4 * ws // math.gcd(4, ws)


def message_class(n: int) -> str:
    """The class edges of tdt_api.hip (kSmallMax = 4096, kMidMax = 32768, kBigMin = 65536; `geometry()`
    in tests/encode_run_cases.py); `tiled`: what TDT_OPT_LARGE_MIN = 65536 hands to the tiles in the
    batches of the GPU tests, taken from 128 KiB on so that `big` keeps cases of its own."""
    return ("small" if n <= 4096 else "mid" if n <= 32768 else "medium" if n <= 65536 else
            "big" if n < 131072 - 4096 else "tiled")


def predicate(n, min_tensor, bandwidth, cpu, bandwidth_threshold, cpu_threshold) -> bool:
    """should_transform: the public predicate, which knows no word size."""
    return (cpu <= cpu_threshold and bandwidth < bandwidth_threshold and n >= min_tensor and n % 4 == 0
            and n >= 64)


def compresses(ws, n, min_tensor, bandwidth, cpu, bandwidth_threshold, cpu_threshold) -> bool:
    """Whether encode gives a TDT blob: the predicate and compress_tdt's guard."""
    return predicate(n, min_tensor, bandwidth, cpu, bandwidth_threshold, cpu_threshold) and n % ws == 0 and n > 0


def terms_of(ws: int) -> tuple:
    if ws in N64_ONLY:
        return ("n64",)
    return tuple(t for t in ("mt", "mod4", "modws", "n64", "bw", "cpu")
                 if (t != "mod4" or ws in (1, 2, 3)) and (t != "modws" or ws in (8, 16, 3, 12, 40)))


def classes_of(term: str) -> tuple:
    """The classes a term's cases reach: `n64` lives below 4 KiB, `bw` and `cpu` at METRIC_SIZES."""
    if term == "n64":
        return ("small",)
    if term in ("bw", "cpu"):
        return tuple(dict.fromkeys(message_class(n) for n in METRIC_SIZES))
    return CLASSES


# ------------------------------------------------------------------ content
QUIET = 256  # the buffer's first bytes: zero but for one (the messages of up to 128 bytes are constant)


@functools.lru_cache(maxsize=None)
def buffer(ws: int) -> np.ndarray:
    rng = np.random.default_rng([SEED, ws])
    if ws in TUNED:
        x = rng.normal(0, 0.01, MAX_N // 4).astype(np.float32)
        x[rng.random(x.size) < 0.9] = 0
        buf = x.view(np.uint8).copy()
    else:
        wc = MAX_N // ws + 1
        msg = np.empty((wc, ws), np.uint8)
        hi = [b for b in range(ws) if b % 3 == 0]
        lo = [b for b in range(ws) if b % 3]
        msg[:, hi] = rng.integers(0, 256, (wc, len(hi)), dtype=np.uint8)
        msg[rng.random(wc) < 0.9] = 0  # (sparse, as the gradient: most words are zero)
        runs = rng.geometric(1.0 / 40.0, wc * len(lo) // 8 + 64)
        vals = rng.integers(0, 4, runs.size).astype(np.uint8)
        msg[:, lo] = np.repeat(vals, runs)[: wc * len(lo)].reshape(wc, len(lo))
        buf = msg.reshape(-1)[:MAX_N].copy()
    buf[:QUIET] = 0
    buf[150] = 0xBD
    buf.setflags(write=False)
    return buf


def _case(ws, term, tag, n, side, **kw) -> Case:
    f = dict(DEFAULTS, **kw)
    assert 0 < n <= MAX_N
    name = "ws%d_%s_%s_n%d_%s" % (ws, term, tag, n, side)
    return Case(name, ws, n, f["min_tensor"], f["bandwidth"], f["cpu"], f["bandwidth_threshold"], f["cpu_threshold"],
                term, side, buffer(ws)[:n])


def _legal_at_or_below(x: int, q: int) -> int:
    return x // q * q


def width_cases(ws: int) -> list:
    q = lcm4(ws)
    out = []
    # mt
    for mt in MT_VALUES if "mt" in terms_of(ws) else ():
        below = _legal_at_or_below(mt - 1, q) if mt > 0 else 0
        first = max(-(-mt // q) * q, -(-64 // q) * q)  # the first legal n that holds mt and n >= 64
        above = first + q if first == mt else first
        if below >= 64:
            out.append(_case(ws, "mt", "mt%d" % mt, below, "off", min_tensor=mt))
        if first == mt:
            out.append(_case(ws, "mt", "mt%d" % mt, mt, "on", min_tensor=mt))
        out.append(_case(ws, "mt", "mt%d" % mt, above, "on", min_tensor=mt))
    for size, side in MT_EXTRA if "mt" in terms_of(ws) else ():
        out.append(_case(ws, "mt", "mt200000", _legal_at_or_below(size, q), side, min_tensor=200000))
    # mod4, modws
    for term, delta in (("mod4", ws), ("modws", 4)):
        if term not in terms_of(ws):
            continue
        for size in CLASS_SIZES:
            base = _legal_at_or_below(size, q)
            for j in ((0, 1, 2) if size == CLASS_SIZES[0] else (-1, 0, 1)):
                k = base + j * q
                bad = k + delta
                assert (bad % 4 != 0 and bad % ws == 0) if term == "mod4" else (bad % 4 == 0 and bad % ws != 0)
                out.append(_case(ws, term, "c%d" % size, k, "on", min_tensor=MOD_MIN_TENSOR))
                out.append(_case(ws, term, "c%d" % size, bad, "off", min_tensor=MOD_MIN_TENSOR))
    # n64
    below = _legal_at_or_below(63, q)
    first = -(-64 // q) * q
    if below:
        out.append(_case(ws, "n64", "mt0", below, "off", min_tensor=0))
    out.append(_case(ws, "n64", "mt0", first, "on", min_tensor=0))
    if first == 64:
        out.append(_case(ws, "n64", "mt0", 64 + q, "on", min_tensor=0))
    # bw, cpu
    for size in METRIC_SIZES if "bw" in terms_of(ws) else ():
        n = _legal_at_or_below(size, q)
        for bt, ct, bw, side in BW_ROWS:
            out.append(_case(ws, "bw", "t%g_b%r" % (bt, bw), n, side, bandwidth=bw, bandwidth_threshold=bt, cpu_threshold=ct))
        for bt, ct, cpu, side in CPU_ROWS:
            out.append(_case(ws, "cpu", "t%g_c%r" % (ct, cpu), n, side, cpu=cpu, bandwidth_threshold=bt, cpu_threshold=ct))
    return out


@functools.lru_cache(maxsize=1)
def _all() -> tuple:
    out = [c for ws in WIDTHS for c in width_cases(ws)]
    names = [c.name for c in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    for c in out:
        assert c.message.size == c.n
        assert compresses(c.ws, c.n, *c[3:8]) == (c.side == "on"), c.name
        flipped = flipped_terms(c)
        assert flipped == ([c.term] if c.side == "off" else []), (c.name, flipped)
    return tuple(out)


def flipped_terms(c: Case) -> list:
    """The names of the terms that fail for a case (bw and cpu counted apart)."""
    return [t for t, ok in (("mt", c.n >= c.min_tensor), ("mod4", c.n % 4 == 0), ("modws", c.n % c.ws == 0),
                            ("n64", c.n >= 64), ("bw", c.bandwidth < c.bandwidth_threshold),
                            ("cpu", c.cpu <= c.cpu_threshold)) if not ok]


def all_cases() -> list:
    """Every case; built once, the messages read-only views of their width's buffer."""
    return list(_all())


def config_key(c: Case) -> tuple:
    """What a context is created with: cases that share it share a context in the GPU tests."""
    return (c.ws, c.min_tensor, c.bandwidth_threshold, c.cpu_threshold)


def metrics_key(c: Case) -> tuple:
    return (c.bandwidth, c.cpu)


def check_coverage(cases):
    """At every width, each term that applies to it has an `on` and an `off` case in every message
    class the term reaches (`classes_of`); the `mt` values and the `bw` / `cpu` rows are all there;
    and in the `on` neighbour of every `off` case only the named term differs."""
    seen = {}
    for c in cases:
        seen.setdefault((c.ws, c.term, message_class(c.n)), set()).add(c.side)
    for ws in WIDTHS:
        sub = [c for c in cases if c.ws == ws]
        for term in terms_of(ws):
            for cl in classes_of(term):
                got = seen.get((ws, term, cl), set())
                assert got == {"on", "off"}, "width %d term %s class %s has %s" % (ws, term, cl, sorted(got))
        if "mt" not in terms_of(ws):
            continue
        assert {c.min_tensor for c in sub if c.term == "mt"} == set(MT_VALUES), ws
        for mt in MT_VALUES[2:]:
            sides = [c.side for c in sub if c.term == "mt" and c.min_tensor == mt]
            assert sides.count("off") >= 1 and sides.count("on") >= 1, (ws, mt)
        for n in {c.n for c in sub if c.term in ("bw", "cpu")}:
            rows = {(c.bandwidth_threshold, c.cpu_threshold, c.bandwidth, c.side) for c in sub if c.term == "bw" and c.n == n}
            assert rows == set(BW_ROWS), (ws, n)
            rows = {(c.bandwidth_threshold, c.cpu_threshold, c.cpu, c.side) for c in sub if c.term == "cpu" and c.n == n}
            assert rows == set(CPU_ROWS), (ws, n)
        assert not [c.name for c in sub if c.term not in terms_of(ws)]
        assert max(c.n for c in sub) <= MAX_N


def frame_exceeds(c: Case) -> bool:
    """A TDT blob's frame — 20 header bytes, the mapping, and a length and one pair per stream, of
    which there is at least one — is longer than n + 4 whatever the content."""
    return 20 + 4 * c.ws + 4 + 2 > c.n + 4


def check_blob_lengths(cases, lengths):
    """The two premises about the content, given the oracle's blob lengths (name -> length)."""
    for c in cases:
        if c.side == "off":
            assert lengths[c.name] == c.n + 4, c.name
            continue
        assert lengths[c.name] != c.n + 4, "%s: a TDT blob of n + 4 bytes" % c.name
        assert (lengths[c.name] > c.n + 4) == frame_exceeds(c), "%s: %d bytes" % (c.name, lengths[c.name])
