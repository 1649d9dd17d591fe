"""Fixtures of the raw fallback (TDT_OPT_RAW_FALLBACK): messages on both sides of the rule
"E > n + 4 -> the UNCP blob", generated deterministically and judged by the CPU oracle.

    expected(x) = b if len(b) <= n + 4 else "UNCP" + x,   b = Oracle.encode(x, cfg, mapping=...)

Kinds (one of each in every batch, interleaved, so that a fallback's neighbours are TDT blobs):
    uniform      uniform random bytes: expands at every width
    dense        fp32 N(0, 1e-3) without zeros, a dense gradient: expands at width 4
    grad70       the benchmark's gradient, 70 % zeros: compresses
    odd / short / ragged / empty
                 messages the UNCP routing takes whatever the option says: n % 4 != 0, n < 64,
                 n % ws != 0 (where a multiple of 4 that is no multiple of ws exists), n == 0
    thr-2 / thr0 / thr+2
                 len(b) - (n + 4) = -2, 0, +2: the last TDT blob, the tie (stays TDT) and the first
                 fallback.  Words of a cheap and a dear variant; every dear word adds one run pair
                 (2 bytes) to the blob, and the count of dear words is solved on the oracle.
    one-2 / one0 / one+2 (the mapped calls)
                 the same trio under the single-stream mapping (every position in stream 0), where
                 E = 24 + 4 ws + 2 P for P runs of the message's bytes.
"""
import json
import pathlib

import numpy as np

from tests.support import digest

UNCP = b"PCNU"  # 0x554E4350, little-endian
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "raw_fallback.json"

# (word size, message size): the smallest sizes that reach every class of the encode.  Tuned widths:
# small (<= 4 KiB), mid (<= 32 KiB), medium resident (<= 64 KiB), medium streaming; TILED under
# TDT_OPT_LARGE_MIN = 65,536.  Generic widths: one workgroup, and tiles at 196,608.
TUNED_SIZES = {4: [1024, 4096, 4100, 8192, 32768, 32772, 65536, 65540, 131088],
               1: [1024, 65536], 2: [1024, 65536], 8: [1024, 65536], 16: [1024, 65536]}
TUNED_TILED = {4: [196640, 589840], 1: [196640], 2: [196640], 8: [196640], 16: [196640]}
GENERIC_SIZES = {3: [1032, 12288, 49152], 12: [1032, 12288, 49152], 40: [1040, 40960]}
GENERIC_TILED = {3: [196608], 12: [196608]}
LARGE_MIN_TILED = 65536
MAPPED_TRIOS = [(4, 1024), (4, 65536), (2, 4096), (12, 12288)]  # (ws, n) of the single-stream threshold trios


def expected_blob(orc, x, ws, mapping=None, policy_on=True):
    """(expected blob under the option, the oracle's plain blob)."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    b = orc.encode(x, cfg=orc.config(sample_fraction=1.0, word_size=ws), bandwidth=10.0 if policy_on else 1000.0,
                   mapping=mapping)
    return (b if len(b) <= x.size + 4 else UNCP + x.tobytes()), b


# ---- the plain kinds -----------------------------------------------------------------------------
def uniform(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def dense(n, seed):
    """fp32 N(0, 1e-3) with no zero among them, as bytes (n // 4 values, the rest zero bytes)."""
    g = np.random.default_rng(seed).normal(0.0, 1e-3, n // 4).astype(np.float32)
    g[g == 0] = np.float32(1e-3)
    out = np.zeros(n, np.uint8)
    out[: 4 * (n // 4)] = g.view(np.uint8)
    return out


def grad70(n, seed):
    """The benchmark's gradient: fp32 N(0, 0.01), 70 % of the values zero."""
    rng = np.random.default_rng(seed)
    g = rng.normal(0.0, 0.01, n // 4).astype(np.float32)
    g[rng.random(n // 4) < 0.7] = 0
    out = np.zeros(n, np.uint8)
    out[: 4 * (n // 4)] = g.view(np.uint8)
    return out


# ---- the threshold trios -------------------------------------------------------------------------
def _succ(r):
    """The next byte in the ring 8..255."""
    return 8 + (r - 7) % 248


def _chain(rng, count):
    """`count` bytes in 8..255, none equal to its predecessor or to the predecessor's successor."""
    if count <= 124:  # few words: every r_j and every successor once, so that each position's entropy is log2(count)
        return 8 + 2 * rng.permutation(124)[:count].astype(np.int64)
    step = rng.integers(2, 248, count, dtype=np.int64)  # (a step of 0 or 1 would give the predecessor or its successor)
    step[0] = rng.integers(0, 248)
    return 8 + np.cumsum(step) % 248


def threshold_words(n, ws, k, seed):
    """n bytes of ws-byte words with k dear units, one run pair (2 bytes of blob) each.  ws >= 3:
    positions 0 .. ws-2 of word j hold one byte r_j of 8..255 (neighbouring words differ), the last
    position 0; a word takes up to ws-2 units, and with e of them its last e positions before the
    zero alternate between r_j's successor in that ring and r_j — e more runs, and every position
    keeps a uniform spread over the ring, so the mapping does not move with k.  The units fill the words from the first on.
    ws <= 2: every position holds the constant 7 where the word is cheap and r_j where it is dear
    (one unit per word)."""
    nw = n // ws
    r = _chain(np.random.default_rng(seed), nw)
    w = np.zeros((nw, ws), np.int64)
    if ws <= 2:
        w[:, :] = 7
        w[:k, :] = r[:k, None]
        return w.astype(np.uint8).reshape(-1)
    w[:, : ws - 1] = r[:, None]
    per = ws - 2
    e = np.zeros(nw, np.int64)
    e[: k // per] = per
    if k % per and k // per < nw:
        e[k // per] = k % per
    start = (ws - 1) - e  # first position of a word's alternating tail (>= 1)
    p = np.arange(ws - 1)[None, :]
    odd = (p >= start[:, None]) & ((p - start[:, None]) % 2 == 0)
    w[:, : ws - 1] = np.where(odd, _succ(r)[:, None], w[:, : ws - 1])
    return w.astype(np.uint8).reshape(-1)


def solve_threshold(orc, n, ws, diff, seed, mapping=None, build=threshold_words):
    """The message of build(n, ws, k, seed) whose oracle blob is n + 4 + diff bytes long: k by the
    closed form (2 bytes per dear word), then by bisection if the blob's other terms moved."""
    def gap(k):
        x = build(n, ws, k, seed)
        return len(expected_blob(orc, x, ws, mapping)[1]) - (n + 4), x
    kmax = n if build is run_bytes else (n // ws) * max(1, ws - 2)
    g0, x = gap(0)
    if g0 > diff:
        raise ValueError("threshold base above the target at ws %d, n %d: %d" % (ws, n, g0))
    k = min(kmax, (diff - g0) // 2)
    g, x = gap(k)
    if g != diff:
        lo, hi = 0, kmax
        while lo < hi:
            mid = (lo + hi) // 2
            if gap(mid)[0] < diff:
                lo = mid + 1
            else:
                hi = mid
        k = lo
        g, x = gap(k)
    if g != diff:
        raise ValueError("no message with gap %+d at ws %d, n %d (k %d gives %+d)" % (diff, ws, n, k, g))
    return x


def run_bytes(n, ws, k, seed):
    """n bytes in 2-valued runs for the single-stream mapping: the first k bytes alternate (a run
    each), the rest is one value in runs the 255 cap cuts."""
    x = np.full(n, 0x11, np.uint8)
    x[:k:2] = 0x5A
    if k and k < n and x[k - 1] == x[k]:
        x[k:] = 0x5A
    return x


# ---- batches -------------------------------------------------------------------------------------
def ragged_size(n, ws):
    """A multiple of 4 near n that is no multiple of ws (None where every multiple of 4 is one)."""
    for d in (4, 8, 12, 16, 20):
        if (n + d) % ws:
            return n + d
    return None


def batch(orc, ws, n, seed):
    """Every kind at (ws, n): a list of dicts name, kind, x, want, plain, falls (True: the rule stores
    the message raw)."""
    out = []

    def add(kind, x, mapping=None):
        want, plain = expected_blob(orc, x, ws, mapping)
        out.append(dict(name="%s/ws%d/n%d" % (kind, ws, n), kind=kind, ws=ws, x=x, want=want, plain=plain,
                        falls=want != plain, mapping=mapping))

    add("uniform", uniform(n, seed))
    add("thr-2", solve_threshold(orc, n, ws, -2, seed + 1))
    add("grad70", grad70(n, seed + 2))
    add("odd", uniform(n + 1, seed + 3))
    add("thr0", solve_threshold(orc, n, ws, 0, seed + 4))
    add("dense", dense(n, seed + 5))
    add("short", uniform(60, seed + 6))
    add("empty", np.zeros(0, np.uint8))
    add("thr+2", solve_threshold(orc, n, ws, +2, seed + 7))
    r = ragged_size(n, ws)
    if r is not None:
        add("ragged", uniform(r, seed + 8))
    return out


def mapped_trio(orc, ws, n):
    """The single-stream threshold trio at (ws, n), with the mapping (all zeros) it is defined under."""
    out = []
    for diff in (-2, 0, +2):
        mp = [0] * ws
        x = solve_threshold(orc, n, ws, diff, 0, mapping=mp, build=run_bytes)
        want, plain = expected_blob(orc, x, ws, mp)
        out.append(dict(name="one%+d/ws%d/n%d" % (diff, ws, n), kind="one%+d" % diff, ws=ws, x=x, want=want, plain=plain,
                        falls=want != plain, mapping=mp))
    return out


def seed_of(ws, n):
    return 20270000 + 1000 * ws + n % 997


def case_digest(case):
    return dict(n=int(case["x"].size), plain_len=len(case["plain"]), falls=bool(case["falls"]),
                x=digest(case["x"].tobytes()),
                want=digest(case["want"]))


def all_configs():
    """Every (ws, n, tiled) the GPU tests run."""
    cfgs = []
    for table, tiled in ((TUNED_SIZES, False), (TUNED_TILED, True), (GENERIC_SIZES, False), (GENERIC_TILED, True)):
        for ws, sizes in table.items():
            cfgs += [(ws, n, tiled) for n in sizes]
    return cfgs


def load_golden():
    return json.loads(GOLDEN.read_text())


def golden_table(orc):
    table = {}
    for ws, n, _ in all_configs():
        for c in batch(orc, ws, n, seed_of(ws, n)):
            table[c["name"]] = case_digest(c)
    for ws, n in MAPPED_TRIOS:
        for c in mapped_trio(orc, ws, n):
            table[c["name"]] = case_digest(c)
    return table


if __name__ == "__main__":  # python -m tests.raw_fallback_cases: rewrite the digests from the oracle
    from oracle.oracle import Oracle
    GOLDEN.write_text(json.dumps(golden_table(Oracle()), indent=0, sort_keys=True) + "\n")
    print("wrote", GOLDEN)
