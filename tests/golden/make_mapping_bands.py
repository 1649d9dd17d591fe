#!/usr/bin/env python3
"""Generate tests/golden/mapping_bands.json: messages whose byte-position entropies tie, or nearly
tie, with their mean, at chosen distances around the encoder's fast-decision margin.

Run after `make -C oracle` (well under a minute; with the compiled reference present its mapping is
recorded per case and its blob is compared with the oracle's; a rerun gives the same bytes):

    python tests/golden/make_mapping_bands.py

tests/mapping_band_cases.py describes the stored form, the bands and the sign.  Per (width, size) cell:

  * near ties   one case per band and sign.  All ws positions share a histogram; j of them get a copy
                with one to three samples moved between bins.  A seeded rejection search over
                histograms and moves finds an entropy difference that puts the smallest gap in the
                wanted band; the band and sign are then confirmed from the oracle's own entropies
                (tdt_oracle_analyze) with the mean taken exactly.  j rotates over 1, ws/2 and ws - 1 and
                the perturbed positions rotate with the case; where three moves cannot reach a band
                with the j in turn (the large gaps of long messages), the next j is taken.
                At word sizes 4 and 8 above 65536 bytes the '+' case of band (M/4, M) and the '-' case
                of band [M, 2M) perturb exactly the positions that give the mapping the encoder
                speculates on ([1,1,1,0], [1,1,1,1,1,1,0,0]); the other cases give other mappings.
                One case per width (size 65536 / 65532, band [2M, 10M), '-') has a 256-symbol alphabet.
  * indep       near ties between unrelated histograms, in bands (0, M/4] and [M, 2M) and both signs:
                the perturbed positions carry a histogram drawn on its own (another alphabet, other
                counts) and steered until its entropy lies the wanted distance from the base's; in band
                (0, M/4] the nearest tie of twelve such draws is kept (gaps down to M / 65536).  In the
                family above all but six bins are the same numbers at every position, so the error of
                an approximate entropy cancels in e_b - mean(e); here it does not.
  * exact ties  a constant message, and same-histogram positions with every count <= 64, every count
                > 64, and counts on both sides of 64, where the word count allows (tie_kinds).  The
                mapping of a tie hangs on the rounding of the entropy sum: all zeros, or all ones with
                an empty stream 0.  At word sizes 3, 8, 12 and 16 up to 64 further histograms are drawn
                per cell until both outcomes are present (family `extra`).  Width 1 has one position:
                ties only.

Tie outcomes found (recorded in the JSON's `tie_outcomes`, asserted by tests/test_mapping_bands.py):
word sizes 3, 8, 12 and 16 show both outcomes in every cell; word sizes 1, 2 and 4 only all zeros
(none was searched for there).  No band needed another j than the one in turn.
"""
from __future__ import annotations

import json
import math
import pathlib
import struct
import sys
import zlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle.oracle import Oracle, Reference  # noqa: E402
from tests import mapping_band_cases as mb  # noqa: E402

SEED = 0xBA9D5
DRAWS = 600        # histograms tried per (case, j)
CANDIDATES = 40000  # move sets tried per histogram
BOTH_OUTCOMES = (3, 8, 12, 16)
DEEP_DRAWS = 12    # histograms compared for the deepest near tie of a cell


def draw_sym(rng) -> list:
    """[a, b] of the alphabet rule: symbol i is (a * i + b) mod 256, a odd."""
    return [2 * int(rng.integers(0, 128)) + 1, int(rng.integers(0, 256))]


def spread(rng, total: int, k: int, floor: int, skew: float) -> np.ndarray:
    """k counts >= floor that sum to total, log-uniform weights over a ratio of e^skew."""
    w = np.exp(rng.uniform(0.0, skew, k))
    rest = total - floor * k
    assert rest >= 0
    c = floor + np.floor(rest * w / w.sum()).astype(np.int64)
    c[int(np.argmax(w))] += total - int(c.sum())
    return c


def draw_hist(rng, n: int, kind: str, k256: bool = False):
    """(alphabet rule, counts) of the wanted family summing to n, or None where this draw does not fit."""
    if kind == "const":
        return [1, int(rng.integers(1, 256))], [n]
    if kind == "any":
        kmax = min(256 if k256 else 24, n // 2)
        k = kmax if k256 else int(np.exp(rng.uniform(np.log(6), np.log(kmax + 0.99))))
        if rng.random() < 0.3:  # a few bins of one or two samples beside heavy ones: the largest moves
            small = rng.integers(1, 3, max(3, k // 2))
            counts = np.concatenate([small, spread(rng, n - int(small.sum()), k - small.size, 1,
                                                   rng.uniform(0, 3))])
        else:
            counts = spread(rng, n, k, 1, rng.uniform(0.0, np.log(n)))
    elif kind == "le64":
        lo = -(-n // 64)
        cap = 64 if lo <= 56 else 256
        k = min(cap, n, max(2, lo + int(rng.integers(1, 9))))
        counts = np.full(k, n // k, np.int64)
        counts[: n % k] += 1
        if counts.max() > 64:
            return None
        for _ in range(4 * k):
            a, b = rng.integers(0, k, 2)
            amt = int(rng.integers(0, min(counts[a] - 1, 64 - counts[b]) + 1)) if a != b else 0
            counts[a] -= amt
            counts[b] += amt
    elif kind == "gt64":
        k = int(rng.integers(2, min(64, n // 65) + 1))
        counts = spread(rng, n, k, 65, rng.uniform(0.0, 4.0))
    elif kind == "mixed":
        big = int(rng.integers(1, min(32, (n - 1) // 65) + 1))
        k1 = int(rng.integers(1, min(32, n - 65 * big) + 1))
        small = rng.integers(1, 65, k1)
        if n - int(small.sum()) < 65 * big:
            return None
        counts = np.concatenate([small, spread(rng, n - int(small.sum()), big, 65, rng.uniform(0.0, 4.0))])
    else:
        raise ValueError(kind)
    counts = counts[rng.permutation(counts.size)]
    assert int(counts.sum()) == n and counts.min() >= 1
    return draw_sym(rng), [int(c) for c in counts]


def find_moves(rng, counts, n: int, lo: float, hi: float, nearest=None):
    """Up to three moves between different bins whose entropy change lies in [lo, hi) (lo, hi of one
    sign): the first such set sampled, or with `nearest` the one whose change is nearest to it."""
    c = np.asarray(counts, np.float64)
    k = c.size

    def f(x):
        p = np.maximum(x, 1e-300) / n
        return np.where(x > 0, -p * np.log2(p), 0.0)

    dminus, dplus = f(c - 1) - f(c), f(c + 1) - f(c)
    bins = rng.integers(0, k, (CANDIDATES, 6))
    nm = rng.integers(1, 4, CANDIDATES)
    srt = np.sort(bins, axis=1)
    distinct = (np.diff(srt, axis=1) != 0)
    # only the first 2 * nm columns are used; demand all six distinct (simple, and k >= 6)
    ok = distinct.all(axis=1)
    d = np.zeros(CANDIDATES)
    for m in range(3):
        use = nm > m
        d += np.where(use, dminus[bins[:, 2 * m]] + dplus[bins[:, 2 * m + 1]], 0.0)
    hit = np.flatnonzero(ok & (d >= lo) & (d < hi))
    if hit.size == 0:
        return None
    t = int(hit[0] if nearest is None else hit[int(np.argmin(np.abs(d[hit] - nearest)))])
    return [[int(bins[t, 2 * m]), int(bins[t, 2 * m + 1])] for m in range(int(nm[t]))]


def entropy(counts, n: int) -> float:
    c = np.asarray(counts, np.float64)
    c = c[c > 0]
    return float(-(c / n * np.log2(c / n)).sum())


def find_indep(rng, n: int, base_counts, lo: float, hi: float, deep: bool = False):
    """(alphabet rule, counts) of a histogram drawn independently of the base, another alphabet and other
    counts, steered until its entropy minus the base's lies in [lo, hi): the skew of its weights by
    bisection, then single moves while they help, then up to three sampled moves.  deep: of the
    sampled move sets the one that brings the difference nearest to the window's inner edge."""
    target = entropy(base_counts, n)
    cap = min(32, n // 2)
    k = int(2.0 ** target * rng.uniform(1.3, 3.0)) + 2
    if k > cap or k < 6:
        return None
    u = rng.uniform(0.0, 1.0, k)

    def shaped(t):
        w = np.exp(u * t)
        c = 1 + np.floor((n - k) * w / w.sum()).astype(np.int64)
        c[int(np.argmax(w))] += n - int(c.sum())
        return c

    a, b = 0.0, 2.0 * np.log(n) + 8.0
    if entropy(shaped(a), n) < target or entropy(shaped(b), n) > target:
        return None
    for _ in range(60):
        t = 0.5 * (a + b)
        if entropy(shaped(t), n) > target:
            a = t
        else:
            b = t
    c = shaped(a)
    mid = 0.5 * (lo + hi)
    for _ in range(400):
        cur = entropy(c, n) - target - mid
        if lo <= cur + mid < hi:
            break
        x = c.astype(np.float64)

        def f(y):
            p = np.maximum(y, 1e-300) / n
            return np.where(y > 0, -p * np.log2(p), 0.0)

        dminus = np.where(c >= 2, f(x - 1) - f(x), np.inf)
        change = dminus[:, None] + (f(x + 1) - f(x))[None, :]
        np.fill_diagonal(change, np.inf)
        left = np.abs(cur + change)
        i, j = np.unravel_index(int(np.argmin(left)), left.shape)
        if not left[i, j] < abs(cur):
            break
        c[i] -= 1
        c[j] += 1
    cur = entropy(c, n) - target
    if deep or not lo <= cur < hi:
        inner = lo if lo > 0 else hi  # the edge next to zero
        moves = find_moves(rng, c, n, lo - cur, hi - cur, nearest=inner - cur if deep else None)
        if moves is None:
            return None
        for i, j in moves:
            c[i] -= 1
            c[j] += 1
    assert int(c.sum()) == n and c.min() >= 0
    return draw_sym(rng), [int(v) for v in c]


def main():
    orc = Oracle()
    ref = Reference() if Reference.available() else None
    M = mb.fast_margin()
    # search windows inside each band, clear of its edges; band 0 keeps a real gap, not a rounding one
    windows = [(M / 32, 0.98 * M / 4), (1.02 * M / 4, 0.98 * M), (1.02 * M, 0.98 * 2 * M), (1.02 * 2 * M, 0.98 * 10 * M)]
    cases, outcomes, fallbacks, deepest = [], {}, 0, []

    def finish(case):
        mb.expand(case)
        msg = mb.build(case)
        case["_crc"] = zlib.crc32(msg.tobytes())
        ws = case["ws"]
        _, ent, mp = orc.analyze(msg, word_size=ws)
        case["mapping"] = [int(x) for x in mp]
        blob = orc.encode(msg, cfg=orc.config(word_size=ws), bandwidth=10.0)
        assert blob[:4] == b"DTDT", case["name"]
        if ref is not None:
            rblob = ref.encode(msg, sample_fraction=1.0, word_size=ws, bandwidth=10.0)
            case["ref_mapping"] = list(struct.unpack_from("<%di" % ws, rblob, 20))
            if rblob != blob:
                print("ORACLE != REFERENCE:", case["name"], case["mapping"], case["ref_mapping"])
                case["oracle_differs"] = True
        return ent

    for ws in mb.WIDTHS:
        for ci, size in enumerate(mb.sizes_for(ws)):
            n = size // ws
            assert n * ws == size
            rng = np.random.default_rng([SEED, ws, size])
            mul = mb.multipliers(n, ws)
            cell = []
            # ---- near ties
            js = mb.j_values(ws)
            spec = mb.SPECULATED.get(ws) if size > 65536 else None
            turn = ci  # the j of the next unforced case
            for k in range(8 if ws > 1 else 0):
                band, sign = k // 2, mb.SIGNS[k % 2]
                forced = None
                if spec is not None and (band, sign) in ((1, "+"), (2, "-")):
                    forced = [b for b in range(ws) if spec[b] == (1 if sign == "+" else 0)]
                k256 = ci == 5 and band == 3 and sign == "-" and n >= 512
                order = [js[(turn + t) % len(js)] for t in range(len(js))] if forced is None else [len(forced)]
                turn += forced is None
                found = None
                for t, j in enumerate(order):
                    scale = ws / min(j, ws - j)
                    lo, hi = windows[band][0] * scale, windows[band][1] * scale
                    if sign == "-":
                        lo, hi = -hi, -lo
                    for _ in range(DRAWS):
                        syms, counts = draw_hist(rng, n, "any", k256)
                        moves = find_moves(rng, counts, n, lo, hi)
                        if moves is None:
                            continue
                        start = (5 * k + ci) % ws
                        pert = forced
                        while pert is None:
                            pert = sorted((start + i) % ws for i in range(j))
                            if [int((b in pert) == (sign == "+")) for b in range(ws)] == spec:
                                pert, start = None, start + 1  # only the forced cases speculate right
                        case = dict(name="ws%d_n%d_b%d%s" % (ws, size, band, sign), ws=ws, size=size, kind="near",
                                    band=band, sign=sign, j=j, sym=syms, counts=counts, moves=moves,
                                    perturbed=pert, mul=mul)
                        ent = finish(case)
                        if mb.classify(case, ent, M) == (band, sign):  # the oracle's entropies decide
                            found = case
                            break
                    if found:
                        fallbacks += t > 0
                        break
                assert found, "unreachable: ws %d size %d band %d sign %s" % (ws, size, band, sign)
                if spec is not None and band in (1, 2):
                    assert (found["mapping"] == spec) == (forced is not None), found["name"]
                cell.append(found)
            if ws > 1:
                assert {c["j"] for c in cell} >= set(js), (ws, size, [c["j"] for c in cell])
            # ---- near ties between unrelated histograms
            rng2 = np.random.default_rng([SEED, ws, size, 1])
            for k, (band, sign) in enumerate((b, s) for b in mb.INDEP_BANDS for s in mb.SIGNS) if ws > 1 else ():
                j = js[(ci + k) % len(js)]
                scale = ws / min(j, ws - j)
                lo, hi = windows[band][0] * scale, windows[band][1] * scale
                if sign == "-":
                    lo, hi = -hi, -lo
                deep = band == 0  # as near a tie as three moves reach: down to M / 65536
                if deep:
                    lo, hi = (M / 65536 * scale, hi) if sign == "+" else (lo, -M / 65536 * scale)
                found, best, tried = None, None, 0
                for _ in range(DRAWS):
                    syms, counts = draw_hist(rng2, n, "any")
                    alt = find_indep(rng2, n, counts, lo, hi, deep)
                    if alt is None:
                        continue
                    start = (3 * k + ci + 1) % ws
                    case = dict(name="ws%d_n%d_indep_b%d%s" % (ws, size, band, sign), ws=ws, size=size, kind="indep",
                                band=band, sign=sign, j=j, sym=syms, counts=counts, moves=[],
                                alt_sym=alt[0], alt_counts=alt[1],
                                perturbed=sorted((start + i) % ws for i in range(j)), mul=mul)
                    ent = finish(case)
                    if mb.classify(case, ent, M) != (band, sign):
                        continue
                    gap = min(abs(d) for d in mb.deviations(ent))
                    if best is None or gap < best:
                        found, best = case, gap
                    tried += 1
                    if not deep or tried == DEEP_DRAWS:
                        break
                if deep and found:
                    deepest.append(float(best))
                assert found, "unreachable: ws %d size %d indep band %d sign %s" % (ws, size, band, sign)
                cell.append(found)
            # ---- exact ties
            ties = []

            def tie(kind, family):
                for _ in range(1000):
                    h = draw_hist(rng, n, kind)
                    if h is not None:
                        break
                else:
                    raise AssertionError("no %s histogram for %d words" % (kind, n))
                case = dict(name="ws%d_n%d_tie_%s" % (ws, size, family), ws=ws, size=size, kind="tie", tie=family,
                            sym=h[0], counts=h[1], moves=[], perturbed=[], mul=mul)
                ent = finish(case)
                assert len({float(e) for e in ent}) == 1 and len(set(case["mapping"])) == 1, case["name"]
                return case

            for kind in mb.tie_kinds(n):
                ties.append(tie(kind, kind))
            if ws in BOTH_OUTCOMES:
                kinds = [x for x in mb.tie_kinds(n) if x != "const"] + ["any"]
                for d in range(64):
                    have = {c["mapping"][0] for c in ties}
                    if have == {0, 1}:
                        break
                    c = tie(kinds[d % len(kinds)], "extra")
                    if c["mapping"][0] not in have:
                        ties.append(c)
            outcomes["ws%d_n%d" % (ws, size)] = sorted({c["mapping"][0] for c in ties})
            cases += cell + ties
            print("ws %2d size %6d: %d near, %d ties, outcomes %s" % (ws, size, len(cell), len(ties),
                                                                     outcomes["ws%d_n%d" % (ws, size)]), flush=True)

    for w in (8, 16):
        for size in mb.sizes_for(w):
            assert outcomes["ws%d_n%d" % (w, size)] == [0, 1], (w, size)
    head = dict(generator="tests/golden/make_mapping_bands.py", margin=M,
                margin_source="kFastMargin, psyne_amd/csrc/tdt_encode.h",
                alphabet="symbol i of a histogram is (a * i + b) mod 256, sym = [a, b]",
                shuffle="column b is the sorted symbols permuted by i -> i * mul mod N, mul = multipliers(N, ws)[b] "
                        "(tests/mapping_band_cases.py)",
                reference=("include/psyne/protocol/tdt_compression.hpp via oracle/_ref/libtdt_ref.so"
                           if ref is not None else None),
                bands=list(mb.BAND_NAMES), tie_outcomes=outcomes,
                crc32=zlib.crc32(b"".join(c["_crc"].to_bytes(4, "little") for c in cases)))
    cells = {}
    for c in cases:
        cells.setdefault((c["ws"], c["size"]), []).append(mb.compact(c))
    lines = ["{"] + ['"%s": %s,' % (k, json.dumps(v)) for k, v in head.items()] + ['"cells": [']
    lines += [json.dumps(dict(ws=k[0], size=k[1], cases=v), separators=(",", ":")) + ("," if i + 1 < len(cells) else "")
              for i, (k, v) in enumerate(cells.items())]  # one (width, size) cell per line
    lines += ["]", "}"]
    mb.FIXTURE.write_text("\n".join(lines) + "\n")
    json.loads(mb.FIXTURE.read_text())
    print("cases", len(cases), "bytes", mb.FIXTURE.stat().st_size, "j fallbacks", fallbacks,
          "message bytes", sum(c["size"] for c in cases))
    q = np.quantile(deepest, [0, 0.5, 1]) / M
    print("deep near ties: smallest gap min %.2e M, median %.2e M, max %.2e M" % tuple(q))


if __name__ == "__main__":
    main()
