"""The run-structured encode cases (tests/encode_run_cases.py) against their pinned record
(tests/golden/encode_runs.json, written by tests/golden/make_encode_runs.py where the compiled
reference exists): the generator still builds the recorded messages, the CPU oracle still gives the
recorded blobs, a plain numpy run-length encoder agrees with it, the encode emulator
(tools/emulate_encode.py) agrees with it on the new edges, and the cap-exclusion rule of pass A1,
restated for every tuned width and stream split, implies what the kernel relies on.  Pins the
yardstick the GPU tests of those messages (tests/test_gpu_encode_runs.py) compare with."""
import json
import struct

import numpy as np
import pytest

from oracle.oracle import Oracle, Reference
from tests import encode_run_cases as ec
from tests.golden_cases import GOLDEN
from tests.support import digest


@pytest.fixture(scope="module")
def meta():
    return json.loads((GOLDEN / "encode_runs.json").read_text())


@pytest.fixture(scope="module")
def cases(meta):
    return [c for c in ec.all_cases() if c.name not in meta["dropped"]]


@pytest.fixture(scope="module")
def blobs(cases):
    """name -> the oracle's blob, computed once."""
    orc = Oracle()
    return {c.name: orc.encode(c.message, cfg=orc.config(word_size=c.ws, sample_fraction=1.0), bandwidth=10.0)
            for c in cases}


def test_generator_reproduces_every_message(meta, cases):
    record = meta["cases"]
    assert meta["seed"] == ec.SEED
    assert [c.name for c in cases] == [r["name"] for r in record]
    for c, r in zip(cases, record):
        got = (c.ws, "".join(str(m) for m in c.mapping), c.n, c.family, digest(c.message.tobytes()))
        assert got == (r["ws"], r["mapping"], r["n"], r["family"], r["message"]), c.name
        assert c.message.size == c.n
    # the premise cap of the pin script: at most 2 % of a width's cases dropped, each by name
    names = {c.name for c in ec.all_cases()}
    assert set(meta["dropped"]) <= names
    for ws in ec.TUNED + ec.GENERIC:
        total = sum(1 for c in ec.all_cases() if c.ws == ws)
        assert total - sum(1 for c in cases if c.ws == ws) <= 0.02 * total, ws


def test_oracle_reproduces_every_blob(meta, cases, blobs):
    for c, r in zip(cases, meta["cases"]):
        b = blobs[c.name]
        assert b[:4] == b"DTDT" and digest(b) == r["blob"], c.name
        assert tuple(np.frombuffer(b[20:20 + 4 * c.ws], np.int32)) == c.mapping, c.name


def test_coverage(cases):
    ec.check_coverage(cases)
    assert 800 <= len(cases) <= 1100
    # every edge has exactly its length: a run of L bytes appears in its stream
    by_name = {c.name: c for c in cases}
    for name in ("ws4_m0011_n8192_v2", "ws16_m0111111111111111_n32784_v1", "ws1_m0_n4112_v0"):
        c = by_name[name]
        for s in range(len(ec.shares(c.ws, c.mapping))):
            runs = set(run_lengths(stream(c.message, c.ws, c.mapping, s)).tolist())
            assert {L for st, _, _, _, L, _ in ec.EDGES[name] if st == s} <= runs, (name, s)


# ------------------------------------------------------------------ plain numpy encoder
def stream(msg, ws, mapping, c):
    """separate_byte_streams (reference :527-549): the positions mapped to c, word-major."""
    return msg.reshape(-1, ws)[:, [b for b in range(ws) if mapping[b] == c]].reshape(-1)


def run_starts(s):
    return np.concatenate([[0], np.flatnonzero(np.diff(s)) + 1])


def run_lengths(s):
    return np.diff(np.append(run_starts(s), s.size))


def numpy_encode(msg, ws, mapping) -> bytes:
    """serialize (:81-117) of simple_rle_compress (:557-582) per stream: a run of L bytes is
    ceil(L / 255) pairs, all of count 255 but the last."""
    ns = max(mapping) + 1
    out = [struct.pack("<5I", 0x54445444, msg.size, ns, ws, ws), np.asarray(mapping, "<i4").tobytes()]
    for c in range(ns):
        s = stream(msg, ws, mapping, c)
        starts = run_starts(s)
        lens = run_lengths(s)
        chunks = -(-lens // 255)
        pairs = np.empty((int(chunks.sum()), 2), np.uint8)
        pairs[:, 0] = 255
        pairs[np.cumsum(chunks) - 1, 0] = lens - 255 * (chunks - 1)
        pairs[:, 1] = np.repeat(s[starts], chunks)
        out += [struct.pack("<I", pairs.size), pairs.tobytes()]
    return b"".join(out)


def test_numpy_encoder_equals_oracle(cases, blobs):
    for c in cases:
        assert numpy_encode(c.message, c.ws, c.mapping) == blobs[c.name], c.name


@pytest.mark.skipif(not Reference.available(), reason="oracle/_ref not built (needs the reference at build time)")
def test_reference_equals_oracle(cases, blobs):
    ref = Reference()
    for c in cases:
        assert ref.encode(c.message, sample_fraction=1.0, word_size=c.ws, bandwidth=10.0) == blobs[c.name], c.name


# ------------------------------------------------------------------ the emulator on the new edges
def test_emulator_equals_oracle(cases, blobs):
    """Every tuned-width edge case of at most 8,192 bytes, at team 64 and 256 (RW up to 8 and 2).
    Sampled by variant to stay near 10 s: variant 0 (bookends) and 2 (none); no width, mapping or
    size is left out."""
    from tools.emulate_encode import encode
    n = 0
    for c in cases:
        if c.family != "edge" or c.n > 8192 or c.name.endswith("_v1"):
            continue
        for team in (64, 256):
            assert encode(c.message.tobytes(), list(c.mapping), ws=c.ws, team=team) == blobs[c.name], (c.name, team)
        n += 1
    assert n == 2 * 4 * sum(len(ec.mappings(ws)) for ws in ec.TUNED)


# ------------------------------------------------------------------ the cap-exclusion rule, every width
def clean(msg, ws, mapping) -> bool:
    """Pass A1's rule (psyne_amd/csrc/tdt_encode.h, "pass A1: run starts"; tests/test_cap_exclusion.py
    has it for word size 4): groups of 16 bytes, Ls = (16 / ws) k slots of stream c per group; the
    255-cap is ruled out when, in every stream, every aligned block of B groups (B = 8, or 4 where
    Ls = 16) holds a run start or reaches past the message's last group."""
    ngroups = (msg.size + 15) // 16
    for c in range(max(mapping) + 1):
        ls = (16 // ws) * sum(1 for m in mapping if m == c)
        blk = 4 if ls == 16 else 8
        has = np.zeros(ngroups, bool)
        has[run_starts(stream(msg, ws, mapping, c)) // ls] = True
        nblk = (ngroups + blk - 1) // blk
        padded = np.ones(nblk * blk, bool)  # groups past the end count as starts
        padded[:ngroups] = has
        if not padded.reshape(nblk, blk).any(axis=1).all():
            return False
    return True


def max_run(msg, ws, mapping) -> int:
    return max(int(run_lengths(stream(msg, ws, mapping, c)).max()) for c in range(max(mapping) + 1))


def adversarial(rng, ws, mapping, n_words, mean_run):
    """Words whose streams change value after geometric runs of mean `mean_run` bytes."""
    streams = []
    for k in ec.shares(ws, mapping):
        runs = rng.geometric(1.0 / mean_run, n_words * k)
        vals = np.cumsum(rng.integers(1, 256, runs.size)).astype(np.uint8)
        streams.append(np.repeat(vals, runs)[: n_words * k])
    return ec.assemble(ws, mapping, streams)


@pytest.mark.parametrize("ws", ec.TUNED)
def test_clean_implies_no_capped_run(cases, ws):
    seen = {True: 0, False: 0}
    for c in cases:
        if c.ws != ws or not c.family.startswith("capex_"):
            continue
        is_clean, longest = clean(c.message, ws, c.mapping), max_run(c.message, ws, c.mapping)
        seen[is_clean] += 1
        assert not is_clean or longest <= 255, c.name
        # the three outcomes are what the generator says they are
        want = {"capex_clean": (True, False), "capex_dirty": (False, False), "capex_256": (False, True)}[c.family]
        assert (is_clean, longest >= 256) == want, (c.name, is_clean, longest)
        if c.family == "capex_256":
            assert 256 in run_lengths(stream(c.message, ws, c.mapping, int(c.name.split("_s")[1][0]))), c.name
    assert seen[True] and seen[False], (ws, seen)
    # every edge case too: clean ones hold no capped run
    for c in cases:
        if c.ws == ws and c.family == "edge" and clean(c.message, ws, c.mapping):
            assert max_run(c.message, ws, c.mapping) <= 255, c.name
    # seeded adversarial runs around Zr = floor(255 / Ls) - 1 groups, for every stream split
    rng = np.random.default_rng([ec.SEED, 0xAD, ws])
    adv = {True: 0, False: 0}
    for mapping in ec.mappings(ws):
        for trial in range(360 // len(ec.mappings(ws))):
            mean_run = [2, 8, 20, 40, 64, 100, 130, 200][trial % 8]
            msg = adversarial(rng, ws, mapping, int(rng.integers(64, 6000)) * 16 // ws, mean_run)
            is_clean = clean(msg, ws, mapping)
            adv[is_clean] += 1
            assert not is_clean or max_run(msg, ws, mapping) <= 255, (ws, mapping, trial)
    assert adv[True] > 10 and adv[False] > 10, (ws, adv)
