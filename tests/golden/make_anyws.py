#!/usr/bin/env python3
"""Generate the generic-word-size fixtures in tests/golden/ from the REFERENCE codec.

Run where the compiled reference exists (after `make -C oracle`):

    python tests/golden/make_anyws.py

Word sizes 3, 5, 6, 7, 12, 24, 32, 40 and 64 — widths the tuned kernels do not take — at
sample_fraction = 1.0, through oracle.oracle.Reference.  Same layout as golden.npz / cases.json:

    anyws.npz          inputs / outputs byte blobs (uint8), compressed
    anyws_cases.json   one record per case: op, config, slices into the blobs, expected status

Case families:
  * constructed   a message built from chosen stream contents: positions b % 3 == 0 are uniform
                  random (the high-entropy stream), the others are filled in word order from one
                  sequence — runs of 254, 255, 256, 509, 510, 511, 1, 765 and 1 bytes of distinct
                  values, then a two-value pattern repeating every 300 bytes.  The generator
                  asserts that the analysis gives exactly that mapping.
  * same          every byte the same value: all entropies 0, num_streams = 1
  * equal         every position carries the same random sequence: equal entropies, so the
                  mapping hangs on the rounding of sum / ws (all 0, or all 1 with an empty stream 0)
  * uniform       uniform random bytes
  * uncp          ws = 12: 1028 bytes (n % 4 == 0, n % ws != 0) and 1020 bytes (< min_tensor_size)
  * decode        crafted blobs: four streams, a short stream, an odd trailing byte, count-0
                  pairs, original_size not a multiple of ws ("ref": "ran": the reference decoded
                  it); a truncated stream, a mapping entry >= num_streams ("ref": "ub": undefined
                  in the reference, the status is the specification's, from the oracle); and a
                  ws = 65 blob, valid for the reference and the oracle ("status"), above the
                  library's bound ("lib_status" = TDT_E_UNSUPPORTED).
"""
from __future__ import annotations

import json
import pathlib
import struct
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle.oracle import Oracle, Reference  # noqa: E402

OUTDIR = pathlib.Path(__file__).resolve().parent
TDT = 0x54445444
WIDTHS = (3, 5, 6, 7, 12, 24, 32, 40, 64)
RUNS = (254, 255, 256, 509, 510, 511, 1, 765, 1)
E_UNSUPPORTED = 6


def low_stream(length: int, rng) -> np.ndarray:
    """RUNS of distinct values, then a two-value pattern with period 300 (200 + 100)."""
    vals = rng.permutation(200)[: len(RUNS) + 2] + 1
    parts = [np.full(r, vals[i], np.uint8) for i, r in enumerate(RUNS)]
    s = np.concatenate(parts)
    period = np.concatenate([np.full(200, vals[-2], np.uint8), np.full(100, vals[-1], np.uint8)])
    reps = (max(length - s.size, 0) + 299) // 300
    s = np.concatenate([s] + [period] * reps)
    assert s.size >= length
    return s[:length]


def constructed(ws: int, rng, min_low: int = sum(RUNS) + 600, low=None, wc=None) -> tuple[np.ndarray, list[int]]:
    mapping = [1 if b % 3 == 0 else 0 for b in range(ws)]
    k_low = mapping.count(0)
    if wc is None:
        wc = max((min_low + k_low - 1) // k_low, (1024 + ws - 1) // ws)
        wc = (wc + 3) // 4 * 4
    msg = np.zeros((wc, ws), np.uint8)
    lo = [b for b in range(ws) if mapping[b] == 0]
    hi = [b for b in range(ws) if mapping[b] == 1]
    msg[:, hi] = rng.integers(0, 256, (wc, len(hi)), dtype=np.uint8)
    seq = low_stream(wc * k_low, rng) if low is None else low
    msg[:, lo] = seq[: wc * k_low].reshape(wc, k_low)
    return msg.reshape(-1), mapping


def blob(orig, ws, mapping, streams, ns=None, msize=None):
    ns = len(streams) if ns is None else ns
    msize = len(mapping) if msize is None else msize
    b = struct.pack("<IIIII", TDT, orig & 0xFFFFFFFF, ns, ws & 0xFFFFFFFF, msize)
    b += b"".join(struct.pack("<i", m) for m in mapping)
    for s in streams:
        b += struct.pack("<I", len(s)) + bytes(s)
    return b


def pairs(*pv):
    return bytes(x for p in pv for x in p)


class Store:
    def __init__(self):
        self.inp, self.out, self.cases = bytearray(), bytearray(), []

    def add(self, rec, inp: bytes, out: bytes | None):
        rec["in"] = [len(self.inp), len(self.inp) + len(inp)]
        self.inp += inp
        if out is not None:
            rec["out"] = [len(self.out), len(self.out) + len(out)]
            self.out += out
        self.cases.append(rec)


def main():
    ref, orc = Reference(), Oracle()
    rng = np.random.default_rng(0xA11C0DE)
    st = Store()

    def enc(name, data: np.ndarray, ws, family, mapping=None):
        d = data.tobytes()
        out = ref.encode(d, sample_fraction=1.0, word_size=ws, bandwidth=10.0)
        assert out == orc.encode(d, cfg=orc.config(word_size=ws), bandwidth=10.0), name
        rec = dict(name=name, op="encode", family=family, ws=ws, sample_fraction=1.0, bandwidth=10.0, cpu=0.5,
                   min_tensor=1024, status=0, ref="ran")
        if mapping is not None:
            rec["mapping"] = mapping
        st.add(rec, d, out)
        s, back, _ = ref.decode(out, cap=len(d) + 16)
        assert s == 0 and back == d, name

    for ws in WIDTHS:
        msg, mapping = constructed(ws, rng)
        _, _, mp = orc.analyze(msg, word_size=ws)
        assert list(mp) == mapping, (ws, list(mp))
        assert msg.size >= 1024 and (msg.size // ws) % 4 == 0
        enc("constructed_ws%d" % ws, msg, ws, "constructed", mapping)
        wc = (1024 + ws - 1) // ws
        wc = (wc + 3) // 4 * 4
        enc("same_ws%d" % ws, np.full(wc * ws, int(rng.integers(1, 256)), np.uint8), ws, "same")
        assert struct.unpack_from("<I", bytes(st.out[st.cases[-1]["out"][0]:]), 8)[0] == 1  # num_streams
        enc("equal_ws%d" % ws, np.repeat(rng.integers(0, 256, wc, dtype=np.uint8), ws), ws, "equal")
        enc("uniform_ws%d" % ws, rng.integers(0, 256, wc * ws, dtype=np.uint8), ws, "uniform")
    enc("uncp_ws12_1028", rng.integers(0, 256, 1028, dtype=np.uint8), 12, "uncp")
    enc("uncp_ws12_1020", rng.integers(0, 256, 1020, dtype=np.uint8), 12, "uncp")

    # ---- decode-only blobs
    def dec(name, b: bytes, ws, defined=True, lib_status=None):
        os_, oout = orc.decode(b)
        rec = dict(name=name, op="decode", family="decode", ws=ws, status=os_, ref="ran" if defined else "ub")
        if lib_status is not None:
            rec["lib_status"] = lib_status
        if defined:
            s, out, _ = ref.decode(b, cap=1 << 16)
            assert s == os_ == 0 and out == oout, name
        st.add(rec, b, oout if os_ == 0 else None)

    m12, _ = constructed(12, rng, wc=96, low=low_stream(96 * 8, rng))
    four = orc.encode(m12[:96 * 12], cfg=orc.config(word_size=12, min_tensor_size=0), bandwidth=10.0,
                      mapping=[0, 1, 2, 0, 1, 2, 3, 3, 3, 0, 1, 2])
    dec("four_streams_ws12", four, 12)
    # 4 words of ws = 12, mapping alternating: streams of 24 bytes each
    alt = [0, 1] * 6
    dec("short_stream_ws12", blob(48, 12, alt, [pairs((10, 0xAA)), pairs((24, 0xBB))]), 12)
    dec("odd_trailing_byte_ws12", blob(48, 12, alt, [pairs((20, 7), (4, 9)) + b"\x05", pairs((24, 4)) + b"\x11"]), 12)
    dec("count_zero_pairs_ws12", blob(48, 12, alt, [pairs((0, 5), (12, 6), (0, 7), (12, 8)),
                                                   pairs((0, 1), (6, 2), (0, 3), (18, 4))]), 12)
    dec("orig_tail_bytes_ws12", blob(55, 12, alt, [pairs((24, 0x10)), pairs((20, 0x20), (4, 0x30))]), 12)
    dec("orig_tail_bytes_ws7", blob(40, 7, [0, 1, 1, 0, 2, 2, 0], [pairs((15, 1)), pairs((3, 2), (7, 3)), pairs((9, 4))]), 7)
    good = blob(48, 12, alt, [pairs((24, 1)), pairs((24, 2))])
    dec("truncated_stream_ws12", good[:-2], 12, defined=False)
    dec("mapping_range_ws12", blob(48, 12, [0, 1] * 5 + [2, 1], [pairs((24, 1)), pairs((24, 2))]), 12, defined=False)
    dec("ws65", blob(130, 65, [0] * 65, [pairs((130, 0x42))]), 65, lib_status=E_UNSUPPORTED)

    np.savez_compressed(OUTDIR / "anyws.npz", inputs=np.frombuffer(bytes(st.inp), np.uint8),
                        outputs=np.frombuffer(bytes(st.out), np.uint8))
    (OUTDIR / "anyws_cases.json").write_text(json.dumps(dict(
        generator="tests/golden/make_anyws.py",
        reference="include/psyne/protocol/tdt_compression.hpp via oracle/_ref/libtdt_ref.so",
        cases=st.cases), indent=0))
    print("cases", len(st.cases), "inputs", len(st.inp), "outputs", len(st.out))


if __name__ == "__main__":
    main()
