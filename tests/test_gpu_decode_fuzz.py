"""Differential decode on the GPU: the crafted blobs of tests/decode_cases.py (every width, any
number of streams, mappings of any shape, short / long / count-0 / odd-byte streams, sizes on both
sides of every decode threshold, and cut or patched blobs) through every decode route of the C ABI,
status for status and byte for byte against the CPU oracle (pinned in tests/golden/decode_fuzz.json,
tests/test_decode_fuzz.py).

In every route the outputs lie between 0xA5 guard bytes that must stay intact, the inputs end with
4 KiB of 0xFF (a read past a blob shows as a wrong status or wrong bytes), and the codec's device
invariant flags must stay 0.  One test per route; each collects every mismatch and reports the
first few by case name."""
import json
import struct

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import decode_cases as dc
from tests.golden_cases import GOLDEN
from tests.support import E_CAPACITY, report

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, i64, make_codec  # noqa: E402, F401
from tests.decode_check import (Expect, FILL, GUARD, TAIL, check_sizes, compare, guarded_output,  # noqa: E402
                                packed_input, run_slotted)

pytestmark = pytest.mark.gpu


def build_batch(cases):
    """The cases with the oracle's result, valid and malformed interleaved."""
    orc = Oracle()
    lib_status = {r["name"]: r["lib_status"] for r in json.loads((GOLDEN / "decode_fuzz.json").read_text())["cases"]
                  if "lib_status" in r}
    exp = []
    for c in cases:
        st, out = orc.decode(c.blob)
        if c.name in lib_status:  # a word size above the library's bound: reported, nothing decoded
            st, out = lib_status[c.name], b""
        assert (st == 0) == (c.family != "malformed") or c.name in lib_status, c.name
        exp.append(Expect(c, st, out if st == 0 else b""))
    good = [e for e in exp if e.family != "malformed"]
    bad = [e for e in exp if e.family == "malformed"]
    keyed = [(i / len(good), 0, e) for i, e in enumerate(good)] + [((i + 0.5) / len(bad), 1, e) for i, e in enumerate(bad)]
    return [e for _, _, e in sorted(keyed, key=lambda t: t[:2])]


@pytest.fixture(scope="module")
def batch():
    return build_batch(dc.all_cases())  # (the oracle runs once for every route)


# ------------------------------------------------------------------ a, b: slotted, two thresholds


def test_route_a_slotted(batch):
    bad = []
    codec = make_codec()
    for in_phase, out_phase in ((0, 0), (5, 9)):
        run_slotted(codec, batch, in_phase, out_phase, "slotted(%d,%d)" % (in_phase, out_phase), bad)
        check_sizes(codec, batch, in_phase, bad)
    assert codec.error_flags() == 0
    report(bad)


def test_route_b_slotted_large_passes(batch):
    """TDT_OPT_LARGE_MIN = 16,384: blobs decoding to 20,000 bytes and more take the large-blob
    passes (fast shapes by 32 KiB tiles, other shapes whole in the prep pass, generic widths deferred
    from there); the same bytes as with the default threshold, and the oracle's."""
    from psyne_amd._lib import TDT_OPT_LARGE_MIN
    bad = []
    plain = make_codec()
    base, bst, bln = run_slotted(plain, batch, 0, 0, "slotted", bad)
    codec = make_codec()
    codec.set_option(TDT_OPT_LARGE_MIN, 16384)
    for in_phase, out_phase in ((0, 0), (5, 9)):
        got, st, ln = run_slotted(codec, batch, in_phase, out_phase, "large(%d,%d)" % (in_phase, out_phase), bad)
        if not (np.array_equal(got, base) and np.array_equal(st, bst) and np.array_equal(ln, bln)):
            bad.append("large(%d,%d): differs from the default threshold's result" % (in_phase, out_phase))
    assert codec.error_flags() == 0 and plain.error_flags() == 0
    report(bad)


# ------------------------------------------------------------------ c: compacted
@pytest.mark.parametrize("path", ["two_phase", "lookback"])
def test_route_c_compacted(batch, path):
    from psyne_amd._lib import TDT_OPT_NO_TWO_PHASE
    bad = []
    n = len(batch)
    codec = make_codec()
    codec.set_option(TDT_OPT_NO_TWO_PHASE, 1 if path == "lookback" else 0)
    want_off = np.concatenate([[0], np.cumsum([e.size for e in batch])]).astype(np.int64)
    for in_phase, out_phase in ((0, 0), (3, 7)):
        d, o, _ = packed_input(batch, in_phase)
        whole, out, lead = guarded_output(int(want_off[-1]), out_phase)
        _, doff, st = codec.decode_batch(d, o, out=out)
        torch.cuda.synchronize()
        h, doff, st = whole.cpu().numpy(), doff.cpu().numpy(), st.cpu().numpy()[:n]
        tag = "%s(%d,%d)" % (path, in_phase, out_phase)
        if not np.array_equal(doff, want_off):
            k = int(np.flatnonzero(doff != want_off)[0])
            bad.append("%s: offsets differ from entry %d (%s)" % (tag, k, batch[max(k - 1, 0)].name))
            continue
        compare(batch, st, None, lambda i: h[lead + want_off[i]:lead + want_off[i + 1]], bad, tag)
        if not ((h[:lead] == GUARD).all() and (h[lead + want_off[-1]:] == GUARD).all()):
            bad.append("%s: wrote outside the output buffer" % tag)
    assert codec.error_flags() == 0
    report(bad)


# ------------------------------------------------------------------ d: scattered


def scatter(batch):
    """Every blob in an allocation of its own at byte phase 0..3 (0xFF behind it), the batch in a
    shuffled order, so the pointer table is in no address order."""
    order = [int(i) for i in np.random.default_rng(4242).permutation(len(batch))]
    exp = [batch[i] for i in order]
    blobs = []
    for k, e in enumerate(exp):
        t = torch.full((k % 4 + len(e.blob) + TAIL,), FILL, dtype=torch.uint8, device="cuda")
        v = t[k % 4:k % 4 + len(e.blob)]
        if e.blob:
            v.copy_(torch.from_numpy(np.frombuffer(e.blob, np.uint8).copy()))
        blobs.append((t, v))
    return exp, blobs


@pytest.fixture(scope="module")
def scattered(batch):
    return scatter(batch)


def run_scattered(exp, blobs, short, tag, bad):
    caps = [(e.size if e.status == 0 else 16) - (1 if i in short else 0) for i, e in enumerate(exp)]
    outs = [torch.full((64 + c + 64,), GUARD, dtype=torch.uint8, device="cuda") for c in caps]
    codec = make_codec()
    ln, st = codec.decode_v(i64(v.data_ptr() for _, v in blobs), i64(len(e.blob) for e in exp),
                            i64(t.data_ptr() + 64 for t in outs), i64(caps))
    torch.cuda.synchronize()
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    for i, e in enumerate(exp):
        h = outs[i].cpu().numpy()
        if i in short:
            if (st[i], ln[i]) != (E_CAPACITY, 0) or not (h == GUARD).all():
                bad.append("%s %s: one byte short gave status %d, length %d" % (tag, e.name, st[i], ln[i]))
            continue
        if not ((h[:64] == GUARD).all() and (h[64 + caps[i]:] == GUARD).all()):
            bad.append("%s %s: wrote outside its allocation's %d bytes" % (tag, e.name, caps[i]))
        if (st[i], ln[i]) != (e.status, e.size):
            bad.append("%s %s: status %d length %d, expected %d and %d" % (tag, e.name, st[i], ln[i], e.status, e.size))
        elif e.status == 0 and h[64:64 + e.size].tobytes() != e.out:
            bad.append("%s %s: bytes differ" % (tag, e.name))
        elif e.status != 0 and not (h == GUARD).all():
            bad.append("%s %s: an error blob's output was written" % (tag, e.name))
    assert codec.error_flags() == 0


def shape_of(e):
    orig, ns, ws, _, mapping, _ = dc.parse(e.blob)
    return orig, ws in dc.TUNED, dc.takes_fast_path(ws, mapping, ns)


def test_route_d_scattered(scattered):
    exp, blobs = scattered
    bad = []
    run_scattered(exp, blobs, (), "scattered", bad)
    codec = make_codec()
    sz, st = codec.decoded_sizes_v(i64(v.data_ptr() for _, v in blobs), i64(len(e.blob) for e in exp))
    torch.cuda.synchronize()
    sz, st = sz.cpu().numpy(), st.cpu().numpy()
    for i, e in enumerate(exp):
        if (sz[i], st[i]) != (e.size, e.status):
            bad.append("sizes_v %s: size %d status %d" % (e.name, sz[i], st[i]))
    assert codec.error_flags() == 0
    report(bad)


def test_route_d_scattered_short_capacity(scattered):
    """Three blobs get a capacity one byte short — a small-list one and a main-list one on
    decode_one's generic path, and one of a generic width: TDT_E_CAPACITY, length 0 and an
    untouched output for them, the rest exact."""
    exp, blobs = scattered
    valid = [(i, shape_of(e)) for i, e in enumerate(exp) if e.status == 0 and e.family != "malformed"]
    short = (next(i for i, (orig, tuned, fast) in valid if tuned and not fast and 1024 < orig <= 8192),
             next(i for i, (orig, tuned, fast) in valid if tuned and not fast and 20000 <= orig <= 70001),
             next(i for i, (orig, tuned, fast) in valid if not tuned and orig >= 5000))
    bad = []
    run_scattered(exp, blobs, short, "short", bad)
    report(bad)


# ------------------------------------------------------------------ e: one blob per host call
def test_route_e_host_one_blob_per_call(batch):
    """tdt_decode_host with one blob: the one-wave kernel up to 4 KiB, above it
    tdt_decode_one_kernel, which decodes fast shapes by tiles and hands every other shape (and every
    malformed blob) to wave 0's decode_one.  Every tuned-width case up to 70,001 bytes.  The generic
    widths go as one batch through the pipeline, as tests/test_gpu_anyws.py::test_host_paths does."""
    from psyne_amd._lib import check
    codec = make_codec()
    lib, h = codec._lib, codec._h
    bad = []
    sub = [e for e in batch if e.ws in dc.TUNED and (e.status != 0 or e.size <= 70001)]
    assert len(sub) >= 100
    for e in sub:
        src = np.full(len(e.blob) + TAIL, FILL, np.uint8)
        src[: len(e.blob)] = np.frombuffer(e.blob, np.uint8)
        # (the host path refuses a call whose capacity is below the header's original_size, and the
        # pipeline, which takes the blobs whose header names no tuned width, may leave scratch bytes
        # inside the capacity past the length it reports: the guards stand around the capacity)
        cap = e.size if e.status == 0 else max(5000, struct.unpack_from("<I", e.blob, 4)[0] if len(e.blob) >= 8 else 0)
        out = np.full(64 + cap + 64, GUARD, np.uint8)
        off = np.array([0, len(e.blob)], np.uint64)
        ooff = np.zeros(2, np.uint64)
        st = np.full(1, -1, np.int32)
        check(lib.tdt_decode_host(h, src.ctypes.data, off.ctypes.data, 1, out.ctypes.data + 64, cap, ooff.ctypes.data,
                                  st.ctypes.data))
        compare([e], st, [int(ooff[1])], lambda i: out[64:] if e.status == 0 else out[64 + cap:], bad, "host")
        if not (out[:64] == GUARD).all():
            bad.append("host %s: wrote before its output" % e.name)
    gen = [e for e in batch if e.ws in dc.GENERIC and e.status == 0 and e.family != "malformed" and e.size <= 70001]
    data = np.frombuffer(b"".join(e.blob for e in gen), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(e.blob) for e in gen])]).astype(np.uint64)
    want_off = np.concatenate([[0], np.cumsum([e.size for e in gen])]).astype(np.uint64)
    dec, doff, st = codec.decode_host(data, off, int(want_off[-1]))
    if not np.array_equal(doff, want_off):
        bad.append("host batch: output offsets differ")
    else:
        compare(gen, st, None, lambda i: dec[int(want_off[i]):int(want_off[i + 1])], bad, "host batch")
    assert codec.error_flags() == 0
    report(bad)
