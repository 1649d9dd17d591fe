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

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD, FILL, TAIL, GAP = 0xA5, 0xFF, 4096, 16
E_CAPACITY = 5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from psyne_amd import _lib
    _lib.load()


class Expect:
    """One case with what the library must report: status, decoded length, bytes."""

    def __init__(self, case, status, out):
        self.name, self.ws, self.family, self.blob = case
        self.status, self.out = status, out
        self.size = len(out)


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


def make_codec():
    from psyne_amd import TDTConfig, TdtCodec
    c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=4))  # (the generic widths: the deferred list)
    c.set_metrics(10.0, 1.0, 0.5)
    return c


def report(bad):
    assert not bad, "%d mismatches, the first: %s" % (len(bad), "; ".join(bad[:8]))


def packed_input(exp, phase):
    """The blobs back to back `phase` bytes past a 64-byte boundary, TAIL bytes of 0xFF behind the
    last: (the device view that starts at the first blob, offsets as a device tensor, offsets)."""
    off = np.zeros(len(exp) + 1, np.int64)
    off[1:] = np.cumsum([len(e.blob) for e in exp])
    lead = 64 + phase
    buf = np.full(lead + int(off[-1]) + TAIL, FILL, np.uint8)
    buf[lead:lead + int(off[-1])] = np.frombuffer(b"".join(e.blob for e in exp), np.uint8)
    d = torch.from_numpy(buf).cuda()
    return d[lead:], torch.from_numpy(off).cuda(), off


def guarded_output(nbytes, phase):
    """`nbytes` of output `phase` bytes past a 64-byte boundary inside an allocation of 0xA5."""
    lead = 64 + phase
    t = torch.full((lead + nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    return t, t[lead:lead + nbytes], lead


def compare(exp, got_st, got_len, region, bad, tag, where=None):
    """region(i) → the bytes the route gave case i, GAP guard bytes behind them included.
    where(e, at) → optional words on where byte `at` of case e's output lies."""
    for i, e in enumerate(exp):
        if int(got_st[i]) != e.status:
            bad.append("%s %s: status %d, expected %d" % (tag, e.name, got_st[i], e.status))
            continue
        if got_len is not None and int(got_len[i]) != e.size:
            bad.append("%s %s: length %d, expected %d" % (tag, e.name, got_len[i], e.size))
            continue
        r = region(i)
        if r[: e.size].tobytes() != e.out:
            diff = np.flatnonzero(r[: e.size] != np.frombuffer(e.out, np.uint8))
            bad.append("%s %s: %d bytes differ, the first at %d%s" % (tag, e.name, diff.size, diff[0],
                                                                      " (%s)" % where(e, int(diff[0])) if where else ""))
        elif not (r[e.size:] == GUARD).all():
            bad.append("%s %s: wrote past its %d bytes" % (tag, e.name, e.size))


# ------------------------------------------------------------------ a, b: slotted, two thresholds
def run_slotted(codec, exp, in_phase, out_phase, tag, bad, where=None):
    n = len(exp)
    d, o, _ = packed_input(exp, in_phase)
    sizes = np.array([e.size for e in exp], np.int64)
    slots = np.zeros(n + 1, np.int64)
    slots[1:] = np.cumsum(sizes + GAP)  # caller-chosen: a write past a blob's bytes lands on guard bytes
    whole, out, lead = guarded_output(int(slots[-1]), out_phase)
    out, _, ln, st = codec.decode_into(d, o, slots=torch.from_numpy(slots).cuda(), out=out)
    torch.cuda.synchronize()
    h = whole.cpu().numpy()
    st, ln = st.cpu().numpy()[:n], ln.cpu().numpy()[:n]
    compare(exp, st, ln, lambda i: h[lead + slots[i]:lead + slots[i + 1]], bad, tag, where)
    if not ((h[:lead] == GUARD).all() and (h[lead + slots[-1]:] == GUARD).all()):
        bad.append("%s: wrote outside the output buffer" % tag)
    return h[lead:lead + slots[-1]].copy(), st, ln


def check_sizes(codec, exp, in_phase, bad):
    n = len(exp)
    d, o, _ = packed_input(exp, in_phase)
    want = np.array([e.size for e in exp], np.int64)
    want_st = np.array([e.status for e in exp], np.int32)
    sz, st = codec.decoded_sizes(d, o)
    dst = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    sl = codec.decode_slots(d, o, status=dst)
    torch.cuda.synchronize()
    sz, st, sl, dst = sz.cpu().numpy(), st.cpu().numpy(), sl.cpu().numpy(), dst.cpu().numpy()
    for i, e in enumerate(exp):
        if (sz[i], st[i], dst[i]) != (want[i], want_st[i], want_st[i]):
            bad.append("sizes %s: size %d status %d / %d, expected %d and %d" % (e.name, sz[i], st[i], dst[i], want[i],
                                                                               want_st[i]))
    if not np.array_equal(sl, np.concatenate([[0], np.cumsum(want)])):
        bad.append("decode_slots: not the prefix sum of the decoded sizes")


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
def i64(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64, device="cuda")


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
