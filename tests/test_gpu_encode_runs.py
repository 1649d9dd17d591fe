"""Differential encode on the GPU: the run-structured messages of tests/encode_run_cases.py (runs
that start, end and reach a 255-cap chunk start on, before and behind every group, block, round,
wave, tile and span boundary, at every tuned width and stream split; the cap-exclusion family; the
generic widths) through every encode route of the library, status for status, length for length
and byte for byte against the CPU oracle (pinned in tests/golden/encode_runs.json,
tests/test_encode_runs.py).  There is no tolerance.

In every route the outputs lie between 0xA5 guard bytes that must stay intact, the inputs end with
4 KiB of 0xFF, and the codec's device invariant flags must stay 0.  One test per route; each
collects every mismatch and reports the first few by case name.  No route is cut: every case of a
width runs in every route that takes the width."""
import json

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import encode_run_cases as ec
from tests.golden_cases import GOLDEN
from tests.support import report

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, i32, i64, make_codec  # noqa: E402, F401

pytestmark = pytest.mark.gpu

GUARD, FILL, TAIL, GAP = 0xA5, 0xFF, 4096, 16
VW_WIDTHS = (1, 2, 4, 8, 16, 3, 12)  # one encode_vw call takes at most 8 widths


class Expect:
    """One case with the oracle's blob."""

    def __init__(self, case, blob):
        self.name, self.ws, self.mapping, self.n, self.family, self.msg = case
        self.blob = blob
        self.size = len(blob)


def oracle_blob(orc, c, mapping=None):
    return orc.encode(c.msg if isinstance(c, Expect) else c.message, cfg=orc.config(word_size=c.ws, sample_fraction=1.0),
                      bandwidth=10.0, mapping=mapping)


@pytest.fixture(scope="module")
def batch():
    """Every recorded case with the oracle's blob (the oracle runs once for every route)."""
    orc = Oracle()
    dropped = set(json.loads((GOLDEN / "encode_runs.json").read_text())["dropped"])
    return [Expect(c, oracle_blob(orc, c)) for c in ec.all_cases() if c.name not in dropped]


def of_width(batch, ws):
    exp = [e for e in batch if e.ws == ws]
    assert exp
    return exp


def prefix(values):
    off = np.zeros(len(values) + 1, np.int64)
    off[1:] = np.cumsum(values)
    return off


def packed_input(exp, phase):
    """The messages back to back `phase` bytes past a 64-byte boundary, TAIL bytes of 0xFF behind the
    last: (the device view that starts at the first message, offsets as a device tensor)."""
    off = prefix([e.n for e in exp])
    lead = 64 + phase
    buf = np.full(lead + int(off[-1]) + TAIL, FILL, np.uint8)
    buf[lead:lead + int(off[-1])] = np.concatenate([e.msg for e in exp])
    return torch.from_numpy(buf).cuda()[lead:], torch.from_numpy(off).cuda()


def guarded_output(nbytes):
    """`nbytes` of output inside an allocation of 0xA5, 64 guard bytes on either side."""
    t = torch.full((64 + nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    return t, t[64:64 + nbytes]


def locate(e, blob, at):
    """Where blob byte `at` lies: the stream, the stream byte its pair starts at, and the case's
    nearest edge there (kind, placement, d, L)."""
    hdr = 20 + 4 * e.ws
    if at < hdr:
        return "header"
    pos = hdr
    for c in range(int.from_bytes(blob[8:12], "little")):
        length = int.from_bytes(blob[pos:pos + 4], "little")
        if at < pos + 4 + length:
            if at < pos + 4:
                return "stream %d's length word" % c
            pairs = np.frombuffer(blob, np.uint8, length, pos + 4)
            byte = int(pairs[0:(at - pos - 4) // 2 * 2:2].sum(dtype=np.int64))
            near = [x for x in ec.EDGES.get(e.name, ()) if x[0] == c]
            if not near:
                return "stream %d byte %d" % (c, byte)
            _, kind, placement, d, L, a = min(near, key=lambda x: 0 if x[5] <= byte < x[5] + x[4] else min(abs(byte - x[5]), abs(byte - x[5] - x[4])))
            return "stream %d byte %d, nearest edge: %s %s d=%+d L=%d at %d" % (c, byte, kind, placement, d, L, a)
        pos += 4 + length
    return "behind the streams"


def compare(exp, got_st, got_len, region, bad, tag, want=None):
    """region(i) -> the bytes the route gave case i with the guard bytes behind them (if any)."""
    for i, e in enumerate(exp):
        blob = e.blob if want is None else want[i]
        if int(got_st[i]) != 0:
            bad.append("%s %s: status %d" % (tag, e.name, got_st[i]))
            continue
        if got_len is not None and int(got_len[i]) != len(blob):
            bad.append("%s %s: length %d, expected %d" % (tag, e.name, got_len[i], len(blob)))
            continue
        r = region(i)
        if r[: len(blob)].tobytes() != blob:
            diff = np.flatnonzero(r[: len(blob)] != np.frombuffer(blob, np.uint8))
            bad.append("%s %s: %d bytes differ, the first at %d of %d (%s)" % (tag, e.name, diff.size, diff[0], len(blob),
                                                                               locate(e, blob, int(diff[0]))))
        elif not (r[len(blob):] == GUARD).all():
            bad.append("%s %s: wrote past its %d bytes" % (tag, e.name, len(blob)))


# ------------------------------------------------------------------ A, C: compacted
def run_compacted(codec, exp, tag, bad, mappings=None, want=None):
    """encode_batch into exactly the bytes the blobs need; returns the compacted bytes."""
    n = len(exp)
    blobs = [e.blob for e in exp] if want is None else want
    want_off = prefix([len(b) for b in blobs])
    d, o = packed_input(exp, 0)
    whole, out = guarded_output(int(want_off[-1]))
    mp = None if mappings is None else torch.from_numpy(np.concatenate(mappings).astype(np.int32)).cuda()
    _, eoff, st = codec.encode_batch(d, o, out=out, mapping=mp)
    torch.cuda.synchronize()
    h, eoff, st = whole.cpu().numpy(), eoff.cpu().numpy(), st.cpu().numpy()[:n]
    if not np.array_equal(eoff, want_off):
        k = int(np.flatnonzero(eoff != want_off)[0])
        bad.append("%s: offsets differ from entry %d (%s: %d, expected %d; status %d)"
                   % (tag, k, exp[max(k - 1, 0)].name, eoff[k], want_off[k], st[max(k - 1, 0)]))
        return None
    compare(exp, st, None, lambda i: h[64 + want_off[i]:64 + want_off[i + 1]], bad, tag, want=want)
    if not ((h[:64] == GUARD).all() and (h[64 + want_off[-1]:] == GUARD).all()):
        bad.append("%s: wrote outside the output buffer" % tag)
    return h[64:64 + want_off[-1]].copy()


@pytest.mark.parametrize("ws", ec.TUNED)
def test_route_a_compacted(batch, ws):
    """Size hints 1,024 (one-wave teams in the one-pass kernels) and 65,536, with the two phases and
    with the look-back (TDT_OPT_NO_TWO_PHASE); the look-back also over the messages of at most 64 KiB."""
    from psyne_amd._lib import TDT_OPT_NO_TWO_PHASE
    exp = of_width(batch, ws)
    bad = []
    for hint in (1024, 65536):
        for path in ("two_phase", "lookback"):
            codec = make_codec(ws, hint, [(TDT_OPT_NO_TWO_PHASE, 1 if path == "lookback" else 0)])
            run_compacted(codec, exp, "%s(hint %d)" % (path, hint), bad)
            assert codec.error_flags() == 0
    codec = make_codec(ws, 65536, [(TDT_OPT_NO_TWO_PHASE, 1)])
    run_compacted(codec, [e for e in exp if e.n <= 65536], "lookback(<= 64 KiB)", bad)
    assert codec.error_flags() == 0
    report(bad)


@pytest.mark.parametrize("ws", ec.TUNED)
def test_route_c_caller_mapping(batch, ws):
    """encode_batch(mapping=...): with the intended mapping the blobs are route A's; with its
    complement 1 - m (width 1 has one stream and no complement) the run-dense content sits in
    stream 1 and the sparse content in stream 0, against Oracle.encode(mapping=...)."""
    exp = of_width(batch, ws)
    bad = []
    codec = make_codec(ws)
    run_compacted(codec, exp, "intended", bad, mappings=[np.asarray(e.mapping) for e in exp])
    if ws > 1:
        orc = Oracle()
        comp = [1 - np.asarray(e.mapping) for e in exp]
        want = [oracle_blob(orc, e, mapping=m) for e, m in zip(exp, comp)]
        run_compacted(codec, exp, "complement", bad, mappings=comp, want=want)
    assert codec.error_flags() == 0
    report(bad)


# ------------------------------------------------------------------ B: slotted
def run_slotted(codec, exp, phase, tag, bad):
    """encode_into with caller slots of blob length + 16 guard bytes, then decode_into of what it wrote."""
    n = len(exp)
    slots = prefix([e.size + GAP for e in exp])
    dslots = prefix([e.n for e in exp])
    d, o = packed_input(exp, phase)
    whole, out = guarded_output(int(slots[-1]))
    sl = torch.from_numpy(slots).cuda()
    _, _, ln, st = codec.encode_into(d, o, slots=sl, out=out)
    torch.cuda.synchronize()
    h, lh, sh = whole.cpu().numpy(), ln.cpu().numpy()[:n], st.cpu().numpy()[:n]
    compare(exp, sh, lh, lambda i: h[64 + slots[i]:64 + slots[i + 1]], bad, tag)
    if not ((h[:64] == GUARD).all() and (h[64 + slots[-1]:] == GUARD).all()):
        bad.append("%s: wrote outside the output buffer" % tag)
    if (sh != 0).any():
        return
    back, _, dl, ds = codec.decode_into(out, sl, in_lengths=ln[:n], slots=torch.from_numpy(dslots).cuda())
    torch.cuda.synchronize()
    back, dl, ds = back.cpu().numpy(), dl.cpu().numpy()[:n], ds.cpu().numpy()[:n]
    for i, e in enumerate(exp):
        if ds[i] != 0 or dl[i] != e.n or not np.array_equal(back[dslots[i]:dslots[i + 1]], e.msg):
            bad.append("%s %s: does not decode back (status %d, length %d)" % (tag, e.name, ds[i], dl[i]))


@pytest.mark.parametrize("ws", ec.TUNED + ec.GENERIC)
def test_route_b_slotted(batch, ws):
    """TDT_OPT_LARGE_MIN default and 65,536 (the 196,640- and 589,840-byte messages then take the
    tiles), input byte phases 0 and 5; every blob decoded back with decode_into."""
    from psyne_amd._lib import TDT_OPT_LARGE_MIN
    exp = of_width(batch, ws)
    bad = []
    for large_min in (None, 65536):
        codec = make_codec(ws, options=[] if large_min is None else [(TDT_OPT_LARGE_MIN, large_min)])
        for phase in (0, 5):
            run_slotted(codec, exp, phase, "slotted(large_min=%s,phase=%d)" % (large_min or "default", phase), bad)
        assert codec.error_flags() == 0
    report(bad)


# ------------------------------------------------------------------ D: scattered


@pytest.fixture(scope="module")
def scattered(batch):
    """name -> the message in a device allocation of its own, 0..3 bytes into it, 0xFF behind it."""
    out = {}
    for k, e in enumerate(batch):
        t = torch.full((k % 4 + e.n + 16,), FILL, dtype=torch.uint8, device="cuda")
        v = t[k % 4:k % 4 + e.n]
        v.copy_(torch.from_numpy(e.msg.copy()))
        out[e.name] = v
    return out


def mixed(batch):
    """The cases of the widths one encode_vw call takes, the widths interleaved."""
    exp = [e for e in batch if e.ws in VW_WIDTHS]
    return [exp[i] for i in np.random.default_rng(ec.SEED).permutation(len(exp))]


def width_mask(widths):
    from psyne_amd import TdtCodec
    return TdtCodec.width_mask(widths)


def check_scattered(exp, outs, ln, st, tag, bad):
    compare(exp, st, ln, lambda i: outs[i].cpu().numpy()[64:], bad, tag)
    for i, e in enumerate(exp):
        if not (outs[i][:64] == GUARD).all():
            bad.append("%s %s: wrote before its output" % (tag, e.name))


@pytest.mark.parametrize("ws", ec.TUNED + ec.GENERIC)
def test_route_d_encode_v(batch, scattered, ws):
    """Every message and every blob in an allocation of its own, the capacity the blob's length."""
    exp = of_width(batch, ws)
    bad = []
    outs = [torch.full((64 + e.size + 64,), GUARD, dtype=torch.uint8, device="cuda") for e in exp]
    codec = make_codec(ws)
    ln, st = codec.encode_v(i64(scattered[e.name].data_ptr() for e in exp), i64(e.n for e in exp),
                            i64(t.data_ptr() + 64 for t in outs), i64(e.size for e in exp))
    torch.cuda.synchronize()
    check_scattered(exp, outs, ln.cpu().numpy(), st.cpu().numpy(), "encode_v", bad)
    assert codec.error_flags() == 0
    report(bad)


def test_route_d_encode_vw(batch, scattered):
    """One call over the widths 1, 2, 4, 8, 16, 3 and 12, interleaved message by message."""
    exp = mixed(batch)
    bad = []
    outs = [torch.full((64 + e.size + 64,), GUARD, dtype=torch.uint8, device="cuda") for e in exp]
    codec = make_codec(4)
    ln, st = codec.encode_vw(i64(scattered[e.name].data_ptr() for e in exp), i64(e.n for e in exp),
                             i32(e.ws for e in exp), width_mask(VW_WIDTHS), i64(t.data_ptr() + 64 for t in outs),
                             i64(e.size for e in exp))
    torch.cuda.synchronize()
    check_scattered(exp, outs, ln.cpu().numpy(), st.cpu().numpy(), "encode_vw", bad)
    assert codec.error_flags() == 0
    report(bad)


@pytest.mark.parametrize("sizes_first", [0, 1])
def test_route_d_encode_vp(batch, scattered, sizes_first):
    """The packed wire buffer of the mixed-width batch, exactly as long as the blobs, with and
    without TDT_OPT_PACK_SIZES_FIRST."""
    from psyne_amd._lib import TDT_OPT_PACK_SIZES_FIRST
    exp = mixed(batch)
    n = len(exp)
    bad = []
    want_off = prefix([e.size for e in exp])
    whole, out = guarded_output(int(want_off[-1]))
    codec = make_codec(4, options=[(TDT_OPT_PACK_SIZES_FIRST, sizes_first)])
    off, st = codec.encode_vp(i64(scattered[e.name].data_ptr() for e in exp), i64(e.n for e in exp),
                              sum(e.n for e in exp), out, word_sizes=i32(e.ws for e in exp), width_mask=width_mask(VW_WIDTHS))
    torch.cuda.synchronize()
    h, off, st = whole.cpu().numpy(), off.cpu().numpy(), st.cpu().numpy()[:n]
    if not np.array_equal(off, want_off):
        k = int(np.flatnonzero(off != want_off)[0])
        bad.append("encode_vp: offsets differ from entry %d (%s)" % (k, exp[max(k - 1, 0)].name))
    else:
        compare(exp, st, None, lambda i: h[64 + want_off[i]:64 + want_off[i + 1]], bad, "encode_vp")
    if not ((h[:64] == GUARD).all() and (h[64 + want_off[-1]:] == GUARD).all()):
        bad.append("encode_vp: wrote outside the output buffer")
    assert codec.error_flags() == 0
    report(bad)


# ------------------------------------------------------------------ E: sizes only
@pytest.mark.parametrize("ws", ec.TUNED + ec.GENERIC)
def test_route_e_encoded_sizes(batch, scattered, ws):
    """MODE_SIZES: encoded_sizes over the contiguous batch (TDT_OPT_LARGE_MIN default and 65,536) and
    encoded_sizes_v over the scattered one give len(oracle blob) with status 0."""
    from psyne_amd._lib import TDT_OPT_LARGE_MIN
    exp = of_width(batch, ws)
    n = len(exp)
    bad = []
    want = np.array([e.size for e in exp], np.int64)
    for large_min in (None, 65536):
        codec = make_codec(ws, options=[] if large_min is None else [(TDT_OPT_LARGE_MIN, large_min)])
        d, o = packed_input(exp, 0)
        runs = [("encoded_sizes", codec.encoded_sizes(d, o)),
                ("encoded_sizes_v", codec.encoded_sizes_v(i64(scattered[e.name].data_ptr() for e in exp), i64(e.n for e in exp)))]
        torch.cuda.synchronize()
        for tag, (sz, st) in runs:
            sz, st = sz.cpu().numpy()[:n], st.cpu().numpy()[:n]
            for i in np.flatnonzero((sz != want) | (st != 0)):
                bad.append("%s(large_min %s) %s: size %d status %d, expected %d" % (tag, large_min or "default", exp[i].name,
                                                                                 sz[i], st[i], want[i]))
        assert codec.error_flags() == 0
    report(bad)


def test_route_e_encoded_sizes_mixed(batch, scattered):
    exp = mixed(batch)
    codec = make_codec(4)
    sz, st = codec.encoded_sizes_v(i64(scattered[e.name].data_ptr() for e in exp), i64(e.n for e in exp),
                                   word_sizes=i32(e.ws for e in exp), width_mask=width_mask(VW_WIDTHS))
    torch.cuda.synchronize()
    sz, st = sz.cpu().numpy(), st.cpu().numpy()
    bad = ["%s: size %d status %d, expected %d" % (e.name, sz[i], st[i], e.size) for i, e in enumerate(exp)
           if (sz[i], st[i]) != (e.size, 0)]
    assert codec.error_flags() == 0
    report(bad)


# ------------------------------------------------------------------ F: one message per host call
@pytest.mark.parametrize("ws", [4, 8])
def test_route_f_encode_host(batch, ws):
    """tdt_encode_host with one message per call, every case of up to 262,144 bytes."""
    from psyne_amd._lib import check
    exp = [e for e in of_width(batch, ws) if e.n <= 262144]
    codec = make_codec(ws)
    lib, h = codec._lib, codec._h
    bad = []
    for e in exp:
        src = np.full(e.n + TAIL, FILL, np.uint8)
        src[: e.n] = e.msg
        out = np.full(64 + e.size + 64, GUARD, np.uint8)
        off = np.array([0, e.n], np.uint64)
        ooff = np.zeros(2, np.uint64)
        st = np.full(1, -1, np.int32)
        check(lib.tdt_encode_host(h, src.ctypes.data, off.ctypes.data, 1, out.ctypes.data + 64, e.size, ooff.ctypes.data,
                                  st.ctypes.data))
        compare([e], st, [int(ooff[1])], lambda i: out[64:], bad, "host")
        if not (out[:64] == GUARD).all():
            bad.append("host %s: wrote before its output" % e.name)
    assert codec.error_flags() == 0
    report(bad)
