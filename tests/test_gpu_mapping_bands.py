"""The encoder's byte-plane mapping decision on the GPU, on messages whose byte-position entropies
tie or nearly tie with their mean (tests/mapping_band_cases.py: gaps banded around kFastMargin, the
margin inside which the hardware-log sums hand over to the exact fma chains).  The mapping is in every
blob's header and a wrong bit still decodes, so each route's blobs, lengths and statuses are compared
with the CPU oracle's, computed once per module:

  A  compacted encode_batch, one-wave teams (size hint 1024) and 512-lane teams (65536), tuned widths
  B  slotted encode_into, one batch of every size per width: with TDT_OPT_LARGE_MIN = 65536 the
     131088- and 589840-byte messages take the tiles (their mapping decided from span histograms
     summed in global memory), with the default (256 KiB) only 589840 does and 131088 streams
  C  one encode_vw call over widths 2, 4, 8, 16, 3 and 12, every message in an allocation of its own
     (the scattered kernel instances), some at byte leads 1, 4 and 8
  D  encode_host, one message per call (the one-message path)
  E  the device's blobs of route B decoded back to the inputs (all-ones mappings: an empty stream 0)
  F  analyze_batch at every width and both team shapes: histograms, bit-exact entropies, mappings
     and statuses, with rejected sizes in between
  G  tdt_analyze_host, with a batch of small messages (64-lane instance) and one of large ones

Every context is fresh: no earlier plan's counts switch a size class off.  The helpers return the
names of the cases that differ, so that a run against a deliberately wrong build can count them:
profiles/mapping_bands/mutation.txt.  With the margin set to 0 only the near ties between unrelated
histograms (kind `indep`, band 0: gaps of 5e-10 to 1.3e-6 bits) take a wrong mapping, in routes A to D;
the hardware-log error on kind `near` and on the exact ties stayed below what those cases resolve."""
import numpy as np
import pytest

from oracle.oracle import Oracle, encode_bound
from tests import mapping_band_cases as mb
from tests.support import E_ARG, offsets_of

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, on_gpu  # noqa: E402, F401

pytestmark = pytest.mark.gpu

VW_WIDTHS = (2, 4, 8, 16, 3, 12)
VW_SIZES = {True: (4096, 32784, 65552), False: (4092, 32784, 65556)}  # tuned, generic
LEADS = (0, 1, 4, 8)
HOST_SIZES = (4096, 65536, 131088)
TILE_SHARE = 4096  # a message is tiled above max(large_min, batch bytes / 4096) (encode plan, tdt_encode.h)


def expected():
    """Every case with its message and the oracle's blob and analysis (histograms, entropies, mapping)."""
    orc = Oracle()
    cs = mb.load_cases()
    for c in cs:
        c["blob"] = orc.encode(c["input"], cfg=orc.config(word_size=c["ws"], sample_fraction=1.0), bandwidth=10.0)
        assert c["blob"][:4] == b"DTDT", c["name"]  # compressed: the header carries the mapping
        c["analysis"] = orc.analyze(c["input"], word_size=c["ws"])
    return cs


@pytest.fixture(scope="module")
def cases():
    return expected()


def of_width(cases, ws):
    return [c for c in cases if c["ws"] == ws]


def make_codec(ws, hint=None, large_min=None):
    from psyne_amd import TDTConfig, TdtCodec
    from psyne_amd._lib import TDT_OPT_LARGE_MIN
    c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws))
    c.set_metrics(10.0, 1.0, 0.5)
    if hint is not None:
        c.set_size_hint(hint)
    if large_min is not None:
        c.set_option(TDT_OPT_LARGE_MIN, large_min)
    return c


def differing(sub, blobs, lengths, statuses):
    """Names of the cases whose blob, length or status is not the oracle's."""
    return [c["name"] for c, b, n, s in zip(sub, blobs, lengths, statuses)
            if int(s) != 0 or int(n) != len(c["blob"]) or b != c["blob"]]


# ---------------------------------------------------------------------------------- the routes
def run_compacted(sub, ws, hint):
    codec = make_codec(ws, hint=hint)
    d, o = on_gpu([c["input"] for c in sub])
    enc, eoff, st = codec.encode_batch(d, o)
    torch.cuda.synchronize()
    e, eo, s = enc.cpu().numpy(), eoff.cpu().numpy(), st.cpu().numpy()
    assert eo[0] == 0
    bad = differing(sub, [e[eo[i]:eo[i + 1]].tobytes() for i in range(len(sub))], np.diff(eo), s)
    assert codec.error_flags() == 0
    return bad


def run_slotted(sub, ws, large_min):
    """(names that differ, names that did not decode back)."""
    codec = make_codec(ws, large_min=large_min)
    d, o = on_gpu([c["input"] for c in sub])
    out, slots, lens, st = codec.encode_into(d, o)
    torch.cuda.synchronize()
    oh, sl, ln, s = out.cpu().numpy(), slots.cpu().numpy(), lens.cpu().numpy(), st.cpu().numpy()
    assert sl.tolist() == offsets_of([b"\0" * encode_bound(c["size"], ws) for c in sub]).tolist()
    bad = differing(sub, [oh[sl[i]:sl[i] + ln[i]].tobytes() for i in range(len(sub))], ln, s)
    assert codec.error_flags() == 0
    # E: the device's own blobs, decoded by a fresh context
    dec = make_codec(ws, large_min=large_min)
    back, bsl, bln, bst = dec.decode_into(out, slots, in_lengths=lens[: len(sub)])
    torch.cuda.synchronize()
    bh, bs, bl, bt = back.cpu().numpy(), bsl.cpu().numpy(), bln.cpu().numpy(), bst.cpu().numpy()
    lost = [c["name"] for i, c in enumerate(sub)
            if bt[i] != 0 or bl[i] != c["size"] or bh[bs[i]:bs[i] + bl[i]].tobytes() != c["input"].tobytes()]
    assert dec.error_flags() == 0
    return bad, lost


def vw_subset(cases):
    """Every near tie (both families: every band and sign) at one size per team shape, the widths
    interleaved message by message."""
    per = {ws: [c for c in of_width(cases, ws) if c["kind"] != "tie" and c["size"] in VW_SIZES[ws in mb.TUNED]]
           for ws in VW_WIDTHS}
    assert all(len(v) == 36 for v in per.values())
    return [per[ws][k] for k in range(36) for ws in VW_WIDTHS]


def run_vw(sub):
    def own(data, lead):
        t = torch.empty(lead + data.size + 16, dtype=torch.uint8, device="cuda")
        v = t[lead:lead + data.size]
        v.copy_(torch.from_numpy(data))
        return v

    def i64(values):
        return torch.tensor([int(v) for v in values], dtype=torch.int64, device="cuda")

    codec = make_codec(4)
    tensors = [own(c["input"], LEADS[i % len(LEADS)]) for i, c in enumerate(sub)]
    caps = [encode_bound(c["size"], c["ws"]) for c in sub]
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for cap in caps]
    widths = torch.tensor([c["ws"] for c in sub], dtype=torch.int32, device="cuda")
    ln, st = codec.encode_vw(i64(t.data_ptr() for t in tensors), i64(c["size"] for c in sub), widths,
                             codec.width_mask(VW_WIDTHS), i64(t.data_ptr() for t in outs), i64(caps))
    torch.cuda.synchronize()
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    bad = differing(sub, [o[: ln[i]].cpu().numpy().tobytes() for i, o in enumerate(outs)], ln, st)
    assert codec.error_flags() == 0
    return bad


def run_host(sub, ws):
    codec = make_codec(ws)
    blobs, lens, sts = [], [], []
    for c in sub:
        enc, eoff, st = codec.encode_host(c["input"], np.array([0, c["size"]], np.uint64))
        blobs.append(enc.tobytes())
        lens.append(int(eoff[1]))
        sts.append(int(st[0]))
    bad = differing(sub, blobs, lens, sts)
    assert codec.error_flags() == 0
    return bad


def with_rejects(sub, ws):
    """The messages of `sub` with rejected sizes (0, ws + 1, 2 * ws - 1: no whole number of words; at
    width 1 only the empty message is) in between: (messages, index of the case or None)."""
    odd = [n for n in (0, ws + 1, 2 * ws - 1) if n == 0 or n % ws]
    msgs, which = [], []
    for i, c in enumerate(sub):
        if i % 4 == 0:
            msgs.append(np.full(odd[(i // 4) % len(odd)], 0x5A, np.uint8))
            which.append(None)
        msgs.append(c["input"])
        which.append(i)
    msgs.append(np.zeros(0, np.uint8))
    which.append(None)
    return msgs, which


def run_analyze(sub, ws, hint):
    want = [c["analysis"] for c in sub]
    msgs, which = with_rejects(sub, ws)
    codec = make_codec(ws, hint=hint)
    d, o = on_gpu(msgs)
    hist, ent, mp, st = codec.analyze_batch(d, o)
    torch.cuda.synchronize()
    hist, ent, mp, st = hist.cpu().numpy(), ent.cpu().numpy(), mp.cpu().numpy(), st.cpu().numpy()
    bad = []
    for k, (m, i) in enumerate(zip(msgs, which)):
        if i is None:
            if st[k] != E_ARG:
                bad.append("rejected size %d at row %d: status %d" % (m.size, k, st[k]))
            continue
        (h, e, p), name = want[i], sub[i]["name"]
        if (st[k] != 0 or not np.array_equal(hist[k].astype(np.uint32), h) or ent[k].tobytes() != e.tobytes()
                or not np.array_equal(mp[k], p)):
            bad.append(name)
    assert codec.error_flags() == 0
    return bad


def run_analyze_host(sub, ws):
    want = [c["analysis"] for c in sub]
    codec = make_codec(ws)
    data = np.concatenate([c["input"] for c in sub])
    off = offsets_of([c["input"] for c in sub]).astype(np.uint64)
    n = len(sub)
    ent = np.full((n, ws), -1.0, np.float64)
    mp = np.full((n, ws), -1, np.int32)
    st = np.full(n, -1, np.int32)
    rc = codec._lib.tdt_analyze_host(codec._h, data.ctypes.data, off.ctypes.data, n, ent.ctypes.data, mp.ctypes.data,
                                     st.ctypes.data)
    assert rc == 0
    bad = [c["name"] for i, c in enumerate(sub)
           if st[i] != 0 or ent[i].tobytes() != want[i][1].tobytes() or not np.array_equal(mp[i], want[i][2])]
    assert codec.error_flags() == 0
    return bad


# ---------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("hint", [1024, 65536])
@pytest.mark.parametrize("ws", mb.TUNED)
def test_compacted(cases, ws, hint):
    assert run_compacted(of_width(cases, ws), ws, hint) == []


@pytest.mark.parametrize("large_min", [65536, None], ids=["tiles_above_64k", "default"])
@pytest.mark.parametrize("ws", mb.WIDTHS)
def test_slotted_and_decoded_back(cases, ws, large_min):
    sub = of_width(cases, ws)
    total = sum(c["size"] for c in sub)
    assert total < TILE_SHARE * 65536  # the batch's share stays below large_min: the option decides
    if large_min is not None:
        assert total // TILE_SHARE < large_min < 131088 and any(c["size"] == 131088 for c in sub)
    bad, lost = run_slotted(sub, ws, large_min)
    assert bad == [] and lost == []


def test_scattered_mixed_widths(cases):
    sub = vw_subset(cases)
    assert {(c["band"], c["sign"]) for c in sub if c["kind"] == "near"} == {(b, s) for b in range(4) for s in mb.SIGNS}
    assert {(c["band"], c["sign"]) for c in sub if c["kind"] == "indep"} == \
        {(b, s) for b in mb.INDEP_BANDS for s in mb.SIGNS}
    assert run_vw(sub) == []


@pytest.mark.parametrize("ws", [4, 8])
def test_one_message_host_path(cases, ws):
    sub = [c for c in of_width(cases, ws) if c["size"] in HOST_SIZES]
    assert {(c["size"], c["band"], c["sign"]) for c in sub if c["kind"] == "near"} == \
        {(n, b, s) for n in HOST_SIZES for b in range(4) for s in mb.SIGNS}
    assert run_host(sub, ws) == []


@pytest.mark.parametrize("hint", [1024, 65536])
@pytest.mark.parametrize("ws", mb.WIDTHS)
def test_analyze_batch(cases, ws, hint):
    sub = [c for c in of_width(cases, ws) if c["size"] <= 131088]
    assert run_analyze(sub, ws, hint) == []


@pytest.mark.parametrize("batch", ["small", "large"])
@pytest.mark.parametrize("ws", mb.WIDTHS)
def test_analyze_host(cases, ws, batch):
    """tdt_analyze_host picks the 64-lane instance when the batch's bytes are at most 4096 per message."""
    if batch == "small":
        sub = [c for c in of_width(cases, ws) if c["size"] <= 4096]
        assert sum(c["size"] for c in sub) <= 4096 * len(sub)
    else:
        sub = [c for c in of_width(cases, ws) if c["size"] in (4096, 4092, 65552, 65556, 131088)]
        assert sum(c["size"] for c in sub) > 4096 * len(sub) and any(c["size"] == 131088 for c in sub)
    assert len(sub) >= 8
    assert run_analyze_host(sub, ws) == []
