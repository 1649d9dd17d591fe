"""The raw fallback on the GPU (TDT_OPT_RAW_FALLBACK): every device-batch encode route stores a message
whose TDT blob would be longer than n + 4 bytes as its UNCP blob, and leaves every other message's
blob, length and status as they are.  Expected bytes are tests/raw_fallback_cases.py's — the CPU
oracle's blob, or "UNCP" + the message where that is longer than n + 4 — and every comparison is
bit-exact.  Outputs lie between 0xA5 guard bytes that must stay intact, results are decoded back with
decode_v, and TDT_STAT_RAW_FALLBACKS tells which path ran."""
import contextlib
import gc

import numpy as np
import pytest

from tests import raw_fallback_cases as rc
from tests.support import CANARY, E_CAPACITY, E_CAPTURE, E_UNSUPPORTED, mask_of

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, guarded, i32, i64, orc, own, ptrs, u64  # noqa: E402, F401

pytestmark = pytest.mark.gpu

OPT_LARGE_MIN, OPT_NO_TWO_PHASE, OPT_PACK_SIZES_FIRST, OPT_ANY_TILED, OPT_RAW_FALLBACK = 1, 5, 7, 8, 10
LEADS = (0, 1, 4)  # pointer offsets of the messages and of the blobs


@pytest.fixture(autouse=True)
def _no_garbage_left():
    yield
    gc.collect()


def make_codec(ws=4, raw=True, tiled=False, bandwidth=10.0):
    from psyne_amd import TDTConfig, TdtCodec
    c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws))
    c.set_metrics(bandwidth, 1.0, 0.5)
    if tiled:
        c.set_option(OPT_LARGE_MIN, rc.LARGE_MIN_TILED)
    if raw:
        c.set_option(OPT_RAW_FALLBACK, 1)
    return c


@pytest.fixture(scope="module")
def cases(orc):
    """The fixture batches by (ws, n), made once and never changed; each with its device tensors."""
    made = {}

    def get(ws, n):
        if (ws, n) not in made:
            b = rc.batch(orc, ws, n, rc.seed_of(ws, n))
            for k, c in enumerate(b):
                c["t"] = own(c["x"], LEADS[k % 3])
            made[(ws, n)] = b
        return made[(ws, n)]
    return get


def outputs(caps):
    return [guarded(c, LEADS[(k + 1) % 3]) for k, c in enumerate(caps)]


def check_blobs(batch, outs, caps, ln, st, want=None, what=""):
    """Bytes, lengths, statuses and guards of one scattered result."""
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    for k, c in enumerate(batch):
        w = want[k] if want is not None else c["want"]
        tag = "%s %s" % (what, c["name"])
        h = outs[k][0].cpu().numpy()
        lead = h.size - 128 - caps[k]
        assert (int(st[k]), int(ln[k])) == (0, len(w)), tag
        assert h[64 + lead:64 + lead + len(w)].tobytes() == w, tag
        assert (h[:64 + lead] == CANARY).all() and (h[64 + lead + caps[k]:] == CANARY).all(), tag


def decode_back(codec, batch, blob_views, lens):
    sizes = [c["x"].size for c in batch]
    back = [torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda") for n in sizes]
    dl, ds = codec.decode_v(ptrs(blob_views), i64(lens), ptrs(back), i64(sizes))
    torch.cuda.synchronize()
    assert int(ds.abs().sum()) == 0 and dl.cpu().numpy()[: len(sizes)].tolist() == sizes
    for c, b in zip(batch, back):
        assert np.array_equal(b.cpu().numpy()[: c["x"].size], c["x"]), c["name"]


def encode_v(codec, batch, caps, **kw):
    outs = outputs(caps)
    tensors = [c["t"] for c in batch]
    ln, st = codec.encode_v(ptrs(tensors), i64(c["x"].size for c in batch), ptrs([v for _, v in outs]), i64(caps), **kw)
    torch.cuda.synchronize()
    return outs, ln, st


def falls(batch):
    return sum(1 for c in batch if c["falls"])


CONFIGS = rc.all_configs()


# ------------------------------------------------------------------------------- 1: every class, every width
@pytest.mark.parametrize("ws,n,tiled", CONFIGS, ids=["ws%d-n%d%s" % (w, n, "-tiled" if t else "") for w, n, t in CONFIGS])
def test_encode_v_exact_slots(cases, ws, n, tiled):
    """Slots of exactly n + 4 bytes: every kind is written, the expanding ones raw."""
    batch = cases(ws, n)
    caps = [c["x"].size + 4 for c in batch]
    for any_tiled in ((0, 1) if tiled and ws not in (1, 2, 4, 8, 16) else (1,)):
        codec = make_codec(ws, tiled=tiled)
        codec.set_option(OPT_ANY_TILED, any_tiled)
        outs, ln, st = encode_v(codec, batch, caps)
        check_blobs(batch, outs, caps, ln, st, what="any_tiled %d" % any_tiled)
        assert codec.stat("RAW_FALLBACKS") == falls(batch) > 0
        assert codec.error_flags() == 0
        decode_back(codec, batch, [v for _, v in outs], ln.cpu().numpy()[: len(batch)])


CAP_CONFIGS = [(4, 1024, False), (4, 65536, False), (4, 196640, True), (8, 1024, False), (2, 65536, False),
               (16, 196640, True), (12, 12288, False)]


@pytest.mark.parametrize("ws,n,tiled", CAP_CONFIGS)
def test_capacities(cases, ws, n, tiled):
    batch = cases(ws, n)
    codec = make_codec(ws, tiled=tiled)
    # the old bound: the same blobs
    caps = [max(c["x"].size + 4, 28 + 4 * ws + 2 * c["x"].size) for c in batch]
    outs, ln, st = encode_v(codec, batch, caps)
    check_blobs(batch, outs, caps, ln, st, what="old bound")
    # one byte short of min(E, n + 4) for the expanding messages, two short of E for the compressing ones
    short = [c["x"].size + 3 if c["falls"] else len(c["want"]) - 2 for c in batch]
    outs, ln, st = encode_v(codec, batch, short)
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    for k, c in enumerate(batch):
        assert (int(st[k]), int(ln[k])) == (E_CAPACITY, 0), c["name"]
        h = outs[k][0].cpu().numpy()
        lead = h.size - 128 - short[k]
        assert (h[:64 + lead] == CANARY).all() and (h[64 + lead + short[k]:] == CANARY).all(), c["name"]
        # nothing at all is written at the tuned widths, whose kernels place before they emit; the
        # one-workgroup generic kernel writes as it counts and stays inside its slot (a byte of a slot
        # beyond the final blob — here all of it — may hold anything), so there the guards above decide
        if c["falls"] and ws in (1, 2, 4, 8, 16):
            assert (h == CANARY).all(), c["name"]
    assert codec.stat("RAW_FALLBACKS") == 0
    # exactly min(E, n + 4)
    exact = [len(c["want"]) for c in batch]
    outs, ln, st = encode_v(codec, batch, exact)
    check_blobs(batch, outs, exact, ln, st, what="exact")
    assert codec.error_flags() == 0


def test_option_off_on_the_same_context(cases):
    batch = cases(4, 1024) + cases(4, 65536)
    codec = make_codec(4)
    caps = [max(c["x"].size + 4, 28 + 16 + 2 * c["x"].size) for c in batch]
    outs, ln, st = encode_v(codec, batch, caps)
    check_blobs(batch, outs, caps, ln, st)
    assert codec.stat("RAW_FALLBACKS") == falls(batch)
    codec.set_option(OPT_RAW_FALLBACK, 0)
    outs, ln, st = encode_v(codec, batch, caps)
    check_blobs(batch, outs, caps, ln, st, want=[c["plain"] for c in batch], what="option off")
    assert codec.stat("RAW_FALLBACKS") == 0
    assert codec.encode_bound(1000) == 28 + 16 + 2000
    codec.set_option(OPT_RAW_FALLBACK, 1)
    assert codec.encode_bound(1000) == 1004
    outs, ln, st = encode_v(codec, batch, caps)
    check_blobs(batch, outs, caps, ln, st, what="option on again")
    assert codec.stat("RAW_FALLBACKS") == falls(batch)


def test_policy_off_takes_uncp_by_routing(cases, orc):
    batch = cases(4, 1024)
    codec = make_codec(4, bandwidth=1000.0)
    caps = [c["x"].size + 4 for c in batch]
    outs, ln, st = encode_v(codec, batch, caps)
    want = [rc.expected_blob(orc, c["x"], 4, policy_on=False)[0] for c in batch]
    assert all(w == rc.UNCP + c["x"].tobytes() for w, c in zip(want, batch))
    check_blobs(batch, outs, caps, ln, st, want=want)
    assert codec.stat("RAW_FALLBACKS") == 0  # (routed, not fallen back)


# ------------------------------------------------------------------------------- 2: the contiguous routes
def contiguous(batch):
    data = np.concatenate([c["x"] for c in batch])
    off = np.zeros(len(batch) + 1, np.int64)
    off[1:] = np.cumsum([c["x"].size for c in batch])
    return torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda(), off


@pytest.mark.parametrize("ws,n,tiled", [(4, 1024, False), (4, 65536, False), (4, 196640, True), (3, 12288, False)])
def test_encode_into_and_sizes(cases, ws, n, tiled):
    batch = cases(ws, n)
    codec = make_codec(ws, tiled=tiled)
    d, o, off = contiguous(batch)
    slots = codec.encode_slots(o)
    want_slots = np.zeros(len(batch) + 1, np.int64)
    want_slots[1:] = np.cumsum([c["x"].size + 4 for c in batch])
    assert slots.cpu().numpy().tolist() == want_slots.tolist()
    assert codec.batch_bound(off) == int(want_slots[-1])
    t, out = guarded(int(want_slots[-1]), 4)
    _, _, ln, st = codec.encode_into(d, o, slots=slots, out=out)
    es, est = codec.encoded_sizes(d, o)
    torch.cuda.synchronize()
    ln, st, h = ln.cpu().numpy(), st.cpu().numpy(), t.cpu().numpy()
    assert es.cpu().numpy().tolist() == [len(c["want"]) for c in batch] and int(est.abs().sum()) == 0
    for k, c in enumerate(batch):
        assert (int(st[k]), int(ln[k])) == (0, len(c["want"])), c["name"]
        b = 68 + int(want_slots[k])
        assert h[b:b + len(c["want"])].tobytes() == c["want"], c["name"]
    assert (h[:68] == CANARY).all() and (h[68 + int(want_slots[-1]):] == CANARY).all()
    assert codec.stat("RAW_FALLBACKS") == falls(batch)
    views = [out[int(want_slots[k]):int(want_slots[k + 1])] for k in range(len(batch))]
    decode_back(codec, batch, views, ln[: len(batch)])
    assert codec.error_flags() == 0


@pytest.mark.parametrize("ws,n", [(4, 1024), (4, 65536), (12, 12288)])
def test_encode_batch_compacted(cases, ws, n):
    from psyne_amd._lib import TdtError
    batch = cases(ws, n)
    codec = make_codec(ws)
    d, o, off = contiguous(batch)
    enc, eoff, st = codec.encode_batch(d, o)
    torch.cuda.synchronize()
    eoff = eoff.cpu().numpy()
    assert int(st.abs().sum()) == 0 and int(eoff[-1]) == sum(len(c["want"]) for c in batch)
    h = enc.cpu().numpy()
    for k, c in enumerate(batch):
        assert h[eoff[k]:eoff[k + 1]].tobytes() == c["want"], c["name"]
    assert codec.stat("RAW_FALLBACKS") == falls(batch)
    codec.set_option(OPT_NO_TWO_PHASE, 1)
    with pytest.raises(TdtError) as ei:
        codec.encode_batch(d, o)
    assert ei.value.code == E_UNSUPPORTED
    del ei
    # and under stream capture (the two phases read the batch size back), with nothing allocated inside it
    codec.set_option(OPT_NO_TWO_PHASE, 0)
    out = torch.zeros(codec.batch_bound(off), dtype=torch.uint8, device="cuda")
    ooff = torch.zeros(len(batch) + 1, dtype=torch.int64, device="cuda")
    ost = torch.zeros(len(batch), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with pytest.raises(TdtError) as ei:
        with capture(gr):
            codec.encode_batch(d, o, out=out, out_offsets=ooff, status=ost)
    assert ei.value.code == E_UNSUPPORTED
    del ei, gr, codec


# ------------------------------------------------------------------------------- 3: mixed widths and packing
MIXED = [(2, 1024), (4, 1024), (8, 1024), (12, 1032), (4, 65536), (12, 12288)]


@pytest.fixture(scope="module")
def mixed(cases):
    """Messages of widths 2, 4, 8 and 12, interleaved width by width."""
    lists = [cases(ws, n) for ws, n in MIXED]
    out = []
    for k in range(max(len(b) for b in lists)):
        out += [b[k] for b in lists if k < len(b)]
    return out


def test_encode_vw(mixed):
    codec = make_codec(4)
    caps = [c["x"].size + 4 for c in mixed]
    outs = outputs(caps)
    tensors = [c["t"] for c in mixed]
    ws, mask = i32(c["ws"] for c in mixed), mask_of([2, 4, 8, 12])
    ln, st = codec.encode_vw(ptrs(tensors), i64(c["x"].size for c in mixed), ws, mask, ptrs([v for _, v in outs]), i64(caps))
    es, est = codec.encoded_sizes_v(ptrs(tensors), i64(c["x"].size for c in mixed), word_sizes=ws, width_mask=mask)
    torch.cuda.synchronize()
    check_blobs(mixed, outs, caps, ln, st)
    assert es.cpu().numpy().tolist() == [len(c["want"]) for c in mixed] and int(est.abs().sum()) == 0
    assert codec.stat("RAW_FALLBACKS") == falls(mixed)
    decode_back(codec, mixed, [v for _, v in outs], ln.cpu().numpy()[: len(mixed)])
    assert codec.error_flags() == 0


@pytest.mark.parametrize("sizes_first", [0, 1, 2])
@pytest.mark.parametrize("widths", [False, True])
def test_encode_vp(cases, mixed, sizes_first, widths):
    batch = mixed if widths else cases(4, 1024) + cases(4, 65536)
    codec = make_codec(4)
    codec.set_option(OPT_PACK_SIZES_FIRST, sizes_first)
    tensors = [c["t"] for c in batch]
    total = sum(len(c["want"]) for c in batch)
    t, out = guarded(total, 1)
    kw = dict(word_sizes=i32(c["ws"] for c in batch), width_mask=mask_of([2, 4, 8, 12])) if widths else {}
    off, st = codec.encode_vp(ptrs(tensors), i64(c["x"].size for c in batch), sum(c["x"].size for c in batch), out, **kw)
    torch.cuda.synchronize()
    off, h = off.cpu().numpy(), t.cpu().numpy()
    assert int(st.abs().sum()) == 0 and int(off[-1]) == total
    for k, c in enumerate(batch):
        assert h[65 + off[k]:65 + off[k + 1]].tobytes() == c["want"], c["name"]
    assert (h[:65] == CANARY).all() and (h[65 + total:] == CANARY).all()
    assert codec.stat("RAW_FALLBACKS") == falls(batch)
    views = [out[int(off[k]):int(off[k + 1])] for k in range(len(batch))]
    decode_back(codec, batch, views, np.diff(off))
    assert codec.error_flags() == 0


@pytest.mark.parametrize("widths", [False, True])
def test_packed_scratch_is_total_plus_4n(cases, mixed, widths):
    """The halving the option is for: the two-phase packed encode's scratch on a fresh context is
    total_bytes + 4 n with the option, 2 total_bytes + n (28 + 4 wmax) without."""
    batch = mixed if widths else cases(4, 1024) + cases(4, 65536)
    tensors = [c["t"] for c in batch]
    n, total_in = len(batch), sum(c["x"].size for c in batch)
    wmax = 12 if widths else 4
    kw = dict(word_sizes=i32(c["ws"] for c in batch), width_mask=mask_of([2, 4, 8, 12])) if widths else {}
    for raw, want in ((True, total_in + 4 * n), (False, 2 * total_in + n * (28 + 4 * wmax))):
        codec = make_codec(4, raw=raw)
        assert codec.stat("PACK_SCRATCH_BYTES") == 0
        out = torch.zeros(2 * total_in + 64 * n, dtype=torch.uint8, device="cuda")
        off, st = codec.encode_vp(ptrs(tensors), i64(c["x"].size for c in batch), total_in, out, **kw)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0
        assert int(off[-1]) == sum(len(c["want"] if raw else c["plain"]) for c in batch)
        assert codec.stat("PACK_SCRATCH_BYTES") == want, "raw_fallback %s" % raw
        # sizes first: no scratch at all, with the option as without
        sf = make_codec(4, raw=raw)
        sf.set_option(OPT_PACK_SIZES_FIRST, 1)
        sf.encode_vp(ptrs(tensors), i64(c["x"].size for c in batch), total_in, out, **kw)
        torch.cuda.synchronize()
        assert sf.stat("PACK_SCRATCH_BYTES") == 0


def test_encode_tensors_packed_exact(cases):
    batch = [c for c in cases(4, 1024) + cases(4, 65536) if c["x"].size]
    codec = make_codec(4)
    out, off, st = codec.encode_tensors([c["t"] for c in batch], packed=True, exact=True)
    torch.cuda.synchronize()
    off, h = off.cpu().numpy(), out.cpu().numpy()
    assert int(st.abs().sum()) == 0 and out.numel() == int(off[-1]) == sum(len(c["want"]) for c in batch)
    for k, c in enumerate(batch):
        assert h[off[k]:off[k + 1]].tobytes() == c["want"], c["name"]
    # the slotted form allocates by the context's bound
    out, slots, ln, st = codec.encode_tensors([c["t"] for c in batch])
    torch.cuda.synchronize()
    assert int(slots[-1]) == sum(c["x"].size + 4 for c in batch) and int(st.abs().sum()) == 0
    assert ln.cpu().numpy()[: len(batch)].tolist() == [len(c["want"]) for c in batch]


# ------------------------------------------------------------------------------- 4: known mappings


@pytest.mark.parametrize("ws,n", [(4, 1024), (4, 65536), (12, 12288)])
def test_mappings_v_and_the_mapped_encodes(cases, ws, n):
    batch = cases(ws, n)
    tensors = [c["t"] for c in batch]
    args = (ptrs(tensors), i64(c["x"].size for c in batch))
    off_codec, codec = make_codec(ws, raw=False), make_codec(ws)
    _, off_bits, _ = off_codec.mappings_v(*args)
    sz, bits, st = codec.mappings_v(*args)
    torch.cuda.synchronize()
    assert torch.equal(bits, off_bits)  # the bits stay the analysed mapping, fallen back or not
    assert any(int(b) for b, c in zip(bits.cpu().numpy(), batch) if c["falls"])
    assert sz.cpu().numpy().tolist() == [len(c["want"]) for c in batch] and int(st.abs().sum()) == 0
    caps = [c["x"].size + 4 for c in batch]
    outs, ln, st = encode_v(codec, batch, caps, mapbits=bits)
    check_blobs(batch, outs, caps, ln, st, what="mapped")
    assert codec.stat("RAW_FALLBACKS") == falls(batch)
    total = sum(len(c["want"]) for c in batch)
    t, out = guarded(total)
    off, st = codec.encode_vp(*args, sum(c["x"].size for c in batch), out, mapbits=bits)
    torch.cuda.synchronize()
    off, h = off.cpu().numpy(), t.cpu().numpy()
    assert int(st.abs().sum()) == 0 and int(off[-1]) == total
    for k, c in enumerate(batch):
        assert h[64 + off[k]:64 + off[k + 1]].tobytes() == c["want"], c["name"]
    assert (h[:64] == CANARY).all() and (h[64 + total:] == CANARY).all()


def test_single_stream_threshold_mappings(orc):
    for ws, n in rc.MAPPED_TRIOS:
        trio = rc.mapped_trio(orc, ws, n)
        assert [c["falls"] for c in trio] == [False, False, True]
        for c in trio:
            c["t"] = own(c["x"], 1)
        codec = make_codec(ws)
        caps = [c["x"].size + 4 for c in trio]
        outs, ln, st = encode_v(codec, trio, caps, mapbits=u64([0, 0, 0]))
        check_blobs(trio, outs, caps, ln, st, what="single stream")
        assert codec.stat("RAW_FALLBACKS") == 1
        decode_back(codec, trio, [v for _, v in outs], ln.cpu().numpy()[:3])
        # and packed: tdt_encode_mapped_vp
        total = sum(len(c["want"]) for c in trio)
        t, out = guarded(total, 4)
        off, st = codec.encode_vp(ptrs([c["t"] for c in trio]), i64(c["x"].size for c in trio), sum(c["x"].size for c in trio),
                                  out, mapbits=u64([0, 0, 0]))
        torch.cuda.synchronize()
        off, h = off.cpu().numpy(), t.cpu().numpy()
        assert int(st.abs().sum()) == 0 and int(off[-1]) == total
        for k, c in enumerate(trio):
            assert h[68 + off[k]:68 + off[k + 1]].tobytes() == c["want"], c["name"]
        assert (h[:68] == CANARY).all() and (h[68 + total:] == CANARY).all()
        assert codec.stat("RAW_FALLBACKS") == 1


# ------------------------------------------------------------------------------- 5: capture
@contextlib.contextmanager
def capture(gr):
    gc.collect()  # (nothing is finalised inside the capture window)
    with torch.cuda.graph(gr):
        yield


def test_capture_on_a_cold_context_is_refused(cases):
    from psyne_amd._lib import TdtError
    batch = cases(4, 1024)
    codec = make_codec(4)
    caps = [c["x"].size + 4 for c in batch]
    outs = outputs(caps)
    args = (ptrs([c["t"] for c in batch]), i64(c["x"].size for c in batch), ptrs([v for _, v in outs]), i64(caps))
    ln = torch.zeros(len(batch), dtype=torch.int64, device="cuda")
    st = torch.zeros(len(batch), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with pytest.raises(TdtError) as ei:
        with capture(gr):
            codec.encode_v(*args, lengths=ln, status=st)
    assert ei.value.code == E_CAPTURE
    del ei, gr, codec


def test_captured_encode_v_replays(cases):
    """One graph, the input swapped in place between compressing and expanding bytes."""
    batch = cases(4, 65536)
    a = next(c for c in batch if c["kind"] == "grad70")
    b = next(c for c in batch if c["kind"] == "uniform")
    bufs = [torch.zeros(65536, dtype=torch.uint8, device="cuda") for _ in range(3)]
    caps = [65540] * 3
    outs = outputs(caps)
    args = (ptrs(bufs), i64([65536] * 3), ptrs([v for _, v in outs]), i64(caps))
    ln = torch.zeros(3, dtype=torch.int64, device="cuda")
    st = torch.zeros(3, dtype=torch.int32, device="cuda")
    codec = make_codec(4)

    def fill(kinds):
        for buf, c in zip(bufs, kinds):
            buf.copy_(torch.from_numpy(c["x"]))
        for t, _ in outs:
            t.fill_(CANARY)
        return [dict(c) for c in kinds]
    fill([a, b, a])
    codec.encode_v(*args, lengths=ln, status=st)  # eager: the workspaces of this batch size exist from here on
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with capture(gr):
        codec.encode_v(*args, lengths=ln, status=st)
    for kinds in ([b, a, b], [a, a, b]):
        now = fill(kinds)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        check_blobs(now, outs, caps, ln, st, what="replay")
    assert codec.error_flags() == 0
    del gr


# ------------------------------------------------------------------------------- 6: the calls that ignore the option
@pytest.mark.parametrize("ws,n", [(4, 1024), (12, 12288), (3, 1032)])
def test_host_and_parity_calls_ignore_the_option(cases, orc, ws, n):
    """At a generic width the parity hook encodes into scratch slots and gathers: slots of the TDT bound."""
    batch = [c for c in cases(ws, n) if c["kind"] in ("uniform", "grad70", "thr+2", "dense")]
    assert falls(batch) >= 2
    codec = make_codec(ws)
    data = np.concatenate([c["x"] for c in batch])
    off = np.zeros(len(batch) + 1, np.uint64)
    off[1:] = np.cumsum([c["x"].size for c in batch])
    out, out_off, st = codec.encode_host(data, off)
    assert int(np.abs(st).sum()) == 0
    for k, c in enumerate(batch):
        assert out[int(out_off[k]):int(out_off[k + 1])].tobytes() == c["plain"], c["name"]
    maps = [[int(x) for x in orc.analyze(c["x"], ws)[2]] for c in batch]
    mp = torch.from_numpy(np.array(maps, np.int32).reshape(-1)).cuda()
    cap = sum(28 + 4 * ws + 2 * c["x"].size for c in batch)
    d, o = torch.from_numpy(data).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    # a caller's buffer of the TDT bound, and the wrapper's own allocation (which must be that bound too)
    for kw in (dict(out_capacity=cap, out=torch.zeros(cap, dtype=torch.uint8, device="cuda")), {}):
        enc, eoff, est = codec.encode_batch(d, o, mapping=mp, **kw)
        torch.cuda.synchronize()
        eoff, h = eoff.cpu().numpy(), enc.cpu().numpy()
        assert int(est.abs().sum()) == 0 and enc.numel() >= cap
        for k, c in enumerate(batch):
            assert h[eoff[k]:eoff[k + 1]].tobytes() == c["plain"], c["name"]
