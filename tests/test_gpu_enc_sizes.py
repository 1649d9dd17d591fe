"""Exact encoded sizes on the GPU (tdt_encoded_sizes_batch / tdt_encoded_sizes_v: TdtCodec.encoded_sizes,
encoded_sizes_v), the sizes-first packed encode (TDT_OPT_PACK_SIZES_FIRST) and
encode_tensors(packed=True, exact=True).  The size pass is checked against the length of the CPU
oracle's blob and against what encode_v reports for the same message, in every message class, at
tuned, generic and mixed widths; the packed encode byte for byte against the oracle."""
import contextlib
import gc

import numpy as np
import pytest

from oracle.oracle import encode_bound
from tests import mapping_band_cases as mb
from tests.anyws_cases import low_pattern
from tests.support import CANARY, E_ARG, E_CAPACITY, E_CAPTURE, E_CONFIG, E_UNSUPPORTED, address_order, mask_of, offsets

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, i32, i64, make_codec, orc, own, packed_blobs, ptrs  # noqa: E402, F401
from tests.mixed_ws_cases import WIDTHS, batch, oracle_blob, records, run_vw  # noqa: E402, F401

pytestmark = pytest.mark.gpu

OPT_LARGE_MIN, OPT_TILE_CAP, OPT_PACK_SIZES_FIRST = 1, 2, 7


@pytest.fixture(autouse=True)
def _no_garbage_left():
    """A test that catches an exception leaves its contexts and tensors in a cycle with the traceback;
    they are collected here, not inside some later test's graph capture (see capture() below)."""
    yield
    gc.collect()


def sizes_v(codec, tensors, widths=None, mask=0):
    """encoded_sizes_v over `tensors`: (sizes, statuses) as host lists."""
    enc, st = codec.encoded_sizes_v(ptrs(tensors), i64(t.numel() for t in tensors),
                                    word_sizes=None if widths is None else i32(widths), width_mask=mask)
    torch.cuda.synchronize()
    return enc.cpu().numpy().tolist(), st.cpu().numpy().tolist()


# ------------------------------------------------------------------------------- 1: every class, every width
@pytest.mark.parametrize("order", ["ascending", "shuffled"])
def test_sizes_every_class_every_width(batch, order):
    idx = address_order(batch["tensors"], order)
    codec = make_codec(2)  # (the context's own width plays no part)
    enc, st = sizes_v(codec, [batch["tensors"][i] for i in idx], [batch["ws"][i] for i in idx], mask_of(WIDTHS))
    for k, i in enumerate(idx):
        what = "message %d (width %d, %d bytes)" % (i, batch["ws"][i], len(batch["msgs"][i]))
        assert enc[k] == len(batch["blobs"][i]), what   # the oracle's blob
        assert enc[k] == batch["sub"][i][1], what       # what encode_v reported
        assert st[k] == 0, what
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 2: one width per context
@pytest.mark.parametrize("w", WIDTHS)
def test_sizes_one_width_scattered_and_contiguous(batch, w):
    idx = [i for i, x in enumerate(batch["ws"]) if x == w]
    want = [len(batch["blobs"][i]) for i in idx]
    assert want == [batch["sub"][i][1] for i in idx]
    codec = make_codec(w)
    enc, st = sizes_v(codec, [batch["tensors"][i] for i in idx])
    assert (enc, st) == (want, [0] * len(idx))
    # the same messages back to back in one buffer (so at other alignments)
    data = torch.from_numpy(np.concatenate([batch["msgs"][i] for i in idx])).cuda()
    off = torch.from_numpy(offsets([len(batch["msgs"][i]) for i in idx])).cuda()
    enc, st = codec.encoded_sizes(data, off)
    torch.cuda.synchronize()
    assert enc.cpu().numpy().tolist() == want and st.cpu().numpy().tolist() == [0] * len(idx)
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 3: near ties
NEAR_WIDTHS = [4, 8, 2, 12]


def near_sizes(ws):
    return sorted(mb.sizes_for(ws))[:3] + ([mb.SIZE_TILED] if mb.SIZE_TILED in mb.sizes_for(ws) else [])


def blob_mapping(blob, ws):
    return [int.from_bytes(blob[20 + 4 * b:24 + 4 * b], "little") for b in range(ws)]


def other_mapping(case):
    """The mapping a decision that went the other way on this near tie gives: the positions nearest
    the mean change streams — the perturbed ones, or the others when those are fewer
    (mapping_band_cases: j perturbed positions lie (ws - j) / ws of the gap from the mean)."""
    ws, pert = case["ws"], set(case["perturbed"])
    near = pert if 2 * len(pert) >= ws else set(range(ws)) - pert
    return [m ^ 1 if b in near else m for b, m in enumerate(blob_mapping(case["blob"], ws))]


@pytest.fixture(scope="module")
def band_run(orc):
    """The mapping-band cases of four widths at their three smallest sizes and the tiled one: the
    oracle's blob, the size pass's answer and, for the near ties below the tiled size, whether the
    blob would have another length under the other mapping (on the CPU)."""
    cases = [c for c in mb.load_cases(build_messages=False) if c["ws"] in NEAR_WIDTHS and c["size"] in near_sizes(c["ws"])]
    for c in cases:
        c["input"] = mb.build(c)
        cfg = orc.config(word_size=c["ws"], sample_fraction=1.0)
        c["blob"] = orc.encode(c["input"], cfg=cfg)
        c["tells"] = False
        if c["kind"] != "tie" and c["size"] != mb.SIZE_TILED:
            c["tells"] = len(orc.encode(c["input"], cfg=cfg, mapping=other_mapping(c))) != len(c["blob"])
    for w in NEAR_WIDTHS:
        sub = [c for c in cases if c["ws"] == w]
        codec = make_codec(w)
        codec.set_option(OPT_LARGE_MIN, 65536)  # SIZE_TILED takes the tiles
        enc, st = sizes_v(codec, [own(c["input"]) for c in sub])
        for c, e, s in zip(sub, enc, st):
            c["got"] = (e, s)
        assert codec.error_flags() == 0
    return cases


@pytest.mark.parametrize("band", range(len(mb.BAND_NAMES)))
def test_sizes_near_ties_by_band(band_run, band):
    sub = [c for c in band_run if c["kind"] != "tie" and c["band"] == band]
    assert sub
    if not any(c["tells"] for c in sub):
        pytest.skip("no case of band %s changes its blob length under the other mapping" % mb.BAND_NAMES[band])
    bad = [c["name"] for c in sub if c["got"] != (len(c["blob"]), 0)]
    assert not bad, bad


def test_sizes_exact_ties_and_tiled_near_ties(band_run):
    assert any(c["size"] == mb.SIZE_TILED for c in band_run) and any(c["kind"] == "tie" for c in band_run)
    bad = [c["name"] for c in band_run if c["got"] != (len(c["blob"]), 0)]
    assert not bad, bad


# ------------------------------------------------------------------------------- 4: tiles, the cap across tiles
@pytest.mark.parametrize("w", [4, 2])
def test_sizes_tiled_runs_and_tile_budget_fallback(orc, w):
    n = mb.SIZE_TILED
    msgs = [np.full(n, 0x3C, np.uint8), low_pattern(n, np.random.default_rng(44))]
    want = [len(oracle_blob(orc, m, w)) for m in msgs]
    tensors = [own(m) for m in msgs]
    for tile_cap in (None, 8):  # 8: the messages' ten tiles are over the budget and stay whole
        codec = make_codec(w)
        codec.set_option(OPT_LARGE_MIN, 65536)
        if tile_cap:
            codec.set_option(OPT_TILE_CAP, tile_cap)
        for _ in range(2):  # (the second call plans from the first one's counts)
            assert sizes_v(codec, tensors) == (want, [0, 0]), tile_cap
        assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 5: history
def test_sizes_and_encode_share_one_history(batch):
    idx = [i for i, x in enumerate(batch["ws"]) if x == 4]
    tensors = [batch["tensors"][i] for i in idx]
    want = [len(batch["blobs"][i]) for i in idx]
    # no small and no UNCP message: above the one-wave class, and compressed
    big = [k for k, i in enumerate(idx) if len(batch["msgs"][i]) > 4096 and batch["blobs"][i][:4] == b"DTDT"]
    assert 0 < len(big) < len(idx)
    codec = make_codec(4)

    def encode():
        caps = [batch["caps"][i] for i in idx]
        outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
        ln, st = codec.encode_v(ptrs(tensors), i64(t.numel() for t in tensors), ptrs(outs), i64(caps))
        torch.cuda.synchronize()
        ln = ln.cpu().numpy()
        assert int(st.abs().sum()) == 0
        return [o[: ln[k]].cpu().numpy().tobytes() for k, o in enumerate(outs)]

    assert sizes_v(codec, tensors) == (want, [0] * len(idx))
    assert encode() == [batch["blobs"][i] for i in idx]
    assert sizes_v(codec, tensors) == (want, [0] * len(idx))
    for _ in range(2):  # twice: the second call runs with the small and copy classes switched off
        assert sizes_v(codec, [tensors[k] for k in big]) == ([want[k] for k in big], [0] * len(big))
    assert sizes_v(codec, tensors) == (want, [0] * len(idx))
    assert encode() == [batch["blobs"][i] for i in idx]
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 6: policy off
def test_sizes_with_compression_off(batch):
    tensors, n = batch["tensors"], len(batch["tensors"])
    codec = make_codec(4)
    codec.set_metrics(100.0, 1.0, 0.5)  # bandwidth at the threshold: should_transform says no
    want = [t.numel() + 4 for t in tensors]
    assert sizes_v(codec, tensors, batch["ws"], mask_of(WIDTHS)) == (want, [0] * n)
    assert sizes_v(codec, tensors) == (want, [0] * n)
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 7: rejected widths
def test_sizes_rejected_widths(orc):
    rng = np.random.default_rng(31)
    #        ok  <=0  ok  <=0  >64  not in mask  ok  ok
    widths = [4, 0, 2, -1, 65, 5, 4, 2]
    sizes = [4096, 4096, 32768, 1024, 65536, 4095, 32768, 1000]
    msgs = [records(rng, w if 1 <= w <= 64 else 4, n) for w, n in zip(widths, sizes)]
    want_st = [0, E_CONFIG, 0, E_CONFIG, E_UNSUPPORTED, E_ARG, 0, 0]
    want = [0 if s else len(oracle_blob(orc, m, w)) for m, w, s in zip(msgs, widths, want_st)]
    codec = make_codec(4)
    assert sizes_v(codec, [own(m) for m in msgs], widths, mask_of([2, 4])) == (want, want_st)
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 8: call-level errors
def test_sizes_call_level_errors():
    from psyne_amd._lib import TdtError
    t = own(records(np.random.default_rng(32), 4, 1024))
    codec = make_codec(4)
    for mask in (0, 0x1ff):  # no width; nine widths
        with pytest.raises(TdtError) as ei:
            codec.encoded_sizes_v(ptrs([t]), i64([1024]), word_sizes=i32([4]), width_mask=mask)
        assert ei.value.code == E_ARG
    p, n, w = ptrs([t]), i64([1024]), i32([4])
    enc = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    st = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    lib, h, s = codec._lib, codec._h, codec._stream(None)
    a = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    # null arrays with messages
    assert lib.tdt_encoded_sizes_v(h, None, a(n), None, 0, 1, a(enc), a(st), s) == E_ARG
    assert lib.tdt_encoded_sizes_v(h, a(p), None, None, 0, 1, a(enc), a(st), s) == E_ARG
    assert lib.tdt_encoded_sizes_v(h, a(p), a(n), None, 0, 1, None, a(st), s) == E_ARG
    assert lib.tdt_encoded_sizes_v(h, a(p), None, a(w), 0b1000, 1, a(enc), a(st), s) == E_ARG
    assert lib.tdt_encoded_sizes_v(h, a(p), a(n), a(w), 0b1000, 1, None, a(st), s) == E_ARG
    assert lib.tdt_encoded_sizes_batch(h, a(t), None, 1, a(enc), a(st), s) == E_ARG
    assert lib.tdt_encoded_sizes_batch(h, a(t), a(n), 1, None, a(st), s) == E_ARG
    # a batch without messages touches nothing, whatever else is passed
    assert lib.tdt_encoded_sizes_v(h, a(p), a(n), None, 0, 0, a(enc), a(st), s) == 0
    assert lib.tdt_encoded_sizes_v(h, a(p), a(n), a(w), 0, 0, a(enc), a(st), s) == 0
    assert lib.tdt_encoded_sizes_batch(h, a(t), a(n), 0, a(enc), a(st), s) == 0
    torch.cuda.synchronize()
    assert enc.cpu().numpy().tolist() == [77, 77] and st.cpu().numpy().tolist() == [77, 77]
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 9: capture
@contextlib.contextmanager
def capture(gr):
    """torch.cuda.graph(gr) behind a garbage collection.  torch.cuda.graph does not collect on entry,
    and an object the cyclic collector finalises INSIDE the capture window — the context or the
    failed graph of an earlier refused capture, kept alive by its exception's traceback — frees device
    memory and destroys streams in the middle of the capture (a run of this suite was aborted in a
    collection inside such a window)."""
    gc.collect()
    with torch.cuda.graph(gr):
        yield


class _Sized:
    """encoded_sizes_v over fixed tensors of widths 2, 4 and 12 (mixed), or all at width 12 (one width)."""
    WS = [2, 4, 12, 4, 2, 12, 4, 2]
    NS = [1000, 4096, 4104, 32768, 65536, 32784, 100000, 262208]

    def __init__(self, mixed):
        self.ws = self.WS if mixed else [12] * len(self.NS)
        self.c = make_codec(4 if mixed else 12)
        self.msgs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in self.NS]
        self.tab = [ptrs(self.msgs), i64(self.NS), i32(self.ws) if mixed else None]
        self.mask = mask_of(self.ws) if mixed else 0
        self.host = [None] * len(self.NS)
        # the results: the caller's tensors, so that a captured call allocates nothing
        self.enc = torch.zeros(len(self.NS), dtype=torch.int64, device="cuda")
        self.st = torch.zeros(len(self.NS), dtype=torch.int32, device="cuda")

    def fill(self, seed, which=None, constant=False):
        rng = np.random.default_rng(seed)
        for i, (w, n) in enumerate(zip(self.ws, self.NS)):
            m = np.full(n, seed, np.uint8) if constant else records(rng, w, n)
            if which is None or i in which:
                self.host[i] = m
                self.msgs[i].copy_(torch.from_numpy(m))

    def run(self):
        p, n, w = self.tab
        self.c.encoded_sizes_v(p, n, word_sizes=w, width_mask=self.mask, enc_sizes=self.enc, status=self.st)

    def want(self, orc):
        return [len(oracle_blob(orc, m, w)) for m, w in zip(self.host, self.ws)]

    def check(self, orc):
        torch.cuda.synchronize()
        assert self.enc.cpu().numpy().tolist() == self.want(orc)
        assert int(self.st.abs().sum()) == 0


@pytest.mark.parametrize("mixed", [False, True])
def test_sizes_capture_on_cold_context_is_refused(mixed):
    from psyne_amd._lib import TdtError
    s = _Sized(mixed)
    s.fill(4)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with pytest.raises(TdtError) as ei:
        with capture(gr):
            s.run()
    assert ei.value.code == E_CAPTURE
    del ei, gr, s  # (destroyed here, outside any capture, not whenever the collector finds the traceback's cycle)


@pytest.mark.parametrize("mixed", [False, True])
def test_sizes_capture_replays(orc, mixed):
    s = _Sized(mixed)
    s.fill(1)
    s.run()  # eager: the workspaces of this n_msgs (and mask) exist from here on
    s.check(orc)
    gr = torch.cuda.CUDAGraph()
    with capture(gr):
        s.run()
    for seed in (2, 3):
        before = s.want(orc)
        # two messages (whole records at either set of widths) change, and their sizes with them:
        # to one long run each, then back to records
        s.fill(seed, which=(2, 5), constant=seed == 2)
        after = s.want(orc)
        assert [i for i in range(len(before)) if before[i] != after[i]] == [2, 5]
        gr.replay()
        s.check(orc)
    assert s.c.error_flags() == 0


# ------------------------------------------------------------------------------- 10: sizes-first packed encode
def inside(cap, lead=1):
    """A `cap`-byte output `lead` bytes past a 16-byte boundary of a larger canary-filled allocation,
    so that with lead 1 the blobs of a packed buffer start at every alignment."""
    t = torch.full((64 + 16 + cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t, t[64 + lead:64 + lead + cap]


def canaries_around(t, view):
    h = t.cpu().numpy()
    b = view.data_ptr() - t.data_ptr()
    return bool((h[:b] == CANARY).all() and (h[b + view.numel():] == CANARY).all())


@pytest.mark.parametrize("w", [4, 12])
def test_sizes_first_vp_one_width(batch, w):
    idx = [i for i, x in enumerate(batch["ws"]) if x == w]
    n = len(idx)
    tensors = [batch["tensors"][i] for i in idx]
    sizes = [t.numel() for t in tensors]
    off_want = offsets([len(batch["blobs"][i]) for i in idx])
    cap = int(off_want[-1])  # exactly what the blobs need
    t, out = inside(cap)
    codec = make_codec(w)
    codec.set_option(OPT_PACK_SIZES_FIRST, 1)
    # total_bytes = 0: there is no scratch to size, so every blob is still written
    off, st = codec.encode_vp(ptrs(tensors), i64(sizes), 0, out)
    torch.cuda.synchronize()
    got, offh = packed_blobs(out, off)
    assert offh.tolist() == off_want.tolist()
    assert st.cpu().numpy()[:n].tolist() == [0] * n
    for k, i in enumerate(idx):
        assert got[k] == batch["blobs"][i] == batch["sub"][i][0], "message %d (%d bytes)" % (i, sizes[k])
    assert len({(out.data_ptr() + int(o)) % 16 for o in offh[:-1]}) >= 4 and out.data_ptr() % 2 == 1  # odd addresses too
    assert canaries_around(t, out)
    # and back, from the packed buffer as it is
    back = [torch.full((max(m, 1),), 1, dtype=torch.uint8, device="cuda")[:m] for m in sizes]
    dl, ds = codec.decode_tensors(out, off, off[1:] - off[:-1], back)
    torch.cuda.synchronize()
    assert int(ds.abs().sum()) == 0 and dl.cpu().numpy()[:n].tolist() == sizes
    for k, i in enumerate(idx):
        assert np.array_equal(back[k].cpu().numpy(), batch["msgs"][i]), "message %d" % i
    # the option back at 0: the two phases as before — with total_bytes = 0 their scratch holds the
    # first slots only, with the true total every blob
    codec.set_option(OPT_PACK_SIZES_FIRST, 0)
    t2, out2 = inside(cap)
    off2, st2 = codec.encode_vp(ptrs(tensors), i64(sizes), 0, out2)
    torch.cuda.synchronize()
    assert E_CAPACITY in st2.cpu().numpy()[:n].tolist() and canaries_around(t2, out2)
    off2, st2 = codec.encode_vp(ptrs(tensors), i64(sizes), sum(sizes), out2)
    torch.cuda.synchronize()
    assert st2.cpu().numpy()[:n].tolist() == [0] * n and off2.cpu().numpy().tolist() == off_want.tolist()
    assert np.array_equal(out2.cpu().numpy(), out.cpu().numpy()) and canaries_around(t2, out2)
    assert codec.error_flags() == 0


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
def test_sizes_first_vp_mixed_equals_encode_vw(batch, order):
    idx, outs, ln, vst, _ = run_vw(batch, order)
    n = len(idx)
    tensors = [batch["tensors"][i] for i in idx]
    sizes = [t.numel() for t in tensors]
    cap = int(sum(ln[:n]))
    t, out = inside(cap)
    codec = make_codec(2)  # (the context's own width plays no part)
    codec.set_option(OPT_PACK_SIZES_FIRST, 1)
    off, st = codec.encode_vp(ptrs(tensors), i64(sizes), 0, out, word_sizes=i32(batch["ws"][i] for i in idx),
                              width_mask=mask_of(WIDTHS))
    torch.cuda.synchronize()
    got, offh = packed_blobs(out, off)
    assert np.diff(offh).tolist() == ln[:n].tolist()
    assert st.cpu().numpy()[:n].tolist() == vst[:n].tolist() == [0] * n
    for k, i in enumerate(idx):
        assert got[k] == outs[k][: ln[k]].cpu().numpy().tobytes() == batch["blobs"][i], "message %d" % i
    assert canaries_around(t, out)
    assert codec.error_flags() == 0


def test_sizes_first_vp_rejected_widths_occupy_nothing(orc):
    rng = np.random.default_rng(41)
    widths = [4, 0, 2, -1, 65, 8, 4, 2]
    sizes = [4096, 4096, 32768, 1024, 65536, 4096, 32768, 1000]
    msgs = [records(rng, w if 1 <= w <= 64 else 4, n) for w, n in zip(widths, sizes)]
    want_st = [0, E_CONFIG, 0, E_CONFIG, E_UNSUPPORTED, E_ARG, 0, 0]
    want = [b"" if s else oracle_blob(orc, m, w) for m, w, s in zip(msgs, widths, want_st)]
    tensors = [own(m) for m in msgs]
    t, out = inside(sum(len(b) for b in want) + 100)
    codec = make_codec(4)
    codec.set_option(OPT_PACK_SIZES_FIRST, 1)
    off, st = codec.encode_vp(ptrs(tensors), i64(sizes), 0, out, word_sizes=i32(widths), width_mask=mask_of([2, 4]))
    torch.cuda.synchronize()
    got, offh = packed_blobs(out, off)
    assert st.cpu().numpy().tolist() == want_st
    assert got == want
    assert (out[int(offh[-1]):].cpu().numpy() == CANARY).all() and canaries_around(t, out)
    assert codec.error_flags() == 0


@pytest.mark.parametrize("where", ["at a blob's end", "one before", "one after", "zero"])
def test_sizes_first_vp_out_cap_cuts_the_batch(batch, where):
    idx = [i for i, x in enumerate(batch["ws"]) if x == 4]
    n = len(idx)
    tensors = [batch["tensors"][i] for i in idx]
    sizes = [t.numel() for t in tensors]
    off_want = offsets([len(batch["blobs"][i]) for i in idx])
    want = np.frombuffer(b"".join(batch["blobs"][i] for i in idx), np.uint8)
    k = n // 2
    cap = {"at a blob's end": int(off_want[k + 1]), "one before": int(off_want[k + 1]) - 1,
           "one after": int(off_want[k + 1]) + 1, "zero": 0}[where]
    t, out_full = inside(int(off_want[-1]))
    codec = make_codec(4)
    codec.set_option(OPT_PACK_SIZES_FIRST, 1)
    off, st = codec.encode_vp(ptrs(tensors), i64(sizes), 0, out_full[:cap])
    torch.cuda.synchronize()
    off, st = off.cpu().numpy(), st.cpu().numpy()
    assert off.tolist() == off_want.tolist()  # (off[n]: what the whole batch needs)
    fits = off[1:] <= cap
    fit = int(off[1:][fits].max()) if fits.any() else 0
    h = out_full.cpu().numpy()
    assert np.array_equal(h[:fit], want[:fit])   # the blobs that end inside out_cap, intact
    assert (h[fit:] == CANARY).all()             # and not a byte of any other
    assert fits.sum() == {"at a blob's end": k + 1, "one before": k, "one after": k + 1, "zero": 0}[where]
    assert st[:n].tolist() == [0 if f else E_CAPACITY for f in fits]
    assert canaries_around(t, out_full)
    assert codec.error_flags() == 0


class _SizesFirst:
    """The sizes-first encode_vp over fixed tensors of widths 2, 4 and 12."""
    WS = [2, 4, 12, 4, 2, 12, 4, 2]
    NS = [1000, 4096, 4104, 32768, 65536, 32784, 100000, 262208]

    def __init__(self):
        self.c = make_codec(4)
        self.c.set_option(OPT_PACK_SIZES_FIRST, 1)
        self.msgs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in self.NS]
        self.out = torch.zeros(sum(encode_bound(n, w) for n, w in zip(self.NS, self.WS)), dtype=torch.uint8, device="cuda")
        self.tab = [ptrs(self.msgs), i64(self.NS), i32(self.WS)]
        self.off = torch.zeros(len(self.NS) + 1, dtype=torch.int64, device="cuda")
        self.st = torch.zeros(len(self.NS), dtype=torch.int32, device="cuda")

    def fill(self, seed):
        rng = np.random.default_rng(seed)
        host = [records(rng, w, n) for w, n in zip(self.WS, self.NS)]
        for t, m in zip(self.msgs, host):
            t.copy_(torch.from_numpy(m))
        return host

    def run(self):
        p, n, w = self.tab
        self.c.encode_vp(p, n, 0, self.out, word_sizes=w, width_mask=mask_of(self.WS), out_offsets=self.off, status=self.st)

    def check(self, orc, host):
        torch.cuda.synchronize()
        got, _ = packed_blobs(self.out, self.off)
        assert int(self.st.abs().sum()) == 0
        for i, m in enumerate(host):
            assert got[i] == oracle_blob(orc, m, self.WS[i]), i


def test_sizes_first_vp_capture(orc):
    from psyne_amd._lib import TdtError
    cold = _SizesFirst()
    cold.fill(4)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with pytest.raises(TdtError) as ei:
        with capture(gr):
            cold.run()
    assert ei.value.code == E_CAPTURE
    del ei, gr, cold  # (destroyed here, outside any capture)
    s = _SizesFirst()
    host = s.fill(1)
    s.run()  # eager: the tables and the workspaces of this batch exist from here on
    s.check(orc, host)
    gr = torch.cuda.CUDAGraph()
    with capture(gr):
        s.run()
    for seed in (2, 3):
        host = s.fill(seed)
        gr.replay()
        s.check(orc, host)
    assert s.c.error_flags() == 0


# ------------------------------------------------------------------------------- 11: tensors
def test_encode_tensors_packed_exact(orc):
    g = torch.Generator(device="cuda")
    g.manual_seed(13)

    def sparse(n):
        return torch.randn(n, device="cuda", generator=g) * (torch.rand(n, device="cuda", generator=g) > 0.7)

    f32 = [sparse(n) for n in (1024, 16384, 80000)]
    tensors = f32 + [f32[1].to(torch.bfloat16), f32[2].to(torch.bfloat16), f32[1].to(torch.float64),
                     torch.zeros(0, dtype=torch.bfloat16, device="cuda"),
                     torch.rand(16384, device="cuda", generator=g),  # dense mantissas: a blob above its size
                     torch.randint(0, 4, (70001,), dtype=torch.uint8, device="cuda", generator=g)]
    raw = [t.contiguous().view(torch.uint8).cpu().numpy() if t.numel() else np.zeros(0, np.uint8) for t in tensors]
    want = [oracle_blob(orc, r, t.element_size()) for r, t in zip(raw, tensors)]
    codec = make_codec(4)
    out, off, st = codec.encode_tensors(tensors, word_sizes="dtype", packed=True, exact=True)
    torch.cuda.synchronize()
    assert off.numel() == len(tensors) + 1 and off.is_cuda
    assert out.numel() == int(off[-1]) == sum(len(b) for b in want)
    assert st.cpu().numpy().tolist() == [0] * len(tensors)
    got, offh = packed_blobs(out, off)
    assert offh.tolist() == offsets([len(b) for b in want]).tolist()
    assert got == want
    fresh = [torch.full_like(t, 1) for t in tensors]
    dl, ds = codec.decode_tensors(out, off, off[1:] - off[:-1], fresh)
    torch.cuda.synchronize()
    assert int(ds.abs().sum()) == 0
    for a, b in zip(tensors, fresh):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # every tensor at the context's width
    out4, off4, st4 = codec.encode_tensors(tensors, packed=True, exact=True)
    torch.cuda.synchronize()
    want4 = [oracle_blob(orc, r, 4) for r in raw]
    assert out4.numel() == int(off4[-1]) == sum(len(b) for b in want4) and int(st4.abs().sum()) == 0
    assert packed_blobs(out4, off4)[0] == want4
    with pytest.raises(ValueError):
        codec.encode_tensors(tensors, exact=True)  # (the slotted form has no exact variant)
    assert codec.error_flags() == 0
