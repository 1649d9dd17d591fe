"""Mixed word sizes in one scattered batch on the GPU (tdt_encode_batch_vw, TdtCodec.encode_vw and
encode_tensors(word_sizes=...)): every message carries its own record width, and each blob, length
and status is what a context of that width gives — bit-exact against the CPU oracle at that width
and against encode_v on the width's sub-batch."""
import numpy as np
import pytest

from oracle.oracle import Oracle, encode_bound
from tests.anyws_cases import from_streams, low_pattern

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_CAPACITY, E_UNSUPPORTED, E_CONFIG, E_ARG, E_CAPTURE = 5, 6, 8, 11, 12
CANARY = 0xA5
WIDTHS = [1, 2, 4, 8, 16, 3, 12]
# the smallest sizes that reach the UNCP copy (0, 3, 64, 1000: below min_tensor), the one-wave
# (<= 4 KiB), 256-lane (<= 32 KiB), resident 512-lane (<= 64 KiB, aligned) and streaming classes and,
# in so small a batch, the tiles (> 256 KiB).  4104, 32784, 65544 and 100008 are multiples of 12;
# 4104 is no multiple of 16 (the per-message n % ws fallback)
SIZES = [0, 3, 64, 1000, 1024, 4096, 4104, 4112, 32768, 32784, 65536, 65544, 65552, 100000, 100008, 262208]
LEADS = {4112: 1, 32784: 4, 65552: 8, 100000: 15}  # views this many bytes into their allocation


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from psyne_amd import _lib
    _lib.load()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def make_codec(ws=4):
    from psyne_amd import TDTConfig, TdtCodec
    c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws))
    c.set_metrics(10.0, 1.0, 0.5)
    return c


def mask_of(widths):
    m = 0
    for w in set(widths):
        m |= 1 << (w - 1)
    return m


def records(rng, ws, n):
    """n bytes of ws-byte records whose byte positions differ in entropy (both streams populated
    from width 2 up); sizes that hold no whole number of records, and width 1, get few-valued bytes."""
    if ws > 1 and n >= ws and n % ws == 0:
        wc = n // ws
        return from_streams(ws, wc, low_pattern(wc * ws, rng), rng)
    return rng.integers(0, 4, n, dtype=np.uint8)


def own(data, lead=0):
    """`data` in a device allocation of its own, `lead` bytes into it."""
    data = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    t = torch.empty(lead + data.size + 16, dtype=torch.uint8, device="cuda")
    v = t[lead:lead + data.size]
    if data.size:
        v.copy_(torch.from_numpy(np.ascontiguousarray(data)))
    return v


def guarded(cap):
    """A `cap`-byte output inside a larger allocation, 64 canary bytes on either side."""
    t = torch.full((64 + cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    return t, t[64:64 + cap]


def canaries_intact(t, cap):
    h = t.cpu().numpy()
    return bool((h[:64] == CANARY).all() and (h[64 + cap:] == CANARY).all())


def i64(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64, device="cuda")


def i32(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device="cuda")


def ptrs(tensors):
    return i64(t.data_ptr() if t.numel() else 0 for t in tensors)


def oracle_blob(orc, m, w):
    return orc.encode(m, cfg=orc.config(sample_fraction=1.0, word_size=w))


def encode_v_sub(ws, tensors, caps):
    """encode_v on a context of width ws: (blobs as bytes, lengths, statuses)."""
    outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    codec = make_codec(ws)
    ln, st = codec.encode_v(ptrs(tensors), i64(t.numel() for t in tensors), ptrs(outs), i64(caps))
    torch.cuda.synchronize()
    ln, st = ln.cpu().numpy()[: len(tensors)], st.cpu().numpy()[: len(tensors)]
    assert codec.error_flags() == 0
    return [o[: ln[k]].cpu().numpy().tobytes() for k, o in enumerate(outs)], ln, st


@pytest.fixture(scope="module")
def batch(orc):
    """Every size at every width, the widths interleaved message by message; the oracle's blobs; and
    per width what encode_v on a context of that width gives for the width's sub-batch."""
    rng = np.random.default_rng(20261)
    ws, msgs, leads = [], [], []
    for k, n in enumerate(SIZES):
        for j, w in enumerate(WIDTHS):
            ws.append(w)
            msgs.append(records(rng, w, n))
            leads.append(LEADS.get(n, 0) if (j + k) % 2 == 0 else 0)
    ws += [2, 8]
    msgs += [np.full(32768, 0x3C, np.uint8), rng.integers(0, 256, 65536, dtype=np.uint8)]  # constant, uniform random
    leads += [0, 0]
    blobs = [oracle_blob(orc, m, w) for m, w in zip(msgs, ws)]
    tensors = [own(m, lead) for m, lead in zip(msgs, leads)]
    caps = [encode_bound(len(m), w) for m, w in zip(msgs, ws)]
    sub = {}
    for w in WIDTHS:
        idx = [i for i, x in enumerate(ws) if x == w]
        b, ln, st = encode_v_sub(w, [tensors[i] for i in idx], [caps[i] for i in idx])
        for k, i in enumerate(idx):
            sub[i] = (b[k], int(ln[k]), int(st[k]))
    return dict(ws=ws, msgs=msgs, blobs=blobs, tensors=tensors, caps=caps, sub=sub, runs={})


def address_order(tensors, order):
    idx = sorted(range(len(tensors)), key=lambda i: tensors[i].data_ptr())
    if order == "shuffled":
        np.random.default_rng(7).shuffle(idx)
    return idx


def run_vw(batch, order):
    """One encode_vw call over the whole batch in the given address order (kept for the round trip)."""
    if order not in batch["runs"]:
        idx = address_order(batch["tensors"], order)
        tensors = [batch["tensors"][i] for i in idx]
        caps = [batch["caps"][i] for i in idx]
        outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
        codec = make_codec(4)
        ln, st = codec.encode_vw(ptrs(tensors), i64(t.numel() for t in tensors), i32(batch["ws"][i] for i in idx),
                                 mask_of(WIDTHS), ptrs(outs), i64(caps))
        torch.cuda.synchronize()
        flags = codec.error_flags()
        batch["runs"][order] = (idx, outs, ln.cpu().numpy(), st.cpu().numpy(), flags)
    return batch["runs"][order]


# ------------------------------------------------------------------------------- 1: every class, every width
@pytest.mark.parametrize("order", ["ascending", "shuffled"])
def test_encode_vw_every_class_every_width(batch, order):
    idx, outs, ln, st, flags = run_vw(batch, order)
    for k, i in enumerate(idx):
        what = "message %d (width %d, %d bytes)" % (i, batch["ws"][i], len(batch["msgs"][i]))
        got = outs[k][: ln[k]].cpu().numpy().tobytes()
        assert st[k] == 0 and got == batch["blobs"][i], what
        sb, sl, ss = batch["sub"][i]
        assert (got, int(ln[k]), int(st[k])) == (sb, sl, ss), what
    assert flags == 0


# ------------------------------------------------------------------------------- 2: round trip
def test_decode_v_restores_mixed_blobs(batch):
    idx, outs, ln, st, _ = run_vw(batch, "ascending")
    sizes = [len(batch["msgs"][i]) for i in idx]
    back = [torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda") for n in sizes]
    codec = make_codec(4)
    dl, ds = codec.decode_v(ptrs(outs), i64(ln[: len(idx)]), ptrs(back), i64(sizes))
    torch.cuda.synchronize()
    assert int(ds.abs().sum()) == 0 and dl.cpu().numpy().tolist() == sizes
    for k, i in enumerate(idx):
        assert np.array_equal(back[k].cpu().numpy()[: sizes[k]], batch["msgs"][i]), "message %d" % i
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 3: rejections and capacities
def test_rejected_widths_and_short_capacity(orc):
    rng = np.random.default_rng(31)
    #        ok  <=0  ok  <=0  >64  not in mask  one byte short  ok
    widths = [4, 0, 2, -1, 65, 8, 4, 2]
    sizes = [4096, 4096, 32768, 1024, 65536, 4096, 32768, 1000]
    msgs = [records(rng, w if 1 <= w <= 64 else 4, n) for w, n in zip(widths, sizes)]
    blobs = [oracle_blob(orc, m, w) if w in (2, 4) else b"" for m, w in zip(msgs, widths)]
    caps = [encode_bound(n, 8) for n in sizes]
    caps[6] = len(blobs[6]) - 1
    want_st = [0, E_CONFIG, 0, E_CONFIG, E_UNSUPPORTED, E_ARG, E_CAPACITY, 0]
    tensors = [own(m) for m in msgs]
    outs = [guarded(c) for c in caps]
    codec = make_codec(4)
    ln = torch.full((len(msgs),), 77, dtype=torch.int64, device="cuda")
    st = torch.full((len(msgs),), 77, dtype=torch.int32, device="cuda")
    codec.encode_vw(ptrs(tensors), i64(sizes), i32(widths), mask_of([2, 4]), ptrs([v for _, v in outs]), i64(caps),
                    lengths=ln, status=st)
    torch.cuda.synchronize()
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    assert st.tolist() == want_st
    for i, (t, v) in enumerate(outs):
        assert canaries_intact(t, caps[i]), "message %d" % i
        if want_st[i]:
            assert ln[i] == 0 and (v.cpu().numpy() == CANARY).all(), "message %d" % i
        else:
            assert v[: ln[i]].cpu().numpy().tobytes() == blobs[i], "message %d" % i
    assert codec.error_flags() == 0


def test_call_level_mask_errors(orc):
    from psyne_amd._lib import TdtError
    msg = records(np.random.default_rng(32), 4, 1024)
    t = own(msg)
    out = torch.zeros(encode_bound(1024, 4), dtype=torch.uint8, device="cuda")
    codec = make_codec(4)
    args = (ptrs([t]), i64([1024]), i32([4]))
    for mask in (0, 0x1ff):  # no width; nine widths
        with pytest.raises(TdtError) as ei:
            codec.encode_vw(*args, mask, ptrs([out]), i64([out.numel()]))
        assert ei.value.code == E_ARG
    ln, st = codec.encode_vw(*args, 0xff, ptrs([out]), i64([out.numel()]))  # eight widths
    torch.cuda.synchronize()
    assert int(st[0]) == 0 and out[: int(ln[0])].cpu().numpy().tobytes() == oracle_blob(orc, msg, 4)
    # a batch without messages touches nothing, whatever the mask
    e = torch.empty(0, dtype=torch.int64, device="cuda")
    codec.encode_vw(e, e, torch.empty(0, dtype=torch.int32, device="cuda"), 0, e, e)


# ------------------------------------------------------------------------------- 4: one width only
@pytest.mark.parametrize("w", [4, 12])
def test_single_width_equals_encode_v(batch, w):
    idx = [i for i, x in enumerate(batch["ws"]) if x == w]
    tensors, caps = [batch["tensors"][i] for i in idx], [batch["caps"][i] for i in idx]
    outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    codec = make_codec(2)  # (the context's own width plays no part)
    ln, st = codec.encode_vw(ptrs(tensors), i64(t.numel() for t in tensors), i32([w] * len(idx)), mask_of([w]),
                             ptrs(outs), i64(caps))
    torch.cuda.synchronize()
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    assert ln[: len(idx)].tolist() == [batch["sub"][i][1] for i in idx]
    assert st[: len(idx)].tolist() == [batch["sub"][i][2] for i in idx]
    for k, i in enumerate(idx):
        assert outs[k][: ln[k]].cpu().numpy().tobytes() == batch["sub"][i][0] == batch["blobs"][i], "message %d" % i
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 5: history
def test_histories_per_width_and_context_history_untouched(orc):
    rng = np.random.default_rng(55)
    codec = make_codec(4)

    def vw(widths, sizes):
        msgs = [records(rng, w, n) for w, n in zip(widths, sizes)]
        tensors = [own(m) for m in msgs]
        caps = [encode_bound(n, w) for w, n in zip(widths, sizes)]
        outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
        ln, st = codec.encode_vw(ptrs(tensors), i64(sizes), i32(widths), mask_of([2, 4, 8]), ptrs(outs), i64(caps))
        torch.cuda.synchronize()
        ln = ln.cpu().numpy()
        assert int(st.abs().sum()) == 0
        for i, (m, w) in enumerate(zip(msgs, widths)):
            assert outs[i][: ln[i]].cpu().numpy().tobytes() == oracle_blob(orc, m, w), "message %d (width %d)" % (i, w)

    plain_msgs = [records(rng, 4, n) for n in (1000, 2048, 20000, 65536, 70000)]
    plain = [own(m) for m in plain_msgs]
    pcaps = [encode_bound(t.numel(), 4) for t in plain]

    def v():
        outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in pcaps]
        ln, st = codec.encode_v(ptrs(plain), i64(t.numel() for t in plain), ptrs(outs), i64(pcaps))
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0
        ln = ln.cpu().numpy()
        return [o[: ln[k]].cpu().numpy().tobytes() for k, o in enumerate(outs)]

    before = v()
    assert before == [oracle_blob(orc, m, 4) for m in plain_msgs]
    a_w, a_n = [2] * 6 + [4] * 4, [1024, 2048, 4096, 1024, 2048, 4096] + [65536] * 4
    vw(a_w, a_n)  # A: only small width-2 and only 64 KiB width-4 messages
    vw(a_w, a_n)  # A again: every other class, and width 8, are recorded empty
    # B: width 8 appears, and the size classes swap between widths 2 and 4
    vw([2] * 4 + [4] * 6 + [8] * 3, [65536] * 4 + [1024, 2048, 4096, 1024, 2048, 4096] + [1024, 20000, 65536])
    assert v() == before
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 6: capture
class _Mixed:
    """encode_vw over fixed tensors of widths 2, 4 and 12."""
    WS = [2, 4, 12, 4, 2, 12, 4, 2]
    NS = [1000, 4096, 4104, 32768, 65536, 32784, 100000, 262208]

    def __init__(self):
        self.c = make_codec(4)
        self.msgs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in self.NS]
        caps = [encode_bound(n, w) for n, w in zip(self.NS, self.WS)]
        self.enc = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
        self.tab = [ptrs(self.msgs), i64(self.NS), i32(self.WS), ptrs(self.enc), i64(caps)]
        self.elen = torch.zeros(len(self.NS), dtype=torch.int64, device="cuda")
        self.est = torch.zeros(len(self.NS), dtype=torch.int32, device="cuda")

    def fill(self, seed):
        rng = np.random.default_rng(seed)
        host = [records(rng, w, n) for w, n in zip(self.WS, self.NS)]
        for t, m in zip(self.msgs, host):
            t.copy_(torch.from_numpy(m))
        return host

    def run(self):
        p, n, w, e, cap = self.tab
        self.c.encode_vw(p, n, w, mask_of(self.WS), e, cap, lengths=self.elen, status=self.est)

    def check(self, orc, host):
        torch.cuda.synchronize()
        ln = self.elen.cpu().numpy()
        assert int(self.est.abs().sum()) == 0
        for i, m in enumerate(host):
            assert self.enc[i][: ln[i]].cpu().numpy().tobytes() == oracle_blob(orc, m, self.WS[i]), i


def test_capture_on_cold_context_is_refused():
    from psyne_amd._lib import TdtError
    s = _Mixed()
    s.fill(4)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with pytest.raises(TdtError) as ei:
        with torch.cuda.graph(gr):
            s.run()
    assert ei.value.code == E_CAPTURE


def test_capture_replays(orc):
    s = _Mixed()
    host = s.fill(1)
    s.run()  # eager: the workspaces of this n_msgs and mask exist from here on
    s.check(orc, host)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        s.run()
    for seed in (2, 3):
        host = s.fill(seed)
        gr.replay()
        s.check(orc, host)
    assert s.c.error_flags() == 0


# ------------------------------------------------------------------------------- 7: tensors
def test_encode_tensors_by_dtype(orc):
    g = torch.Generator(device="cuda")
    g.manual_seed(12)

    def sparse(n):
        return torch.randn(n, device="cuda", generator=g) * (torch.rand(n, device="cuda", generator=g) > 0.7)

    f32 = [sparse(n) for n in (1024, 16384, 80000)]
    tensors = f32 + [f32[1].to(torch.bfloat16), f32[2].to(torch.bfloat16), f32[1].to(torch.float16),
                     f32[1].to(torch.float64), (f32[1] * 1000).to(torch.int64),
                     torch.randint(0, 4, (70001,), dtype=torch.uint8, device="cuda", generator=g),  # 70001 % 4 != 0
                     torch.zeros(0, dtype=torch.float16, device="cuda"),
                     f32[0].to(torch.bfloat16)[:1001]]  # 2002 bytes: no multiple of 4
    raw = [t.contiguous().view(torch.uint8).cpu().numpy() if t.numel() else np.zeros(0, np.uint8) for t in tensors]
    codec = make_codec(4)
    out, slots, ln, st = codec.encode_tensors(tensors, word_sizes="dtype")
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    oh, sl, lh = out.cpu().numpy(), slots.cpu().numpy(), ln.cpu().numpy()
    bounds = [encode_bound(r.size, t.element_size()) for r, t in zip(raw, tensors)]
    assert sl.tolist() == np.concatenate([[0], np.cumsum(bounds)]).tolist()
    for i, (r, t) in enumerate(zip(raw, tensors)):
        want = oracle_blob(orc, r, t.element_size())
        assert oh[sl[i]:sl[i] + lh[i]].tobytes() == want, "tensor %d (%s)" % (i, t.dtype)
    fresh = [torch.full_like(t, 1) for t in tensors]
    dl, ds = codec.decode_tensors(out, slots, ln, fresh)
    torch.cuda.synchronize()
    assert int(ds.abs().sum()) == 0
    for a, b in zip(tensors, fresh):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # one width per tensor, as ints: the same call
    out2, _, ln2, _ = codec.encode_tensors(tensors, word_sizes=[t.element_size() for t in tensors])
    torch.cuda.synchronize()
    assert torch.equal(ln2[: len(tensors)], ln[: len(tensors)]) and torch.equal(out2, out)
    # the default call: every tensor at the context's width, as before
    out4, sl4, ln4, st4 = codec.encode_tensors(tensors)
    torch.cuda.synchronize()
    assert int(st4.abs().sum()) == 0
    oh, sl, lh = out4.cpu().numpy(), sl4.cpu().numpy(), ln4.cpu().numpy()
    for i, r in enumerate(raw):
        assert oh[sl[i]:sl[i] + lh[i]].tobytes() == oracle_blob(orc, r, 4), "tensor %d at width 4" % i
    assert codec.error_flags() == 0
    with pytest.raises(ValueError):
        codec.encode_tensors(tensors, word_sizes=[4])
    with pytest.raises(ValueError):
        codec.encode_tensors(tensors[:2], word_sizes=[4, 65])
