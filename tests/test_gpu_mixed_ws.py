"""Mixed word sizes in one scattered batch on the GPU (tdt_encode_batch_vw, TdtCodec.encode_vw and
encode_tensors(word_sizes=...)): every message carries its own record width, and each blob, length
and status is what a context of that width gives — bit-exact against the CPU oracle at that width
and against encode_v on the width's sub-batch."""
import numpy as np
import pytest

from oracle.oracle import encode_bound
from tests.support import CANARY, E_ARG, E_CAPACITY, E_CAPTURE, E_CONFIG, E_UNSUPPORTED, mask_of

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, canaries_intact, guarded, i32, i64, make_codec, orc, own, ptrs  # noqa: E402, F401
from tests.mixed_ws_cases import batch, oracle_blob, records, run_vw  # noqa: E402, F401

pytestmark = pytest.mark.gpu


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
