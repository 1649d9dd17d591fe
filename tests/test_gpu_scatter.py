"""Scattered batches on the GPU (tdt_encode_batch_v / tdt_decode_batch_v / tdt_decoded_sizes_v and the
tensor API above them): every message and every result in its own allocation, at any alignment
and in any address order.  Bit-exact against the CPU oracle, and per message the same status and
length as the slotted calls give on the packed batch."""
import numpy as np
import pytest

from oracle.oracle import encode_bound
from tests.support import CANARY, E_CAPACITY, E_CAPTURE, E_MAGIC, E_TRUNCATED, address_order, gradient

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, canaries_intact, guarded, i64, make_codec, orc, own, ptrs  # noqa: E402, F401

pytestmark = pytest.mark.gpu

# the smallest sizes that reach every encode class: UNCP copies (0, 3, 64 and 1000 are below
# min_tensor), one-wave teams (<= 4 KiB), 256-lane teams (<= 32 KiB), 512-lane resident teams
# (<= 64 KiB, aligned), the streaming list (longer, or unaligned) and, in so small a batch, tiles
# (> 256 KiB)
SIZES = [0, 3, 64, 1000, 1024, 4096, 4112, 32768, 32784, 65536, 65552, 100000, 262144 + 64]
LEADS = [(4112, 1), (32784, 4), (65552, 8), (100000, 15)]  # views this many bytes into an allocation


def message(rng, n):
    return gradient(rng, n) if n % 4 == 0 and n >= 64 else rng.integers(0, 256, n, dtype=np.uint8)


def pack(chunks):
    off = np.zeros(len(chunks) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in chunks])
    buf = np.concatenate([np.frombuffer(bytes(c), np.uint8) for c in chunks] + [np.zeros(1, np.uint8)])
    return torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda(), off


@pytest.fixture(scope="module")
def batch(orc):
    """The messages of tests 1, 4 and 5, their oracle blobs, and what encode_into gives on the packed batch."""
    rng = np.random.default_rng(20260)
    msgs = [message(rng, n) for n in SIZES]
    leads = [0] * len(msgs)
    msgs.append(np.full(32768, 0x3C, np.uint8))                      # constant
    msgs.append(rng.integers(0, 256, 65536, dtype=np.uint8))         # uniform random
    leads += [0, 0]
    for n, lead in LEADS:
        msgs.append(message(rng, n))
        leads.append(lead)
    cfg = orc.config(sample_fraction=1.0)
    blobs = [orc.encode(m, cfg=cfg, bandwidth=10.0) for m in msgs]
    tensors = [own(m, lead) for m, lead in zip(msgs, leads)]
    twice = SIZES.index(65536)                                       # one tensor listed twice
    msgs.append(msgs[twice]), blobs.append(blobs[twice]), tensors.append(tensors[twice])
    d, o, _ = pack(msgs)
    codec = make_codec()
    _, _, ln, st = codec.encode_into(d, o)
    torch.cuda.synchronize()
    return dict(msgs=msgs, blobs=blobs, tensors=tensors, packed_len=ln.cpu().numpy()[: len(msgs)],
                packed_st=st.cpu().numpy()[: len(msgs)])


# ------------------------------------------------------------------------------- 1: encode classes
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_encode_v_every_class(batch, order):
    idx = address_order(batch["tensors"], order)
    tensors = [batch["tensors"][i] for i in idx]
    caps = [encode_bound(t.numel(), 4) for t in tensors]
    outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    codec = make_codec()
    ln, st = codec.encode_v(ptrs(tensors), i64(t.numel() for t in tensors), ptrs(outs), i64(caps))
    torch.cuda.synchronize()
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    for k, i in enumerate(idx):
        assert st[k] == batch["packed_st"][i] == 0 and ln[k] == batch["packed_len"][i], "message %d" % i
        assert outs[k][: ln[k]].cpu().numpy().tobytes() == batch["blobs"][i], "message %d (%d bytes)" % (
            i, len(batch["msgs"][i]))
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 2: headline shape
def test_encode_v_headline_shape(orc):
    rng = np.random.default_rng(3)
    msgs = [gradient(rng, 65536) for _ in range(256)]
    tensors = [own(m) for m in msgs]
    cap = encode_bound(65536, 4)
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in msgs]
    codec = make_codec()
    ln, st = codec.encode_v(ptrs(tensors), i64([65536] * 256), ptrs(outs), i64([cap] * 256))
    torch.cuda.synchronize()
    ln = ln.cpu().numpy()
    assert int(st.abs().sum()) == 0
    cfg = orc.config(sample_fraction=1.0)
    for i, m in enumerate(msgs):
        assert outs[i][: ln[i]].cpu().numpy().tobytes() == orc.encode(m, cfg=cfg, bandwidth=10.0), "message %d" % i
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 3: generic widths
@pytest.mark.parametrize("ws", [3, 12])
def test_encode_v_generic_width(orc, ws):
    rng = np.random.default_rng(100 + ws)
    sizes = [12 * k for k in (86, 340, 341, 342, 343, 1000)] + [4100]  # 4100: not whole words, UNCP
    msgs = [rng.integers(0, 4, n, dtype=np.uint8) for n in sizes]
    tensors = [own(m, lead=i % 4) for i, m in enumerate(msgs)]
    caps = [encode_bound(n, ws) for n in sizes]
    outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    codec = make_codec(ws)
    ln, st = codec.encode_v(ptrs(tensors), i64(sizes), ptrs(outs), i64(caps))
    torch.cuda.synchronize()
    ln = ln.cpu().numpy()
    assert int(st.abs().sum()) == 0
    cfg = orc.config(word_size=ws, sample_fraction=1.0)
    for i, m in enumerate(msgs):
        want = orc.encode(m, cfg=cfg, bandwidth=10.0)
        assert outs[i][: ln[i]].cpu().numpy().tobytes() == want, "size %d" % sizes[i]
    assert want[:4] == b"PCNU"  # (the last one stayed UNCP)
    # and back, through the deferred generic decode of a scattered batch
    back = [torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda") for n in sizes]
    dl, ds = codec.decode_v(ptrs(outs), i64(ln), ptrs(back), i64(sizes))
    torch.cuda.synchronize()
    assert int(ds.abs().sum()) == 0 and dl.cpu().numpy().tolist() == sizes
    for i, m in enumerate(msgs):
        assert np.array_equal(back[i].cpu().numpy()[: sizes[i]], m)


@pytest.mark.parametrize("ws", [1, 2, 8, 16])
def test_round_trip_v_other_tuned_widths(orc, ws):
    """The scattered instances of the other tuned word sizes: one message per class, there and back."""
    rng = np.random.default_rng(200 + ws)
    sizes = [1000, 1024, 4112, 32768, 32784, 65552, 262144 + 64]
    msgs = [message(rng, n) for n in sizes]
    tensors = [own(m, lead=(i % 2) * 16) for i, m in enumerate(msgs)]
    caps = [encode_bound(n, ws) for n in sizes]
    outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    back = [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in sizes]
    codec = make_codec(ws)
    ln, st = codec.encode_v(ptrs(tensors), i64(sizes), ptrs(outs), i64(caps))
    dl, ds = codec.decode_v(ptrs(outs), ln, ptrs(back), i64(sizes))
    torch.cuda.synchronize()
    ln = ln.cpu().numpy()
    assert int(st.abs().sum()) == 0 and int(ds.abs().sum()) == 0 and dl.cpu().numpy().tolist() == sizes
    cfg = orc.config(word_size=ws, sample_fraction=1.0)
    for i, m in enumerate(msgs):
        assert outs[i][: ln[i]].cpu().numpy().tobytes() == orc.encode(m, cfg=cfg, bandwidth=10.0), "size %d" % sizes[i]
        assert np.array_equal(back[i].cpu().numpy(), m), "size %d" % sizes[i]
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 4, 5: decode
@pytest.fixture(scope="module")
def dbatch(orc, batch):
    """Blobs of every decode class (+ error blobs), each in its own allocation at byte phases 0..3,
    and what decoded_sizes / decode_into give on the packed blobs."""
    rng = np.random.default_rng(77)
    msgs = list(batch["msgs"])
    blobs = list(batch["blobs"])
    cfg = orc.config(sample_fraction=1.0)
    for n in (160 * 1024, 288 * 1024):  # decoding to > 128 KiB (dispatched first) and > 256 KiB (tiled)
        msgs.append(gradient(rng, n))
        blobs.append(orc.encode(msgs[-1], cfg=cfg, bandwidth=10.0))
    m12 = rng.integers(0, 4, 6000, dtype=np.uint8)  # a word-size-12 blob inside the word-size-4 context
    msgs.append(m12)
    blobs.append(orc.encode(m12, cfg=orc.config(word_size=12, sample_fraction=1.0), bandwidth=10.0))
    good = len(blobs)
    blobs.append(blobs[SIZES.index(4096)][:-7])   # truncated
    blobs.append(b"\x11\x22\x33\x44" + bytes(60))  # bad magic
    msgs += [np.zeros(0, np.uint8)] * 2
    tensors = [own(b, lead=i % 4) for i, b in enumerate(blobs)]
    d, o, _ = pack(blobs)
    codec = make_codec()
    sz, sst = codec.decoded_sizes(d, o)
    _, _, ln, st = codec.decode_into(d, o)
    torch.cuda.synchronize()
    n = len(blobs)
    ref = dict(sizes=sz.cpu().numpy()[:n], sizes_st=sst.cpu().numpy()[:n], len=ln.cpu().numpy()[:n],
               st=st.cpu().numpy()[:n])
    assert ref["st"][good:].tolist() == [E_TRUNCATED, E_MAGIC] and not ref["st"][:good].any()
    return dict(msgs=msgs, blobs=blobs, tensors=tensors, good=good, ref=ref)


def _decode_v(dbatch, short=()):
    msgs, tensors = dbatch["msgs"], dbatch["tensors"]
    caps = [len(m) - (1 if i in short else 0) for i, m in enumerate(msgs)]
    caps[-1] = 16  # (an error blob with room: still nothing is written)
    outs = [guarded(c) for c in caps]
    codec = make_codec()
    ln, st = codec.decode_v(ptrs(tensors), i64(len(b) for b in dbatch["blobs"]), ptrs([v for _, v in outs]), i64(caps))
    torch.cuda.synchronize()
    assert codec.error_flags() == 0
    return outs, caps, ln.cpu().numpy(), st.cpu().numpy()


def test_decode_v_every_class(dbatch):
    outs, caps, ln, st = _decode_v(dbatch)
    ref = dbatch["ref"]
    for i, m in enumerate(dbatch["msgs"]):
        assert st[i] == ref["st"][i] and ln[i] == ref["len"][i], "blob %d" % i
        assert canaries_intact(outs[i][0], caps[i]), "blob %d" % i
        if i < dbatch["good"]:
            assert ln[i] == len(m) and np.array_equal(outs[i][1].cpu().numpy(), m), "blob %d" % i
    assert (outs[-1][1].cpu().numpy() == CANARY).all()  # the error blob's output is untouched


def test_decode_v_short_capacity(dbatch):
    short = [SIZES.index(1000), SIZES.index(65536), SIZES.index(262144 + 64)]  # a copy, a one-wave blob, a tiled one
    outs, caps, ln, st = _decode_v(dbatch, short)
    for i, m in enumerate(dbatch["msgs"]):
        assert canaries_intact(outs[i][0], caps[i]), "blob %d" % i
        if i in short:
            assert st[i] == E_CAPACITY and ln[i] == 0, "blob %d" % i
        elif i < dbatch["good"]:
            assert st[i] == 0 and ln[i] == len(m) and np.array_equal(outs[i][1].cpu().numpy(), m), "blob %d" % i


def test_encode_v_short_capacity(batch):
    short = [SIZES.index(1000), SIZES.index(32768), SIZES.index(262144 + 64)]  # a copy, a resident team, tiles
    tensors, blobs = batch["tensors"], batch["blobs"]
    caps = [len(b) - 1 if i in short else encode_bound(t.numel(), 4) for i, (t, b) in enumerate(zip(tensors, blobs))]
    outs = [guarded(c) for c in caps]
    codec = make_codec()
    ln, st = codec.encode_v(ptrs(tensors), i64(t.numel() for t in tensors), ptrs([v for _, v in outs]), i64(caps))
    torch.cuda.synchronize()
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    for i, b in enumerate(blobs):
        assert canaries_intact(outs[i][0], caps[i]), "message %d" % i
        if i in short:
            assert st[i] == E_CAPACITY and ln[i] == 0, "message %d" % i
        else:
            assert st[i] == 0 and outs[i][1][: ln[i]].cpu().numpy().tobytes() == b, "message %d" % i
    assert codec.error_flags() == 0


def test_decoded_sizes_v(dbatch):
    codec = make_codec()
    sz, st = codec.decoded_sizes_v(ptrs(dbatch["tensors"]), i64(len(b) for b in dbatch["blobs"]))
    torch.cuda.synchronize()
    assert sz.cpu().numpy().tolist() == dbatch["ref"]["sizes"].tolist()
    assert st.cpu().numpy().tolist() == dbatch["ref"]["sizes_st"].tolist()
    assert sz.cpu().numpy()[: dbatch["good"]].tolist() == [len(m) for m in dbatch["msgs"][: dbatch["good"]]]


# ------------------------------------------------------------------------------- 6: tensor API
def test_tensor_round_trip():
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    f32 = [torch.randn(n, device="cuda", generator=g) * (torch.rand(n, device="cuda", generator=g) > 0.7)
           for n in (16, 1024, 16384, 80000)]
    f16 = [t.to(torch.float16) for t in (f32[1], f32[2])] + [torch.zeros(4096, dtype=torch.float16, device="cuda")]
    u8 = [torch.randint(0, 4, (n,), dtype=torch.uint8, device="cuda", generator=g) for n in (0, 5, 2048, 70001)]
    tensors = f32 + f16 + u8 + [f32[2].view(128, 128)]
    codec = make_codec()
    out, slots, ln, st = codec.encode_tensors(tensors)
    assert int(st.abs().sum()) == 0
    fresh = [torch.full_like(t, 1) for t in tensors]
    dl, ds = codec.decode_tensors(out, slots, ln, fresh)
    torch.cuda.synchronize()
    assert int(ds.abs().sum()) == 0
    assert dl.cpu().numpy().tolist() == [t.numel() * t.element_size() for t in tensors]
    for a, b in zip(tensors, fresh):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert codec.error_flags() == 0
    with pytest.raises(ValueError):
        codec.encode_tensors([f32[2].view(128, 128).t()])
    with pytest.raises(ValueError):
        codec.encode_tensors([torch.zeros(64)])


# ------------------------------------------------------------------------------- 7: capture
class _Pair:
    """encode_v → decode_v over fixed tensors (every class, one allocation per message)."""

    def __init__(self, codec, sizes):
        self.c, self.sizes = codec, sizes
        self.msgs = [torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")[:n] for n in sizes]
        caps = [encode_bound(n, 4) for n in sizes]
        self.enc = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
        self.dec = [torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")[:n] for n in sizes]
        n = len(sizes)
        self.tab = [ptrs(self.msgs), i64(sizes), ptrs(self.enc), i64(caps), ptrs(self.dec)]
        self.elen = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.est = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.dlen = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.dst = torch.zeros(n, dtype=torch.int32, device="cuda")

    def fill(self, seed):
        rng = np.random.default_rng(seed)
        host = [message(rng, n) for n in self.sizes]
        for t, m in zip(self.msgs, host):
            if m.size:
                t.copy_(torch.from_numpy(m))
        return host

    def run(self):
        p, n, e, cap, d = self.tab
        self.c.encode_v(p, n, e, cap, lengths=self.elen, status=self.est)
        self.c.decode_v(e, self.elen, d, n, lengths=self.dlen, status=self.dst)

    def check(self, orc, host):
        torch.cuda.synchronize()
        cfg = orc.config(sample_fraction=1.0)
        ln = self.elen.cpu().numpy()
        assert int(self.est.abs().sum()) == 0 and int(self.dst.abs().sum()) == 0
        for i, m in enumerate(host):
            assert self.enc[i][: ln[i]].cpu().numpy().tobytes() == orc.encode(m, cfg=cfg, bandwidth=10.0), i
            assert np.array_equal(self.dec[i].cpu().numpy(), m), i


def test_capture_replays(orc):
    s = _Pair(make_codec(), SIZES + [300 * 1024])
    host = s.fill(1)
    s.run()  # eager: the workspaces exist from here on
    s.check(orc, host)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        s.run()
    for seed in (2, 3):
        host = s.fill(seed)
        gr.replay()
        s.check(orc, host)
    assert s.c.error_flags() == 0


def test_capture_on_cold_context_is_refused():
    from psyne_amd._lib import TdtError
    s = _Pair(make_codec(), [65536, 1024])
    s.fill(4)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with pytest.raises(TdtError) as ei:
        with torch.cuda.graph(gr):
            s.run()
    assert ei.value.code == E_CAPTURE
