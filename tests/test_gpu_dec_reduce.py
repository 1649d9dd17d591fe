"""Decode-reduce on the GPU (tdt_decode_reduce_v, decode_reduce_tensors): the blobs of K peers summed
into each destination in one pass.  The reference is tests/test_gpu_dec_acc.py's correctly rounded
sum (float64 on the CPU, rounded once to the element type) applied K times in peer order, compared
bitwise; under TDT_REDUCE_SET the chain starts from peer 0's decoded bits.  No NaN and no Inf go in;
+-0, subnormals and pairs whose sum overflows do."""
import numpy as np
import pytest

from tests.decode_edge_cases import geometry
from tests.support import E_ARG, E_CAPACITY, E_MAGIC, E_TRUNCATED, E_UNSUPPORTED, gradient
from tests.test_gpu_dec_acc import E_ELEMENT, TYPES, UNCP, _List, crafted, finite, rounded_sum, specials

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, i32, i64, make_codec, orc, own, ptrs  # noqa: E402, F401

pytestmark = pytest.mark.gpu

E_MISMATCH = 14  # (include/psyne_tdt.h)
WINDOW = geometry()["wr"] * 1024  # the decoder's window: WR rounds of 64 16-byte groups


def chained(before, decs, t, set_):
    want = decs[0] if set_ else rounded_sum(before, decs[0], t)
    for d in decs[1:]:
        want = rounded_sum(want, d, t)
    return want


class _Peers(_List):
    """_List with K blobs per destination: dests[i] = [(blob, decoded)] * K, laid out peer-major."""

    def __init__(self, t, dests, phases, **kw):
        super().__init__(t, [d[0] for d in dests], phases, **kw)
        self.dests, self.k = dests, len(dests[0])
        self.pblobs = [own(d[k][0], lead=1) for k in range(self.k) for d in dests]
        self.pstat = i32([-1] * len(self.pblobs))
        self.args = (ptrs(self.pblobs), i64(b.numel() for b in self.pblobs), self.k) + self.args[2:]

    def run(self, codec, set_=False, **kw):
        return codec.decode_reduce_v(*self.args, elems=self.elems, set=set_, peer_status=self.pstat, **kw)

    def want(self, i, set_=False):
        decs = [dec for _, dec in self.dests[i]]
        return chained(self.before[i].view(decs[0].dtype), decs, self.t, set_)


def dests_of(orc, rng, t, K):
    """Per destination, K (blob, decoded) pairs: every size at which the kernel takes another path, then
    the peer mixes at one window plus a group."""
    es, src = TYPES[t][1], specials(t)[0]
    cfg = orc.config(word_size=es, sample_fraction=1.0)

    def msg(n):
        u = finite(gradient(rng, n + 3)[:n], t)
        u[:src.size] = src
        return u

    def pair(blob):
        st, dec = orc.decode(blob)
        assert st == 0 and finite(dec, t).tobytes() == dec, "a bad blob, or a NaN or an Inf in the decoded message"
        return blob, finite(dec, t)

    enc = lambda n: pair(orc.encode(msg(n), cfg=cfg, bandwidth=10.0))  # noqa: E731
    out = [[enc(n) for _ in range(K)] for n in (512, 1024, WINDOW - 16, WINDOW, WINDOW + 16, 8 * WINDOW + 16, 65536,
                                                  100000 + max(es, 4))]
    assert all(b[:4] == UNCP for b, _ in out[0]) and all(b[:4] == b"DTDT" for b, _ in out[1])
    n = WINDOW + 16
    splits = ([0, 0, 0, 1], [0, 1, 1, 1], [0, 0, 1, 1])  # segments 12 + 4, 4 + 12, 8 + 8
    out.append([pair(crafted(msg(n), 4, splits[k % 3])) for k in range(K)])
    for pos in sorted({0, K // 2, K - 1}):  # one UNCP peer: first, middle, last
        out.append([pair(UNCP + msg(n).tobytes()) if k == pos else enc(n) for k in range(K)])
    out.append([pair(crafted(msg(n), 4, [0, 0, 0, 1], keep=0.5)) if k == K - 1 else enc(n) for k in range(K)])
    out.append([pair(crafted(msg(n), 4, [0, 1, 2, 2])) if k == K // 2 else enc(n) for k in range(K)])  # the serial path
    out.append([pair(crafted(msg(n), (2, 4)[k % 2], ([0, 1], [0, 0, 1, 1])[k % 2])) for k in range(K)])
    return out


@pytest.mark.parametrize("set_", [False, True], ids=["add", "set"])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("t", list(TYPES))
def test_sums_bitwise(orc, t, K, set_):
    rng, es = np.random.default_rng(2701 + K), TYPES[t][1]
    dests = dests_of(orc, rng, t, K)
    L = _Peers(t, dests * 3, [p for p in (0, es, 16 - es) for _ in dests])
    L.fill(rng)
    lens, st = L.run(make_codec(), set_)
    torch.cuda.synchronize()
    lens, st = lens.cpu().numpy(), st.cpu().numpy()
    assert not L.pstat.cpu().numpy().any()
    for i, d in enumerate(L.dests):
        assert (st[i], lens[i]) == (0, d[0][1].nbytes), i
        assert np.array_equal(L.got(i).view(d[0][1].dtype), L.want(i, set_)), (i, d[0][1].nbytes)
        assert L.guards_intact(i), i


# kind: (element type, destination phase, capacity short by, status, blob edit, the blob's own fault)
REFUSALS = {
    "truncated": ("f32", 0, 0, E_TRUNCATED, "cut", True),
    "bad_magic": ("f32", 0, 0, E_MAGIC, "magic", True),
    "capacity": ("f32", 0, 1, E_CAPACITY, None, False),
    "phase_1": ("f32", 1, 0, E_ELEMENT, None, False),
    "size_not_elements": ("f64", 0, 0, E_ELEMENT, None, False),
    "width_12": ("f32", 0, 0, E_UNSUPPORTED, 12, True),
    "longer_peer": ("f32", 0, 0, E_MISMATCH, "longer", None),
}


@pytest.mark.parametrize("pos", [0, 2], ids=["first", "last"])
@pytest.mark.parametrize("kind", list(REFUSALS))
def test_refused_destination_is_untouched(orc, kind, pos):
    t, phase, short, status, edit, own_fault = REFUSALS[kind]
    rng, n = np.random.default_rng(2702), 1200 if edit == 12 else 1028  # (1,028: whole f32 elements, no whole f64 ones)
    enc = lambda m, ws=4: (orc.encode(m, cfg=orc.config(word_size=ws), bandwidth=10.0), m)  # noqa: E731
    bad = [enc(finite(gradient(rng, n), "f32")) for _ in range(3)]
    if edit == 12:
        bad[pos] = enc(rng.integers(0, 3, n, dtype=np.uint8).view(np.uint32), 12)
    elif edit == "longer":
        bad[pos] = enc(finite(gradient(rng, n + 16), "f32"))
    elif edit:
        b = bad[pos][0]
        bad[pos] = (b[:len(b) - 7] if edit == "cut" else b"XXXX" + b[4:], bad[pos][1])
    good = [enc(finite(gradient(rng, 2048), t)) for _ in range(3)]
    L = _Peers(t, [bad, good], [phase, 0], caps=[max(m.nbytes for _, m in bad) - short, good[0][1].nbytes])
    L.fill(rng)
    lens, st = L.run(make_codec())
    torch.cuda.synchronize()
    assert st.cpu().tolist()[:2] == [status, 0] and lens.cpu().tolist()[:2] == [0, good[0][1].nbytes]
    assert np.array_equal(L.got(0), L.before[0]) and L.guards_intact(0)
    assert np.array_equal(L.got(1).view(good[0][1].dtype), L.want(1)) and L.guards_intact(1)
    ps = L.pstat.cpu().numpy().reshape(3, 2)
    want = [0] * 3 if own_fault is None else [status if k == pos or not own_fault else 0 for k in range(3)]
    assert ps[:, 0].tolist() == want and not ps[:, 1].any()


def test_argument_errors(orc):
    from psyne_amd._lib import TdtError
    rng = np.random.default_rng(2703)
    m = finite(gradient(rng, 2048), "f32")
    item = [(orc.encode(m, bandwidth=10.0), m)] * 2
    for code in (0, 5):  # a bad code per destination: that one is refused, its neighbour summed
        L = _Peers("f32", [item, item], [0, 0], codes=[code, 1])
        L.fill(rng)
        lens, st = L.run(make_codec())
        torch.cuda.synchronize()
        assert st.cpu().tolist()[:2] == [E_ARG, 0] and lens.cpu().tolist()[:2] == [0, m.nbytes]
        assert np.array_equal(L.got(0), L.before[0]) and np.array_equal(L.got(1).view(m.dtype), L.want(1))
    for n_peers, elem in ((0, 1), (9, 1), (2, 0)):
        with pytest.raises(TdtError) as ei:
            make_codec().decode_reduce_v(L.args[0].repeat(5), L.args[1].repeat(5), n_peers, *L.args[3:], elem=elem)
        assert ei.value.code == E_ARG


def test_captured_call_adds_on_every_replay(orc):
    rng = np.random.default_rng(2704)
    dests = []
    for n in (512, WINDOW, 65536 + 16):
        ms = [finite(gradient(rng, n), "f32") for _ in range(3)]
        for m in ms:
            m[m.view(np.float32) == 0] = 0  # (+0 only, as in the accumulate call's capture test)
        dests.append([(orc.encode(m, bandwidth=10.0), m) for m in ms])
    L, codec = _Peers("f32", dests, [0, 4, 12]), make_codec()
    L.fill(rng)
    L.run(codec)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        L.run(codec)
    gr.replay()
    gr.replay()
    torch.cuda.synchronize()
    for i in range(len(dests)):
        want = L.before[i]
        for _ in range(3):  # the eager call and two replays
            want = chained(want.view(np.uint32), [d for _, d in dests[i]], "f32", False)
        assert np.array_equal(L.got(i).view(np.uint32), want), i
    assert codec.error_flags() == 0


def test_tensor_call(orc):
    rng = np.random.default_rng(2705)
    tt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
    decs = {t: [finite(gradient(rng, 4096 + 16 * TYPES[t][1]), t) for _ in range(3)] for t in tt}
    peers = []
    for k in range(3):
        blobs = [orc.encode(decs[t][k], cfg=orc.config(word_size=TYPES[t][1]), bandwidth=10.0) for t in tt]
        off = np.cumsum([0] + [len(b) for b in blobs])
        peers.append((own(b"".join(blobs), lead=1), i64(off), i64(len(b) for b in blobs)))
    before = {t: finite(rng.integers(0, 256, decs[t][0].nbytes, dtype=np.uint8), t) for t in tt}
    outs = [torch.from_numpy(before[t].view(np.uint8).copy()).cuda().view(tt[t]) for t in tt]
    codec = make_codec()
    lens, st = codec.decode_reduce_tensors(peers, outs)
    torch.cuda.synchronize()
    assert not st.cpu().numpy()[:4].any() and lens.cpu().tolist()[:4] == [decs[t][0].nbytes for t in tt]
    for o, t in zip(outs, tt):
        assert np.array_equal(o.view(torch.uint8).cpu().numpy(), chained(before[t], decs[t], t, False).view(np.uint8)), t
    with pytest.raises(ValueError):
        codec.decode_reduce_tensors(peers, [outs[0].view(torch.int32)])
