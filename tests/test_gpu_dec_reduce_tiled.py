"""The tiled form of decode-reduce (tdt_dec_reduce_tiled.h): destinations of tdt_decode_reduce_v above the
large-message threshold summed as tiles of TDT_REDUCE_TILE_BYTES, one workgroup per tile.  The reference
is tests/test_gpu_dec_reduce.py's: the correctly rounded sum (float64, rounded once per add) chained in
peer order, compared bitwise.  No NaN and no Inf go in.

The f64 list's last size is (3T + 100 + 8) rounded down to whole elements: 3T + 108 itself is no whole
number of f64 elements and would be refused (TDT_E_ELEMENT); the rounded size keeps the partial group."""
import numpy as np
import pytest

from tests.support import E_CAPACITY, E_TRUNCATED, gradient
from tests.test_gpu_dec_acc import E_ELEMENT, LARGE_MIN, TYPES, UNCP, crafted, finite, specials
from tests.test_gpu_dec_reduce import E_MISMATCH, WINDOW as W, _Peers, chained

torch = pytest.importorskip("torch")
from psyne_amd._lib import TDT_OPT_REDUCE_TILED, TDT_OPT_TILE_CAP, TDT_REDUCE_TILE_BYTES as T  # noqa: E402
from tests.gpu_support import _gpu, i64, make_codec, orc, own  # noqa: E402, F401

pytestmark = pytest.mark.gpu

THR = 16384  # TDT_OPT_LARGE_MIN of these tests: the lists are far below 4096 times it, so it is the threshold
OPTS = ((LARGE_MIN, THR),)
SERIAL = [0, 1, 2, 2]  # three referenced streams: off the fast path


def dests_of(orc, rng, t, K):
    """(destinations, tiled): per destination K (blob, decoded) pairs; tiled[i]: the rule puts it on tiles."""
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

    enc = lambda m: pair(orc.encode(m, cfg=cfg, bandwidth=10.0))  # noqa: E731
    sizes = (THR, THR + 16, T - 16, T, T + 16, 2 * T + W + 16, (3 * T + 100 + max(es, 4)) // es * es)
    out = [[enc(msg(n)) for _ in range(K)] for n in sizes]
    n = 2 * T + 16
    splits = ([0, 0, 0, 1], [0, 1, 1, 1], [0, 0, 1, 1])  # segments 12 + 4, 4 + 12, 8 + 8
    out.append([pair(crafted(msg(n), 4, splits[k % 3])) for k in range(K)])
    for pos in sorted({0, K // 2, K - 1}):  # one UNCP peer: first, middle, last
        out.append([pair(UNCP + msg(n).tobytes()) if k == pos else enc(msg(n)) for k in range(K)])
    out.append([pair(crafted(msg(n), 4, splits[0], keep=0.5)) if k == K - 1 else enc(msg(n)) for k in range(K)])
    out.append([pair(crafted(msg(n), (2, 4)[k % 2], ([0, 1], splits[2])[k % 2])) for k in range(K)])
    serial = len(out)
    out.append([pair(crafted(msg(n), 4, SERIAL)) if k == K // 2 else enc(msg(n)) for k in range(K)])
    edged = []  # constant around every tile edge: capped runs of both streams cross each boundary
    for k in range(K):
        m = msg(3 * T + 16)
        for e in (T, 2 * T, 3 * T):
            m[(e - 1100) // es:(e + 1100) // es] = m[e // es]
        edged.append(enc(m))
    out.append(edged)
    return out, [d[0][1].nbytes > THR and i != serial for i, d in enumerate(out)]


def check(L, lens, st, set_=False):
    lens, st = lens.cpu().numpy(), st.cpu().numpy()
    assert not L.pstat.cpu().numpy().any()
    for i, d in enumerate(L.dests):
        assert (st[i], lens[i]) == (0, d[0][1].nbytes), i
        assert np.array_equal(L.got(i).view(d[0][1].dtype), L.want(i, set_)), (i, d[0][1].nbytes)
        assert L.guards_intact(i), i


@pytest.mark.parametrize("set_", [False, True], ids=["add", "set"])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("t", list(TYPES))
def test_tiled_sums_bitwise(orc, t, K, set_):
    rng, es = np.random.default_rng(2711 + K), TYPES[t][1]
    dests, tiled = dests_of(orc, rng, t, K)
    L = _Peers(t, dests * 3, [p for p in (0, es, 16 - es) for _ in dests])
    L.fill(rng)
    codec = make_codec(options=OPTS)
    lens, st = L.run(codec, set_)
    torch.cuda.synchronize()
    check(L, lens, st, set_)
    assert codec.stat("REDUCE_LARGE") == 3 * sum(tiled)
    assert codec.stat("REDUCE_TILES") == 3 * sum(-(-d[0][1].nbytes // T) for d, on in zip(dests, tiled) if on)


@pytest.mark.parametrize("how", ["option_0", "tile_cap_1", "captured_cold"])
def test_fallbacks_same_bits(orc, how):
    """Every destination is longer than a tile, so a budget of one tile holds none of them."""
    rng, t, K = np.random.default_rng(2712), "f32", 3
    dests = [d for d in dests_of(orc, rng, t, K)[0] if d[0][1].nbytes > T]
    L = _Peers(t, dests, [(0, 4, 12)[i % 3] for i in range(len(dests))])
    L.fill(rng)
    codec = make_codec(options=OPTS + {"option_0": ((TDT_OPT_REDUCE_TILED, 0),), "tile_cap_1": ((TDT_OPT_TILE_CAP, 1),),
                                       "captured_cold": ()}[how])
    if how == "captured_cold":
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            lens, st = L.run(codec)
        gr.replay()
    else:
        lens, st = L.run(codec)
    torch.cuda.synchronize()
    check(L, lens, st)
    assert codec.stat("REDUCE_LARGE") == 0 and codec.error_flags() == 0


# kind: (destination phase, capacity short by, status, edit of the last peer's blob, the blob's own fault)
REFUSALS = {
    "truncated": (0, 0, E_TRUNCATED, "cut", True),
    "capacity": (0, 1, E_CAPACITY, None, False),
    "longer_peer": (0, 0, E_MISMATCH, "longer", None),
    "phase_1": (1, 0, E_ELEMENT, None, False),
}


@pytest.mark.parametrize("kind", list(REFUSALS))
def test_refused_long_destination_is_untouched(orc, kind):
    phase, short, status, edit, own_fault = REFUSALS[kind]
    rng, n, K = np.random.default_rng(2713), 2 * T + 16, 3
    enc = lambda m: (orc.encode(m, bandwidth=10.0), m)  # noqa: E731
    bad = [enc(finite(gradient(rng, n), "f32")) for _ in range(K)]
    if edit == "longer":
        bad[-1] = enc(finite(gradient(rng, n + 16), "f32"))
    elif edit == "cut":
        bad[-1] = (bad[-1][0][:-7], bad[-1][1])
    good = [enc(finite(gradient(rng, n), "f32")) for _ in range(K)]
    L = _Peers("f32", [bad, good], [phase, 0], caps=[max(m.nbytes for _, m in bad) - short, n])
    L.fill(rng)
    codec = make_codec(options=OPTS)
    lens, st = L.run(codec)
    torch.cuda.synchronize()
    assert st.cpu().tolist()[:2] == [status, 0] and lens.cpu().tolist()[:2] == [0, n]
    assert np.array_equal(L.got(0), L.before[0]) and L.guards_intact(0)
    assert np.array_equal(L.got(1).view(np.uint32), L.want(1)) and L.guards_intact(1)
    ps = L.pstat.cpu().numpy().reshape(K, 2)
    want = [0] * K if own_fault is None else [status if k == K - 1 or not own_fault else 0 for k in range(K)]
    assert ps[:, 0].tolist() == want and not ps[:, 1].any()
    assert codec.stat("REDUCE_LARGE") == 1


def test_captured_tiled_call_adds_on_every_replay(orc):
    rng = np.random.default_rng(2714)
    dests = []
    for n in (512, T + 16, 3 * T + 16):
        ms = [finite(gradient(rng, n), "f32") for _ in range(3)]
        for m in ms:
            m[m.view(np.float32) == 0] = 0  # (+0 only, as in the one-workgroup call's capture test)
        dests.append([(orc.encode(m, bandwidth=10.0), m) for m in ms])
    L, codec = _Peers("f32", dests, [0, 4, 12]), make_codec(options=OPTS)
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
    assert codec.error_flags() == 0 and codec.stat("REDUCE_LARGE") == 2


def test_tensor_call_default_threshold(orc):
    """Default options: 300,016 bytes is above the default threshold, the 4 KiB tensors are not."""
    rng = np.random.default_rng(2715)
    tt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
    names = [(t, n) for n in (300016, 4096) for t in tt]
    decs = {tn: [finite(gradient(rng, tn[1]), tn[0]) for _ in range(3)] for tn in names}
    peers = []
    for k in range(3):
        blobs = [orc.encode(decs[tn][k], cfg=orc.config(word_size=TYPES[tn[0]][1]), bandwidth=10.0) for tn in names]
        off = np.cumsum([0] + [len(b) for b in blobs])
        peers.append((own(b"".join(blobs), lead=1), i64(off), i64(len(b) for b in blobs)))
    before = {tn: finite(rng.integers(0, 256, tn[1], dtype=np.uint8), tn[0]) for tn in names}
    outs = [torch.from_numpy(before[tn].view(np.uint8).copy()).cuda().view(tt[tn[0]]) for tn in names]
    codec = make_codec()
    lens, st = codec.decode_reduce_tensors(peers, outs)
    torch.cuda.synchronize()
    assert not st.cpu().numpy()[:8].any() and lens.cpu().tolist()[:8] == [n for _, n in names]
    for o, tn in zip(outs, names):
        want = chained(before[tn], decs[tn], tn[0], False)
        assert np.array_equal(o.view(torch.uint8).cpu().numpy(), want.view(np.uint8)), tn
    assert codec.stat("REDUCE_LARGE") == 4
