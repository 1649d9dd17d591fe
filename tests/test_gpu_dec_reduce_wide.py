"""Decode-reduce into wide destinations (TDT_ELEM_F32_FROM_BF16 / TDT_ELEM_F32_FROM_F16): bf16 / fp16 blobs
summed into float32 tensors in one pass, on the one-workgroup and the tiled route.  The reference is
tests/test_gpu_dec_reduce.py's chain of correctly rounded sums (float64 on the CPU, rounded once to fp32:
one IEEE fp32 add) over the oracle-decoded wire elements widened on the CPU, compared bitwise.  No NaN
and no Inf go in; +-0, subnormals and pairs whose sum overflows do."""
import numpy as np
import pytest

from tests.support import E_CAPACITY, E_UNSUPPORTED, gradient
from tests.test_gpu_dec_acc import E_ELEMENT, LARGE_MIN, UNCP, crafted, finite, specials
from tests.test_gpu_dec_reduce import E_MISMATCH, WINDOW as W, _Peers, chained, dests_of

torch = pytest.importorskip("torch")
from psyne_amd._lib import TDT_OPT_REDUCE_TILED, TDT_REDUCE_TILE_BYTES as T  # noqa: E402
from tests.gpu_support import _gpu, i64, make_codec, orc, own  # noqa: E402, F401

pytestmark = pytest.mark.gpu

CODES = {"bf16": 0x31, "f16": 0x21}  # (include/psyne_tdt.h)
THR = 16384  # TDT_OPT_LARGE_MIN of the tiled tests, as in tests/test_gpu_dec_reduce_tiled.py
SERIAL = [0, 1, 2, 2]  # three referenced streams: off the fast path


def widen(u, t):
    """Wire elements (uint16 view) as the uint32 view of their exact float32 values."""
    return u.astype(np.uint32) << 16 if t == "bf16" else u.view(np.float16).astype(np.float32).view(np.uint32)


def encoded(orc, rng, t, n, uncp=False):
    """(blob, decoded) of n bytes of type t elements, the specials first."""
    m, src = finite(gradient(rng, n + 3)[:n], t), specials(t)[0]
    m[:src.size] = src
    blob = UNCP + m.tobytes() if uncp else orc.encode(m, cfg=orc.config(word_size=2, sample_fraction=1.0), bandwidth=10.0)
    assert orc.decode(blob) == (0, m.tobytes())
    return blob, m


class _Wide(_Peers):
    """_Peers whose destination i is float32 of twice the decoded bytes, its blobs elements of type wts[i]."""

    def __init__(self, wts, dests, phases, caps=None):
        super().__init__("f32", dests, phases, caps=caps or [2 * d[0][1].nbytes for d in dests],
                         codes=[CODES[t] for t in wts])
        self.wts = wts

    def want(self, i, set_=False):
        return chained(self.before[i].view(np.uint32), [widen(d, self.wts[i]) for _, d in self.dests[i]], "f32", set_)


def check(L, lens, st, set_=False):
    lens, st = lens.cpu().numpy(), st.cpu().numpy()
    assert not L.pstat.cpu().numpy().any()
    for i, d in enumerate(L.dests):
        assert (st[i], lens[i]) == (0, 2 * d[0][1].nbytes), i
        assert np.array_equal(L.got(i).view(np.uint32), L.want(i, set_)), (i, d[0][1].nbytes)
        assert L.guards_intact(i), i


@pytest.mark.parametrize("set_", [False, True], ids=["add", "set"])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("t", list(CODES))
def test_wide_sums_bitwise(orc, t, K, set_):
    """dests_of's sizes (512 as UNCP ... 100,004) and peer mixes at one window plus a group, without its
    serial-path entry (the last but one), and the sizes around the window's edge it lacks."""
    rng = np.random.default_rng(2801 + K)
    d = dests_of(orc, rng, t, K)
    dests = d[:-2] + d[-1:] + [[encoded(orc, rng, t, n) for _ in range(K)] for n in (W - 2, W + 2, W + 8, 100002)]
    L = _Wide([t] * 3 * len(dests), dests * 3, [p for p in (0, 4, 12) for _ in dests])
    L.fill(rng)
    lens, st = L.run(make_codec(), set_)
    torch.cuda.synchronize()
    check(L, lens, st, set_)


@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("t", list(CODES))
def test_wide_tiled_sums_bitwise(orc, t, K):
    rng = np.random.default_rng(2811 + K)
    sizes = (THR, THR + 2, T - 2, T, T + 8, 2 * T + 16)
    dests = [[encoded(orc, rng, t, n) for _ in range(K)] for n in sizes]
    dests.append([encoded(orc, rng, t, 2 * T + 16, uncp=k == 1) for k in range(K)])
    tiled = [d[0][1].nbytes for d in dests if d[0][1].nbytes > THR]
    bits = []
    for options, large in (((), len(tiled)), (((TDT_OPT_REDUCE_TILED, 0),), 0)):
        L = _Wide([t] * len(dests), dests, [(0, 4, 12)[i % 3] for i in range(len(dests))])
        L.fill(np.random.default_rng(2812))
        codec = make_codec(options=((LARGE_MIN, THR),) + options)
        # (one code for the call: the instances are chosen on the host)
        lens, st = codec.decode_reduce_v(*L.args, elem=CODES[t], peer_status=L.pstat)
        torch.cuda.synchronize()
        check(L, lens, st)
        assert codec.stat("REDUCE_LARGE") == large
        assert not large or codec.stat("REDUCE_TILES") == sum(-(-n // T) for n in tiled)
        bits.append([L.got(i) for i in range(len(dests))])
    assert all(np.array_equal(a, b) for a, b in zip(*bits))


# kind: (decoded bytes w, destination phase, capacity, status, what peer `pos` is)
REFUSALS = {
    "capacity_2w_less_4": (1028, 0, lambda w: 2 * w - 4, E_CAPACITY, None),
    "capacity_w": (1028, 0, lambda w: w, E_CAPACITY, None),  # (enough for the wire, not for the destination)
    "phase_2": (1028, 2, lambda w: 2 * w, E_ELEMENT, None),
    "odd_w": (1028, 0, lambda w: 2 * w, E_ELEMENT, "odd"),
    "longer_peer": (1028, 0, lambda w: 2 * w + 64, E_MISMATCH, "longer"),
    "three_streams": (1028, 0, lambda w: 2 * w, E_UNSUPPORTED, "serial"),
    "capacity_w_tiled": (2 * T + 16, 0, lambda w: w, E_CAPACITY, None),
    "three_streams_tiled": (2 * T + 16, 0, lambda w: 2 * w, E_UNSUPPORTED, "serial"),
}


@pytest.mark.parametrize("pos", [0, 2], ids=["first", "last"])
@pytest.mark.parametrize("kind", list(REFUSALS))
def test_refused_wide_destination_is_untouched(orc, kind, pos):
    n, phase, cap, status, edit = REFUSALS[kind]
    rng, t = np.random.default_rng(2803), "bf16"
    bad = [encoded(orc, rng, t, n) for _ in range(3)]
    if edit == "odd":  # an UNCP blob of 1,027 bytes
        raw = rng.integers(0, 127, n - 1, dtype=np.uint8)
        bad[pos] = (UNCP + raw.tobytes(), raw)
    elif edit == "longer":
        bad[pos] = encoded(orc, rng, t, n + 16)
    elif edit == "serial":
        bad[pos] = (crafted(bad[pos][1], 4, SERIAL), bad[pos][1])
    good = [encoded(orc, rng, t, 2048) for _ in range(3)]
    L = _Wide([t, t], [bad, good], [phase, 0], caps=[cap(n), 4096])
    L.fill(rng)
    lens, st = L.run(make_codec(options=((LARGE_MIN, THR),)))
    torch.cuda.synchronize()
    assert st.cpu().tolist()[:2] == [status, 0] and lens.cpu().tolist()[:2] == [0, 4096]
    assert np.array_equal(L.got(0), L.before[0]) and L.guards_intact(0)
    assert np.array_equal(L.got(1).view(np.uint32), L.want(1)) and L.guards_intact(1)


def test_mixed_list_and_tensor_call(orc):
    rng, K, n = np.random.default_rng(2804), 3, W + 16
    # (element code, wire type, destination type): fp32 and bf16 summed in their own type beside both widening codes
    rows = [(1, "f32", "f32"), (3, "bf16", "bf16"), (0x31, "bf16", "f32"), (0x21, "f16", "f32")]
    enc = lambda m: (orc.encode(m, cfg=orc.config(word_size=m.itemsize), bandwidth=10.0), m)  # noqa: E731
    dests = [[enc(finite(gradient(rng, n), wt)) for _ in range(K)] for _, wt, _ in rows]
    caps = [d[0][1].nbytes * (2 if c > 4 else 1) for d, (c, _, _) in zip(dests, rows)]
    L = _Peers("f32", dests, [0, 4, 12, 0], caps=caps, codes=[c for c, _, _ in rows])
    before = [finite(rng.integers(0, 256, cap, dtype=np.uint8), dt) for cap, (_, _, dt) in zip(caps, rows)]
    for b, (_, v) in zip(before, L.outs):
        v.copy_(torch.from_numpy(b.view(np.uint8)))
    lens, st = L.run(make_codec())
    torch.cuda.synchronize()
    assert not st.cpu().numpy()[:4].any() and lens.cpu().tolist()[:4] == caps and not L.pstat.cpu().numpy().any()
    for i, (c, wt, dt) in enumerate(rows):
        decs = [widen(d, wt) if c > 4 else d for _, d in dests[i]]
        assert np.array_equal(L.got(i), chained(before[i], decs, dt, False).view(np.uint8)), rows[i]
        assert L.guards_intact(i), i
    # the tensor call: the bf16 row's blobs into a float32 tensor, the bits of the pointer call
    peers = [(own(dests[2][k][0], lead=1), i64([0]), i64([len(dests[2][k][0])])) for k in range(K)]
    out = torch.from_numpy(before[2].view(np.uint8).copy()).cuda().view(torch.float32)
    codec = make_codec()
    lens, st = codec.decode_reduce_tensors(peers, [out], wire_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert (int(st[0]), int(lens[0])) == (0, caps[2]) and np.array_equal(out.view(torch.uint8).cpu().numpy(), L.got(2))
    with pytest.raises(ValueError):
        codec.decode_reduce_tensors(peers, [out.view(torch.bfloat16)], wire_dtype=torch.bfloat16)
