"""Encode-narrow with error feedback (tdt_encode_narrow_ef_v): v = g + r in float32 is narrowed and encoded,
the residual becomes r' = v - widen(narrow(v)), bit pattern 0 where the wire value is an infinity or a NaN.
The reference is plain numpy over tests/test_gpu_enc_narrow.py's `narrow` / `widen` and the oracle's width-2
encode; blobs, lengths, statuses and residuals are compared bit for bit, with canaries around both."""
import numpy as np
import pytest

from tests.support import CANARY, E_CAPACITY
from tests.test_gpu_enc_narrow import (CODES, COMMON, E_ARG, E_ELEMENT, R, VECTORS, bound, family, narrow, run, want,
                                       widen)

torch = pytest.importorskip("torch")
from psyne_amd._lib import TDT_OPT_LARGE_MIN, TDT_OPT_NARROW_TILED, TDT_OPT_RAW_FALLBACK, TDT_OPT_TILE_CAP  # noqa: E402
from tests.gpu_support import _gpu, guarded, i64, make_codec, orc, own, ptrs  # noqa: E402, F401

pytestmark = pytest.mark.gpu

RAW = ((TDT_OPT_RAW_FALLBACK, 1),)
OPTS = ((TDT_OPT_LARGE_MIN, 4 * R),)  # a tensor of more than R elements tiles
HOW = {"tiled": (), "option_0": ((TDT_OPT_NARROW_TILED, 0),), "tile_cap_1": ((TDT_OPT_TILE_CAP, 1),)}
ULP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}  # half a wire ulp of 1.0


def expect(orc, g, r, t, raw=False):
    """(blob, r' as uint32) for source bits g (uint32) and residual r (float32)."""
    with np.errstate(all="ignore"):
        v = g.view(np.float32) + r
        h = narrow(v.view(np.uint32), t)
        ex = 0x7F80 if t == "bf16" else 0x7C00
        rn = np.where((h & ex) == ex, np.float32(0), v - widen(h, t).view(np.float32)).astype(np.float32)
    return want(orc, h.tobytes(), raw), rn.view(np.uint32)


def run_ef(codec, gs, rs, codes, gleads=None, rleads=None, caps=None):
    """Message i = source bits gs[i], residual rs[i] (None: address 0), `gleads[i]` / `rleads[i]` bytes off a
    16-byte boundary; [(blob, length, status, the residual afterwards as uint32)], canaries checked."""
    n = len(gs)
    gleads, rleads = gleads or [0] * n, rleads or [0] * n
    caps = caps or [bound(2 * g.size) for g in gs]
    ins = [own(g.view(np.uint8), l) for g, l in zip(gs, gleads)]
    res = [guarded(4 * g.size, l) if r is not None else None for g, r, l in zip(gs, rs, rleads)]
    [x[1].copy_(torch.from_numpy(r.view(np.uint8))) for x, r in zip(res, rs) if x]
    outs = [guarded(c, i % 4) for i, c in enumerate(caps)]
    lens, st = codec.encode_narrow_v(ptrs(ins), i64(4 * g.size for g in gs), ptrs([v for _, v in outs]), i64(caps),
                                     elems=torch.tensor(codes, dtype=torch.uint8, device="cuda"),
                                     resid_ptrs=i64(x[1].data_ptr() if x else 0 for x in res))
    torch.cuda.synchronize()
    lens, st, got = lens.cpu().numpy(), st.cpu().numpy(), []
    for i, ((t, _), x) in enumerate(zip(outs, res)):
        h, lead = t.cpu().numpy(), 64 + i % 4
        assert (h[:lead] == CANARY).all() and (h[lead + lens[i]:] == CANARY).all(), i  # (nothing outside the blob)
        rn = None
        if x:
            hr, rl = x[0].cpu().numpy(), 64 + rleads[i]
            assert (hr[:rl] == CANARY).all() and (hr[rl + 4 * gs[i].size:] == CANARY).all(), i
            rn = hr[rl:rl + 4 * gs[i].size].copy().view(np.uint32) if rleads[i] % 4 == 0 else hr[rl:rl + 4 * gs[i].size]
        got.append((h[lead:lead + lens[i]].tobytes(), int(lens[i]), int(st[i]), rn))
    return got


def sized(t, sizes, seed):
    """(sources, residuals of about half a wire ulp) of the gradient and dense families at every size, and the
    constant tensors whose narrowing changes once the residual is updated (a stale read shows in the blob)."""
    rng = np.random.default_rng(seed)
    gs = [family(rng, f, n, t) for n in sizes for f in ("gradient", "dense")]
    with np.errstate(all="ignore"):
        rs = [np.nan_to_num(g.view(np.float32) * np.float32(ULP[t]) * rng.uniform(-1, 1, g.size).astype(np.float32),
                            posinf=0, neginf=0).astype(np.float32) for g in gs]
    if sizes[-1] == 8 * R:  # g = 1.0, r = 0.75 ulp: v narrows to 0x3F81 / 0x3C01, g + r' to 0x3F80 / 0x3C00
        gs.append(np.full(8 * R, 0x3F800000, np.uint32))
        rs.append(np.full(8 * R, 1.5 * ULP[t], np.float32))
    return gs, rs


def twice(orc, codec, gs, rs, t, raw):
    """Two calls on one codec: the second starts from the first call's r'."""
    n = len(gs)
    leads, rleads = [4 * (i % 4) for i in range(n)], [4 * ((i // 2 + i) % 4) for i in range(n)]
    for _ in range(2):
        got = run_ef(codec, gs, rs, [CODES[t]] * n, leads, rleads)
        for i, (g, r, (blob, ln, st, rn)) in enumerate(zip(gs, rs, got)):
            eb, er = expect(orc, g, r, t, raw)
            assert (st, ln) == (0, len(eb)) and blob == eb and np.array_equal(rn, er), (i, g.size)
        rs = [x[3].view(np.float32) for x in got]


@pytest.mark.parametrize("raw", [False, True], ids=["tdt", "rawfb"])
@pytest.mark.parametrize("t", list(CODES))
def test_sizes_one_workgroup(orc, t, raw):
    """The UNCP floor, the resident form, the chunk edge and a partial last group."""
    gs, rs = sized(t, (30, 512, R - 2, R, R + 2, 2 * R + 18), 3201)
    twice(orc, make_codec(options=RAW if raw else ()), gs, rs, t, raw)


@pytest.mark.parametrize("how", list(HOW))
@pytest.mark.parametrize("raw", [False, True], ids=["tdt", "rawfb"])
@pytest.mark.parametrize("t", list(CODES))
def test_sizes_tiles(orc, t, raw, how):
    gs, rs = sized(t, (R + 2, 2 * R + 18, 3 * R - 2, 8 * R), 3202)
    codec = make_codec(options=OPTS + HOW[how] + (RAW if raw else ()))
    twice(orc, codec, gs, rs, t, raw)
    assert codec.stat("NARROW_LARGE") == (len(gs) if how == "tiled" else 0)


ANCHORS = {  # (g, r) -> (h, r'), worked by hand: ties of v, a sum that rounds, subnormal sums, overflow, NaN
    "bf16": {(0x3F800000, 0x3BC00000): (0x3F81, 0xBB000000), (0x3F800000, 0x33C00000): (0x3F80, 0x34000000),
             (0x00800000, 0x80400001): (0x0040, 0x80000001), (0x7FC00001, 0x3F800000): (0x7FC0, 0),
             (0x7F7FFFFF, 0x7F7FFFFF): (0x7F80, 0), (0x7F7FFFFF, 0x00000000): (0x7F80, 0)},
    "f16": {(0x3F800000, 0x3A400000): (0x3C01, 0xB9800000), (0x3F800000, 0x33C00000): (0x3C00, 0x34000000),
            (0x00800000, 0x80400001): (0x0000, 0x003FFFFF), (0x7FC00001, 0x3F800000): (0x7E00, 0),
            (0x477FF000, 0x00000000): (0x7C00, 0), (0x47800000, 0x3F800000): (0x7C00, 0)},
}


@pytest.mark.parametrize("t", list(CODES))
def test_rule_vectors(orc, t):
    """The narrowing rule's patterns as v, split into g (the high mantissa bits) and r = v - g where that sum is
    exact and into v + (-0.0) elsewhere; the anchors ahead of them."""
    pos = np.array(VECTORS[t] + COMMON, np.uint32)
    v = np.concatenate([pos, pos | 0x80000000])
    with np.errstate(all="ignore"):
        g = v & np.uint32(0xFFFFF000)
        r = v.view(np.float32) - g.view(np.float32)
        bad = (g.view(np.float32) + r).view(np.uint32) != v
        g, r = np.where(bad, v, g), np.where(bad, np.float32(-0.0), r).astype(np.float32)
        nan = (v & 0x7FFFFFFF) > 0x7F800000
        assert np.array_equal((g.view(np.float32) + r).view(np.uint32)[~nan], v[~nan])
    ag, ar = (np.array([k[i] for k in ANCHORS[t]], np.uint32) for i in (0, 1))
    g, r = np.resize(np.concatenate([ag, g]), 1024), np.resize(np.concatenate([ar.view(np.float32), r]), 1024)
    (blob, ln, st, rn), = run_ef(make_codec(), [g], [r], [CODES[t]])
    eb, er = expect(orc, g, r, t)
    assert (st, blob) == (0, eb) and np.array_equal(rn, er)
    (blob, ln, st, _), = run_ef(make_codec(bandwidth=1000.0), [g], [r], [CODES[t]])  # the policy off: the halfwords
    for i, (h, rp) in enumerate(ANCHORS[t].values()):
        assert (int(np.frombuffer(blob[4:], np.uint16)[i]), int(rn[i])) == (h, rp), i


@pytest.mark.parametrize("n,opts", [(2048, ()), (2 * R + 18, OPTS)], ids=["one_workgroup", "tiled"])
def test_refusals_and_mixing(orc, n, opts):
    rng = np.random.default_rng(3204)
    # runs of 64 equal elements keep their TDT blob under raw fallback; dense data falls back
    g, d = np.repeat(family(rng, "gradient", n // 64 + 1, "bf16"), 64)[:n], family(rng, "dense", n, "bf16")
    r =(g.view(np.float32) * np.float32(2.0 ** -9)).astype(np.float32)
    (eg, rg), (ed, rd) = expect(orc, g, r, "bf16", True), expect(orc, d, r, "bf16", True)
    assert eg[:4] != ed[:4] and len(ed) == 2 * n + 4  # the TDT route and the raw route
    #        ordinary  resid lead 2  bad code  TDT - 1      raw - 1      no residual  ordinary raw  fp16
    gs = [g,           g,            g,        g,           d,           g,           d,            g]
    rs = [r,           r,            r,        r,           r,           None,        r,            r]
    codes = [0x13,     0x13,         0x31,     0x13,        0x13,        0x13,        0x13,         0x12]
    rleads = [4,       2,            0,        8,           12,          0,           0,            12]
    caps = [len(eg),   bound(2 * n), bound(2 * n), len(eg) - 1, len(ed) - 1, bound(2 * n), len(ed), bound(2 * n)]
    stats = [0,        E_ELEMENT,    E_ARG,    E_CAPACITY,  E_CAPACITY,  0,           0,            0]
    codec = make_codec(options=opts + RAW)
    got = run_ef(codec, gs, rs, codes, [0, 4, 8, 12, 0, 4, 8, 12], rleads, caps)
    assert [x[2] for x in got] == stats
    for i in (1, 2, 3, 4):  # refused: the residual bit for bit, nothing in the blob (run_ef: canaries from length 0 on)
        assert got[i][1] == 0 and got[i][3].tobytes() == r.tobytes(), i
    assert (got[0][0], got[6][0]) == (eg, ed) and np.array_equal(got[0][3], rg) and np.array_equal(got[6][3], rd)
    assert got[5][0] == run(codec, [g], [0x13])[0][0] == want(orc, narrow(g, "bf16").tobytes(), True)
    ef, rf = expect(orc, g, r, "f16", True)
    assert got[7][0] == ef and np.array_equal(got[7][3], rf)
    x = i64([0]).data_ptr()  # a null residual array: TDT_E_ARG for the whole call, before anything is read
    assert codec._lib.tdt_encode_narrow_ef_v(codec._h, x, x, 1, None, None, 0x13, x, x, x, x, None) == E_ARG


@pytest.mark.parametrize("t,dt", [("bf16", torch.bfloat16), ("f16", torch.float16)])
def test_python_surface(t, dt):
    rng = np.random.default_rng(3205)
    sizes = (1000, R + 6, 5 * R)
    gs = [torch.from_numpy(rng.normal(0, 0.01, n).astype(np.float32)).cuda() for n in sizes]
    rs = [torch.from_numpy(rng.normal(0, 1e-5, n).astype(np.float32)).cuda() for n in sizes]
    rs[1] = None
    vs = [g.cpu().numpy() + (r.cpu().numpy() if r is not None else np.float32(0)) for g, r in zip(gs, rs)]
    codec = make_codec(ws=2, options=OPTS)
    out, slots, lens, st = codec.encode_tensors(gs, wire_dtype=dt, residuals=rs)
    outs = [torch.empty_like(g) for g in gs]
    _, ds = codec.decode_reduce_tensors([(out, slots, lens)], outs, set=True, wire_dtype=dt)
    torch.cuda.synchronize()
    assert not st.cpu().numpy()[:3].any() and not ds.cpu().numpy()[:3].any()
    for v, o, r in zip(vs, outs, rs):
        assert np.array_equal(o.cpu().numpy().view(np.uint32), widen(narrow(v.view(np.uint32), t), t))
        if r is not None:  # decoded + r' is v, bit for bit
            assert np.array_equal((o.cpu().numpy() + r.cpu().numpy()).view(np.uint32), v.view(np.uint32))
    for bad, kw in [([rs[0].double(), None, rs[2]], {"wire_dtype": dt}), ([rs[0][:-1], None, rs[2]], {"wire_dtype": dt}),
                    ([rs[0].cpu(), None, rs[2]], {"wire_dtype": dt}), (rs[:2], {"wire_dtype": dt}), (rs, {})]:
        with pytest.raises(ValueError):
            codec.encode_tensors(gs, residuals=bad, **kw)
