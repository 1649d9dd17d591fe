"""Encode-narrow (tdt_encode_narrow_v): float32 tensors encoded as the width-2 blobs of their bf16 / fp16
narrowing.  The reference is `narrow`, a numpy restatement of the rule in include/psyne_tdt.h, followed by
the oracle's encode of the narrowed bytes at word size 2 (the UNCP form instead where raw fallback is on
and that blob is longer than w + 4).  Blob, length and status are compared byte for byte, the canaries
around every blob checked, and every blob decoded back to the narrowed bytes."""
import numpy as np
import pytest

from tests.support import CANARY, E_CAPACITY

torch = pytest.importorskip("torch")
from psyne_amd._lib import TDT_OPT_RAW_FALLBACK, TdtError  # noqa: E402
from tests.gpu_support import _gpu, guarded, i64, make_codec, orc, own, ptrs  # noqa: E402, F401

pytestmark = pytest.mark.gpu

R = 16384  # the elements whose planes the kernel keeps in LDS (kNarResident, psyne_amd/csrc/tdt_enc_narrow.h)
CODES = {"bf16": 0x13, "f16": 0x12}  # (include/psyne_tdt.h)
E_ARG, E_ELEMENT = 11, 13
UNCP = (0x554E4350).to_bytes(4, "little")
SIZES = (30, 510, 511, 512, 512 + 6, R - 2, R, R + 2, 2 * R + 18)


def narrow(u, t):
    """fp32 bit patterns (uint32) -> the wire halfwords (uint16)."""
    u = np.asarray(u, np.uint32)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    if t == "bf16":
        r = (u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16
        return np.where(nan, (u >> 16) | 0x0040, r).astype(np.uint16)
    with np.errstate(over="ignore"):
        r = np.where(nan, 0, u).astype(np.uint32).view(np.float32).astype(np.float16).view(np.uint16)
    return np.where(nan, ((u >> 16) & 0x8000) | 0x7E00 | ((u >> 13) & 0x3FF), r).astype(np.uint16)


def widen(h, t):
    """Wire halfwords as the bit patterns of their exact float32 values."""
    h = np.asarray(h, np.uint16)
    return h.astype(np.uint32) << 16 if t == "bf16" else h.view(np.float16).astype(np.float32).view(np.uint32)


def bound(w):
    return max(w + 4, 36 + 2 * w)


def want(orc, wire, raw=False, bandwidth=10.0):
    blob = orc.encode(np.frombuffer(wire, np.uint8), cfg=orc.config(word_size=2), bandwidth=bandwidth)
    return UNCP + wire if raw and len(blob) > len(wire) + 4 else blob


def run(codec, srcs, codes, leads=None, bleads=None, caps=None, elem=None):
    """Message i = the bytes srcs[i] `leads[i]` bytes off a 16-byte boundary, its blob `bleads[i]` bytes off
    one; returns [(blob bytes, length, status)], having checked the canaries and the round trip."""
    n = len(srcs)
    srcs = [np.ascontiguousarray(s).view(np.uint8) for s in srcs]
    leads, bleads = leads or [0] * n, bleads or [0] * n
    caps = caps or [bound(s.size // 2) for s in srcs]
    ins = [own(s, l) for s, l in zip(srcs, leads)]
    outs = [guarded(c, l) for c, l in zip(caps, bleads)]
    elems = torch.tensor(codes, dtype=torch.uint8, device="cuda") if elem is None else None
    lens, st = codec.encode_narrow_v(ptrs(ins), i64(s.size for s in srcs), ptrs([v for _, v in outs]), i64(caps),
                                     elems=elems, elem=elem or 0)
    torch.cuda.synchronize()
    lens, st = lens.cpu().numpy(), st.cpu().numpy()
    res = []
    for i, (t, v) in enumerate(outs):
        h = t.cpu().numpy()
        assert (h[:64 + bleads[i]] == CANARY).all() and (h[64 + bleads[i] + caps[i]:] == CANARY).all(), i
        body = h[64 + bleads[i]:64 + bleads[i] + caps[i]]
        assert (body[lens[i]:] == CANARY).all(), i  # (nothing behind the blob either)
        res.append((body[:lens[i]].tobytes(), int(lens[i]), int(st[i])))
    ok = [i for i in range(n) if res[i][2] == 0]
    back = [torch.empty(max(srcs[i].size // 2, 1), dtype=torch.uint8, device="cuda") for i in ok]
    dl, ds = codec.decode_v(ptrs([outs[i][1] for i in ok]), i64(res[i][1] for i in ok), ptrs(back),
                            i64(srcs[i].size // 2 for i in ok))
    torch.cuda.synchronize()
    assert not ds.cpu().numpy()[:len(ok)].any()
    for k, i in enumerate(ok):
        code = codes[i] if elem is None else elem
        exp = narrow(srcs[i].view(np.uint32), "bf16" if code == 0x13 else "f16").tobytes()
        assert back[k].cpu().numpy()[:len(exp)].tobytes() == exp and int(dl[k]) == len(exp), i
    return res


VECTORS = {
    "bf16": [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,  # ties both ways, and beside them
             0x3FFFFFFF, 0x7F7FFFFF, 0x7F7F7FFF, 0x00008000, 0x00018000, 0x00000001, 0x007FFFFF],
    "f16": [0x3F801000, 0x3F803000, 0x3F800FFF, 0x3F801001, 0x3F802FFF, 0x3F803001,
            0x3FFFF000, 0x477FE000, 0x477FEFFF, 0x477FF000, 0x47800000, 0x7F7FFFFF,  # carry; the largest finite; -> inf
            0x38800000, 0x387FE000, 0x387FC000, 0x38000000, 0x33800000, 0x33C00000, 0x33BFFFFF, 0x34200000,  # subnormals, ties
            0x33000000, 0x33000001, 0x32FFFFFF, 0x00000001, 0x007FFFFF, 0x7F802000],
}
COMMON = [0x00000000, 0x7F800000, 0x3F800000, 0x7FC00000, 0x7FC00001, 0x7F800001, 0x7FFFFFFF, 0x7FABCDEF, 0x7F80FFFF]
ANCHORS = {  # the rule's own figures, so that `narrow` is not the only witness
    "bf16": {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3FFFFFFF: 0x4000, 0x7F7FFFFF: 0x7F80, 0x7F800001: 0x7FC0,
             0xFF800001: 0xFFC0, 0x7FABCDEF: 0x7FEB, 0x80000000: 0x8000},
    "f16": {0x3F801000: 0x3C00, 0x3F803000: 0x3C02, 0x477FF000: 0x7C00, 0x477FEFFF: 0x7BFF, 0x33000000: 0x0000,
            0x33000001: 0x0001, 0x387FE000: 0x0400, 0x7F800001: 0x7E00, 0xFF800001: 0xFE00, 0x7F802000: 0x7E01},
}


@pytest.mark.parametrize("t", list(CODES))
def test_rounding_vectors(orc, t):
    pos = np.array(VECTORS[t] + COMMON, np.uint32)
    u = np.resize(np.concatenate([pos, pos | 0x80000000]), 1024)  # 2,048 wire bytes: the TDT route
    h = narrow(u, t)
    for k, v in ANCHORS[t].items():
        assert int(narrow([k], t)[0]) == v, hex(k)
        assert k in u
    (blob, ln, st), = run(make_codec(), [u], [CODES[t]])
    assert (st, blob) == (0, want(orc, h.tobytes())) and blob[:4] != UNCP
    # the narrowing alone: the policy off, the blob is the marker and the halfwords (the scalar code's route too)
    (blob, ln, st), = run(make_codec(bandwidth=1000.0), [u], None, elem=CODES[t])
    assert st == 0 and blob[:4] == UNCP
    assert np.array_equal(np.frombuffer(blob[4:], np.uint16), h)


def family(rng, name, n, t):
    """n elements whose wire halfwords have the family's planes."""
    lo, hi = rng.integers(0, 256, n), rng.integers(0, 256, n)
    if name == "gradient":  # the low plane has the high entropy: mapping [1,0]
        hi = rng.choice([0x3C, 0xBC, 0x3B, 0xBB], n)
    elif name == "lowconst":  # the other two-stream mapping, [0,1]
        lo = np.full(n, 0x55)
    elif name == "zeros":  # mapping [0,0]: the interleaved stream, one run
        lo, hi = np.zeros(n, np.int64), np.zeros(n, np.int64)
    elif name == "repeated":  # [0,0] again, every run one byte long
        lo, hi = np.full(n, 0x7B), np.full(n, 0x3C)
    return widen((lo | (hi << 8)).astype(np.uint16), t)


@pytest.mark.parametrize("raw", [False, True], ids=["tdt", "rawfb"])
@pytest.mark.parametrize("t", list(CODES))
def test_sizes_families_alignments(orc, t, raw):
    """Every size and family, the source 0 / 4 / 8 / 12 bytes and the blob 0 .. 3 bytes off a boundary; dense
    random data and raw fallback give UNCP at w + 4 below and above R, compressible data keeps its TDT bytes."""
    rng = np.random.default_rng(3001)
    cases = [(f, n) for n in SIZES for f in ("gradient", "lowconst", "zeros", "repeated", "dense")]
    srcs = [family(rng, f, n, t) for f, n in cases]
    leads = [4 * (i % 4) for i in range(len(cases))]
    bleads = [(i // 4) % 4 for i in range(len(cases))]
    codec = make_codec(ws=4, options=((TDT_OPT_RAW_FALLBACK, 1),) if raw else ())  # (its own word size plays no part)
    res = run(codec, srcs, [CODES[t]] * len(cases), leads, bleads)
    for (f, n), u, (blob, ln, st) in zip(cases, srcs, res):
        wire = narrow(u, t).tobytes()
        assert (st, ln) == (0, len(blob)) and blob == want(orc, wire, raw), (f, n)
        if n >= 512 and f in ("zeros", "dense"):
            assert (blob[:4] == UNCP) == (raw and f == "dense"), (f, n)


@pytest.mark.parametrize("plane", [0, 1])
def test_runs_at_lane_step_and_chunk_edges(orc, plane):
    """Runs of 254 .. 765 equal bytes (and one longer than a lane may stage) in one plane of otherwise
    run-free data: starting at, ending at and straddling a lane's 16 bytes, and straddling element R."""
    rng = np.random.default_rng(3002 + plane)
    n, srcs = 3 * R, []
    for L in (254, 255, 256, 510, 765, 5000):
        pl = [rng.integers(0, 254, n), 0x3C + (np.arange(n) & 1)]  # (no two equal neighbours in either plane)
        pl[0] = np.where(pl[0] == np.roll(pl[0], 1), pl[0] ^ 1, pl[0])
        for start in (16, R - L // 2, R + 8192 + (-L) % 16, 2 * R + 4101):
            pl[plane][start:start + L] = 0x7E
        srcs.append(widen((pl[0] | (pl[1] << 8)).astype(np.uint16), "bf16"))
    res = run(make_codec(), srcs, [0x13] * len(srcs), leads=[0, 4, 8, 12, 0, 4], bleads=[0, 1, 2, 3, 2, 0])
    for u, (blob, ln, st) in zip(srcs, res):
        assert (st, blob) == (0, want(orc, narrow(u, "bf16").tobytes()))


def test_statuses_in_one_mixed_list(orc):
    rng = np.random.default_rng(3003)
    g = family(rng, "gradient", 2048, "bf16").view(np.uint8)
    small = family(rng, "gradient", 100, "f16").view(np.uint8)  # (UNCP by the 1,024-byte floor)
    exact = len(want(orc, narrow(g.view(np.uint32), "bf16").tobytes()))
    f16len = len(want(orc, narrow(g.view(np.uint32), "f16").tobytes()))
    #        good bf16  one byte short  source lead 2  size % 4 = 2  bad code   good fp16  UNCP short  UNCP exact
    srcs = [g,          g,              g,             g[:-2],       g,         g,         small,      small]
    codes = [0x13,      0x13,           0x13,          0x12,         0x31,      0x12,      0x12,       0x12]
    leads = [0,         4,              2,             0,            0,         8,         0,          12]
    caps = [exact,      exact - 1,      bound(4096),   bound(4096),  bound(4096), f16len,  203,        204]
    stats = [0,         E_CAPACITY,     E_ELEMENT,     E_ELEMENT,    E_ARG,     0,         E_CAPACITY, 0]
    res = run(make_codec(), srcs, codes, leads, [0, 1, 2, 3, 0, 1, 2, 3], caps)
    assert [r[2] for r in res] == stats
    for i, (blob, ln, st) in enumerate(res):  # (run() found the refused blobs' bytes untouched: nothing behind length 0)
        assert ln == (0 if st else caps[i]), i
    assert res[0][0] == want(orc, narrow(g.view(np.uint32), "bf16").tobytes())
    assert res[5][0] == want(orc, narrow(g.view(np.uint32), "f16").tobytes())
    assert res[7][0] == UNCP + narrow(small.view(np.uint32), "f16").tobytes()
    with pytest.raises(TdtError):  # a bad code for the whole call
        run(make_codec(), [g], None, elem=0x31)


@pytest.mark.parametrize("raw", [False, True], ids=["tdt", "rawfb"])
def test_sender_to_receiver(raw):
    """Two peers' float32 tensors through encode_tensors(wire_dtype=bf16) into decode_reduce_tensors(set=True,
    wire_dtype=bf16): the float32 sum of the widened reference halfwords, exactly."""
    rng = np.random.default_rng(3004)
    sizes = (1000, R + 6)
    peers = [[rng.normal(0, 0.01, n).astype(np.float32) for n in sizes] for _ in range(2)]
    codec = make_codec(ws=2, options=((TDT_OPT_RAW_FALLBACK, 1),) if raw else ())
    sent = []
    for p in peers:
        out, slots, lens, st = codec.encode_tensors([torch.from_numpy(x).cuda() for x in p], wire_dtype=torch.bfloat16)
        assert not st.cpu().numpy()[:len(sizes)].any()
        sent.append((out, slots, lens))
    outs = [torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for n in sizes]
    lens, st = codec.decode_reduce_tensors(sent, outs, set=True, wire_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert not st.cpu().numpy()[:len(sizes)].any()
    for i, n in enumerate(sizes):
        a, b = (widen(narrow(p[i].view(np.uint32), "bf16"), "bf16").view(np.float32) for p in peers)
        assert np.array_equal(outs[i].cpu().numpy().view(np.uint32), (a + b).view(np.uint32)), n
