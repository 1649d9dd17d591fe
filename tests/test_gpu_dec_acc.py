"""Decode-accumulate on the GPU (tdt_decode_accumulate_v, decode_tensors(accumulate=True)): decoded
messages ADDED to their destinations as f32 / f16 / bf16 / f64 elements, on every route of the
scattered decode.  The reference is the correctly rounded sum: float64 on the CPU, rounded once to
the element type (53 bits >= 2p + 2 for every type here, so the device's own form — a packed half
add, or an fp32 add then a rounding — gives the same bits), compared bitwise.  No NaN and no Inf
go in; +-0, subnormals and pairs whose sum overflows do."""
import numpy as np
import pytest

from tests.decode_cases import serialize
from tests.support import CANARY, E_ARG, E_CAPACITY, E_MAGIC, E_TRUNCATED, E_UNSUPPORTED, gradient

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, guarded, i64, make_codec, orc, own, ptrs  # noqa: E402, F401

pytestmark = pytest.mark.gpu

E_ELEMENT, LARGE_MIN = 13, 1  # (status and option numbers of include/psyne_tdt.h)
# name: (element code, element size, exponent mask)
TYPES = {"f32": (1, 4, 0x7F800000), "f16": (2, 2, 0x7C00), "bf16": (3, 2, 0x7F80), "f64": (4, 8, 0x7FF << 52)}
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
FLOAT = {"f32": np.float32, "f16": np.float16, "f64": np.float64}
UNCP = b"PCNU"


def finite(raw, t):
    """The bytes `raw` as elements of type t (their uint view), Inf and NaN patterns made finite."""
    _, es, mask = TYPES[t]
    u = np.frombuffer(bytes(raw), UINT[es]).copy()
    low = UINT[es](mask & -mask)
    u[(u & UINT[es](mask)) == UINT[es](mask)] ^= low
    return u


def specials(t):
    """(message, destination) element pairs: max + max and its negative (overflow), +0 + -0, -0 + -0,
    the smallest subnormal twice, the largest subnormal minus the smallest."""
    _, es, mask = TYPES[t]
    mant, sign = (mask & -mask) - 1, 1 << (8 * es - 1)
    top = (mask - (mask & -mask)) | mant
    return (np.array([top, top | sign, 0, sign, 1, mant], UINT[es]),
            np.array([top, top | sign, sign, sign, 1, 1 | sign], UINT[es]))


def to_f64(u, t):
    if t == "bf16":
        return (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return u.view(FLOAT[t]).astype(np.float64)


def rounded_sum(dst, dec, t):
    """dst + dec as uint views of type t: the float64 sum rounded once."""
    with np.errstate(over="ignore"):
        s = to_f64(dst, t) + to_f64(dec, t)
        if t == "bf16":  # (float64 -> fp32 -> bf16 is still one rounding of such a sum: 24 >= 2 * 8 + 2)
            w = s.astype(np.float32).view(np.uint32)
            return ((w + 0x7FFF + ((w >> 16) & 1)) >> 16).astype(np.uint16)
        return s.astype(FLOAT[t]).view(dst.dtype)


def rle(b):
    """simple_rle_compress: (count, value) pairs, runs cut at 255."""
    out = bytearray()
    starts = np.r_[0, np.flatnonzero(np.diff(b)) + 1, b.size]
    for s, e in zip(starts[:-1], starts[1:]):
        for c in range(s, e, 255):
            out += bytes([min(255, e - c), b[s]])
    return bytes(out)


def crafted(msg, ws, mapping, keep=1.0):
    """The blob of `msg` at word size ws with the streams of `mapping`; keep < 1 cuts every stream's
    pairs short, so the decoder fills the rest with zeros."""
    words = np.frombuffer(bytes(msg), np.uint8).reshape(-1, ws)
    streams = [rle(words[:, [b for b in range(ws) if mapping[b] == s]].ravel()) for s in range(max(mapping) + 1)]
    return serialize(words.size, ws, mapping, [s[:int(len(s) * keep) & ~1] for s in streams])


def shapes(orc, rng, t):
    """(blob, decoded uint view) of every kernel path's smallest shapes, in type t."""
    _, es, _ = TYPES[t]
    src, _ = specials(t)
    out = []

    def msg(n, kind):
        u = finite(gradient(rng, n + 3)[:n] if kind == "grad" else rng.integers(0, 256, n, dtype=np.uint8), t)
        u[:src.size] = src
        return u

    def add(blob):
        st, dec = orc.decode(blob)
        out.append((blob, finite(dec, t)))
        assert st == 0 and out[-1][1].tobytes() == dec, "a bad blob, or a NaN or an Inf in the decoded message"

    cfg = orc.config(word_size=es, sample_fraction=1.0)
    for kind in ("grad", "bits"):
        add(orc.encode(msg(512, kind), cfg=cfg, bandwidth=10.0))  # below min_tensor_size: the 16-lane copy list
        assert out[-1][0][:4] == UNCP
        add(UNCP + msg(80 * 1024 + 8, kind).tobytes())  # one-wave copy (tiled at the lowered threshold)
        add(UNCP + msg(70000, kind).tobytes())  # the same, a partial last tile
        # small class and its edge, main class, a partial last group, the list dispatched first, three tiles
        # (100,004 or 100,008: whole elements, no multiple of 16, and of 4 as the encoder's TDT route asks)
        for n in (1024, 8192, 8208, 65536, 100000 + max(es, 4), 131072 + 16, 98304 + 16):
            add(orc.encode(msg(n, kind), cfg=cfg, bandwidth=10.0))
            assert out[-1][0][:4] == b"DTDT"
        # decode_one's generic path: three referenced streams; width 8 with shares of 3 and 5
        add(crafted(msg(2088, kind), 4, [0, 1, 2, 2]))
        add(crafted(msg(2088, kind), 8, [0, 0, 0, 1, 1, 1, 1, 1]))
        add(crafted(msg(4096, kind), 4, [0, 0, 0, 1], keep=0.5))  # both streams end early: zeros are added
    return out


class _List:
    """Messages on the GPU, each blob at an odd address and each destination between guards."""

    def __init__(self, t, items, phases, codes=None, caps=None):
        self.t, self.items, self.phases = t, items, phases
        self.blobs = [own(b, lead=1) for b, _ in items]
        self.caps = caps or [d.nbytes for _, d in items]
        self.outs = [guarded(c, lead=p) for c, p in zip(self.caps, phases)]
        self.codes = codes or [TYPES[t][0]] * len(items)
        self.elems = torch.tensor(self.codes, dtype=torch.uint8, device="cuda")
        self.args = (ptrs(self.blobs), i64(b.numel() for b in self.blobs), ptrs(v for _, v in self.outs), i64(self.caps))

    def fill(self, rng):
        """Random finite destinations (-0.0 where the message decodes to zeros, the specials' partners first)."""
        self.before = []
        es = TYPES[self.t][1]
        for (_, dec), (_, v), cap in zip(self.items, self.outs, self.caps):
            u = finite(rng.integers(0, 256, cap // es * es, dtype=np.uint8), self.t)
            if dec.itemsize == es and dec.size == u.size:
                u[dec == 0] = 1 << (8 * es - 1)
            u[:min(6, u.size)] = specials(self.t)[1][:u.size]
            b = np.r_[u.view(np.uint8), np.zeros(cap - u.nbytes, np.uint8)]
            v.copy_(torch.from_numpy(b))
            self.before.append(b)

    def run(self, codec):
        return codec.decode_accumulate_v(*self.args, elems=self.elems)

    def got(self, i):
        return self.outs[i][1].cpu().numpy()

    def guards_intact(self, i):
        h, lo = self.outs[i][0].cpu().numpy(), 64 + self.phases[i]
        return bool((h[:lo] == CANARY).all() and (h[lo + self.caps[i]:] == CANARY).all())


@pytest.mark.parametrize("t", list(TYPES))
def test_every_route_sums_bitwise(orc, t):
    rng, es = np.random.default_rng(2611), TYPES[t][1]
    items = shapes(orc, rng, t)
    L = _List(t, items * 3, [p for p in (0, es, 16 - es) for _ in items])
    for options in ((), ((LARGE_MIN, 65536),)):  # one-wave routes; then everything above 64 KiB as tiles
        L.fill(rng)
        lens, st = L.run(make_codec(options=options))
        torch.cuda.synchronize()
        lens, st = lens.cpu().numpy(), st.cpu().numpy()
        for i, (_, dec) in enumerate(L.items):
            want = rounded_sum(L.before[i].view(dec.dtype), dec, t)
            assert (st[i], lens[i]) == (0, dec.nbytes), (i, options)
            assert np.array_equal(L.got(i).view(dec.dtype), want), (i, dec.nbytes, options)
            assert L.guards_intact(i), i


def test_mixed_list_of_sums_and_stores(orc):
    rng = np.random.default_rng(2612)
    items, codes, types = [], [], []
    for t, store in [("f32", False), ("f16", False), ("bf16", False), ("f64", False), ("f32", True), ("f16", True)]:
        es = TYPES[t][1]
        m = finite(gradient(rng, 4096 + 16 * es), t)
        items.append((orc.encode(m, cfg=orc.config(word_size=es), bandwidth=10.0), m))
        codes.append(0 if store else TYPES[t][0])
        types.append(t)
    m12 = rng.integers(0, 3, 2400, dtype=np.uint8)  # a generic width, stored through the deferred kernel
    items.append((orc.encode(m12, cfg=orc.config(word_size=12), bandwidth=10.0), m12.view(np.uint32)))
    codes, types = codes + [0], types + ["f32"]
    assert items[-1][0][12:16] == (12).to_bytes(4, "little")
    L = _List("f32", items, [0] * len(items), codes=codes)
    dests = [finite(rng.integers(0, 256, dec.nbytes, dtype=np.uint8), t) for (_, dec), t in zip(items, types)]
    for b, (_, v) in zip(dests, L.outs):
        v.copy_(torch.from_numpy(b.view(np.uint8)))
    want = [dec if c == 0 else rounded_sum(b, dec, t) for (_, dec), c, b, t in zip(items, codes, dests, types)]
    lens, st = L.run(make_codec())
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and lens.cpu().tolist() == [d.nbytes for _, d in items]
    for i, w in enumerate(want):
        assert np.array_equal(L.got(i), w.view(np.uint8)), i
    # the tensor call derives the codes from the dtypes: the four sums again, on top of the first
    tt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
    outs = [L.outs[i][1].view(tt[types[i]]) for i in range(4)]
    blob = torch.cat(L.blobs[:4])
    off = i64(np.cumsum([0] + [b.numel() for b in L.blobs[:4]]))
    _, st = make_codec().decode_tensors(blob, off, off[1:] - off[:-1], outs, accumulate=True)
    torch.cuda.synchronize()
    assert not st.cpu().numpy()[:4].any()
    for i in range(4):
        assert np.array_equal(L.got(i), rounded_sum(want[i], items[i][1], types[i]).view(np.uint8)), i
    with pytest.raises(ValueError):
        make_codec().decode_tensors(blob, off, off[1:] - off[:-1], [outs[0].view(torch.int32)], accumulate=True)


# kind: (element type, destination phase, capacity short by, expected status, blob edit)
REFUSALS = {
    "phase_1": ("f32", 1, 0, E_ELEMENT, None),
    "size_not_elements": ("f64", 0, 0, E_ELEMENT, None),
    "capacity": ("f32", 0, 1, E_CAPACITY, None),
    "width_12": ("f32", 0, 0, E_UNSUPPORTED, 12),
    "truncated": ("f32", 0, 0, E_TRUNCATED, "cut"),
    "bad_magic": ("f32", 0, 0, E_MAGIC, "magic"),
}


@pytest.mark.parametrize("n", [1028, 98308], ids=["one_wave", "tiled"])
@pytest.mark.parametrize("kind", list(REFUSALS))
def test_refused_message_is_untouched(orc, kind, n):
    t, phase, short, status, edit = REFUSALS[kind]
    rng = np.random.default_rng(2613)
    if edit == 12:  # (whole 12-byte words, and above min_tensor_size)
        n = 1200 if n < 65536 else 98304
    m = finite(gradient(rng, n), "f32")  # (1,028 and 98,308 bytes: whole f32 elements, no whole f64 ones)
    blob = orc.encode(m, cfg=orc.config(word_size=12 if edit == 12 else 4), bandwidth=10.0)
    if edit == "cut":
        blob = blob[:len(blob) - 7]
    elif edit == "magic":
        blob = b"XXXX" + blob[4:]
    good = finite(gradient(rng, 2048), t)
    items = [(blob, m), (orc.encode(good, cfg=orc.config(word_size=4), bandwidth=10.0), good)]
    L = _List(t, items, [phase, 0], caps=[m.nbytes - short, good.nbytes])
    L.fill(rng)
    lens, st = L.run(make_codec(options=((LARGE_MIN, 65536),)))
    torch.cuda.synchronize()
    assert st.cpu().tolist()[:2] == [status, 0] and lens.cpu().tolist()[:2] == [0, good.nbytes]
    assert np.array_equal(L.got(0), L.before[0]) and L.guards_intact(0)
    assert np.array_equal(L.got(1).view(good.dtype), rounded_sum(L.before[1].view(good.dtype), good, t))


def test_unknown_element_code_is_an_argument_error(orc):
    from psyne_amd._lib import TdtError
    m = finite(gradient(np.random.default_rng(2614), 2048), "f32")
    L = _List("f32", [(orc.encode(m, bandwidth=10.0), m)] * 2, [0, 0], codes=[5, 1])
    L.fill(np.random.default_rng(1))
    lens, st = L.run(make_codec())
    torch.cuda.synchronize()
    assert st.cpu().tolist()[:2] == [E_ARG, 0] and lens.cpu().tolist()[:2] == [0, m.nbytes]
    assert np.array_equal(L.got(0), L.before[0])
    with pytest.raises(TdtError) as ei:
        make_codec().decode_accumulate_v(*L.args, elem=5)
    assert ei.value.code == E_ARG


def test_captured_call_adds_on_every_replay(orc):
    rng = np.random.default_rng(2615)
    items = []
    for n in (512, 4096, 65536 + 16):
        m = finite(gradient(rng, n), "f32")
        m[m.view(np.float32) == 0] = 0  # (+0 only: x + d + d below is then two roundings of finite sums)
        items.append((orc.encode(m, bandwidth=10.0), m))
    L, codec = _List("f32", items, [0, 4, 12]), make_codec()
    L.fill(rng)
    L.run(codec)  # eager: the workspaces exist from here on
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        L.run(codec)
    gr.replay()
    gr.replay()
    torch.cuda.synchronize()
    for i, (_, dec) in enumerate(items):
        want = L.before[i].view(dec.dtype)
        for _ in range(3):  # the eager call and two replays (a capture itself runs nothing)
            want = rounded_sum(want, dec, "f32")
        assert np.array_equal(L.got(i).view(dec.dtype), want), i
    assert codec.error_flags() == 0
