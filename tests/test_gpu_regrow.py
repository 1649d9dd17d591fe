"""Buffers of a context that grow and are then used by a smaller call (psyne_amd/csrc/tdt_grow.h: every
workspace of the batch API grows through one function).  One context per entry-point family, the calls
small -> large -> small: the large batch makes the family's buffers grow, the small one after it runs in
the grown buffers.  Every batch's blobs (encode) or bytes (decode) are checked against the CPU oracle,
never against another GPU call."""
import ctypes as C

import numpy as np
import pytest

from oracle.oracle import Oracle, encode_bound
from tests.support import E_CAPTURE, gradient, mask_of, offsets_of

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, i32, i64, make_codec  # noqa: E402, F401

pytestmark = pytest.mark.gpu

ORDER = ("small", "large", "small")


class _Ref:
    """The batches, and the oracle's blobs of each at a width per message (computed once, shared)."""

    def __init__(self):
        rng = np.random.default_rng(20264)
        self.orc = Oracle()
        self.msgs = {
            "small": [gradient(rng, 2048) for _ in range(4)],
            # 600 x 2 KiB and one 100 KiB message: the compacted encode takes its two phases
            "large": [gradient(rng, 2048) for _ in range(600)] + [gradient(rng, 100 * 1024)],
            # one message more than a single 8,192-message scan chunk holds: the chunk sums are needed
            "tiny": [rng.integers(0, 256, 64, dtype=np.uint8) for _ in range(8200)],
        }
        self._blobs = {}

    def blobs(self, name, widths):
        """widths: one int, or one per message"""
        msgs = self.msgs[name]
        ws = [widths] * len(msgs) if isinstance(widths, int) else list(widths)
        key = (name, tuple(ws))
        if key not in self._blobs:
            cfg = {w: self.orc.config(word_size=w, sample_fraction=1.0) for w in set(ws)}
            self._blobs[key] = [self.orc.encode(m, cfg=cfg[w], bandwidth=10.0) for m, w in zip(msgs, ws)]
        return self._blobs[key]


@pytest.fixture(scope="module")
def ref():
    return _Ref()


def _concat(parts):
    """(bytes back to back, offsets) of a list of byte strings / uint8 arrays"""
    arrs = [np.frombuffer(p, np.uint8) if isinstance(p, (bytes, bytearray)) else p for p in parts]
    return np.concatenate(arrs), offsets_of(arrs)


def _split(buf, off):
    return [buf[off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == (w if isinstance(w, bytes) else w.tobytes()), "%s: message %d" % (what, i)


# ---------------------------------------------------------------------------- compacted, word size 4
def _compacted_encode(codec, ref, name, ws):
    data, off = _concat(ref.msgs[name])
    out, eoff, st = codec.encode_batch(torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda())
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0, name
    _same(_split(out.cpu().numpy(), eoff.cpu().numpy()), ref.blobs(name, ws), "encode_batch " + name)


def _compacted_decode(codec, ref, name, ws):
    blobs, boff = _concat(ref.blobs(name, ws))
    out, doff, st = codec.decode_batch(torch.from_numpy(blobs).cuda(), torch.from_numpy(boff).cuda())
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0, name
    _same(_split(out.cpu().numpy(), doff.cpu().numpy()), ref.msgs[name], "decode_batch " + name)


def test_compacted_ws4(ref):
    """cp_idx, cp_buf and the plan buffer (two phases), then the chunk sums of the scan (8,200
    messages), then the look-back workspace (the one-pass kernels, forced by the option)."""
    from psyne_amd._lib import TDT_OPT_NO_TWO_PHASE
    codec = make_codec(4)
    for name in ORDER + ("tiny", "small"):
        _compacted_encode(codec, ref, name, 4)
        _compacted_decode(codec, ref, name, 4)
    codec.set_option(TDT_OPT_NO_TWO_PHASE, 1)
    for name in ORDER:
        _compacted_encode(codec, ref, name, 4)
        _compacted_decode(codec, ref, name, 4)
    assert codec.error_flags() == 0


def test_compacted_encode_ws12(ref):
    """the generic width's compacted encode: always the two phases"""
    codec = make_codec(12)
    for name in ORDER:
        _compacted_encode(codec, ref, name, 12)
    assert codec.error_flags() == 0


# ---------------------------------------------------------------------------- scattered
class _Scattered:
    """A batch as a scattered call sees it: every message (or blob) at its own address, every output
    in a slot of its own capacity."""

    def __init__(self, parts, caps):
        data, off = _concat(parts)
        self.src = torch.from_numpy(data).cuda()
        self.ptrs = i64(self.src.data_ptr() + off[:-1])
        self.sizes = i64(np.diff(off))
        self.slots = np.zeros(len(caps) + 1, np.int64)
        self.slots[1:] = np.cumsum(caps)
        self.out = torch.zeros(int(self.slots[-1]), dtype=torch.uint8, device="cuda")
        self.out_ptrs = i64(self.out.data_ptr() + self.slots[:-1])
        self.caps = i64(caps)

    def outputs(self, lengths):
        h, ln = self.out.cpu().numpy(), lengths.cpu().numpy()
        return [h[self.slots[i]:self.slots[i] + ln[i]].tobytes() for i in range(len(self.slots) - 1)]


def test_scattered_v(ref):
    codec = make_codec(4)
    for name in ORDER:
        msgs, want = ref.msgs[name], ref.blobs(name, 4)
        e = _Scattered(msgs, [encode_bound(m.size, 4) for m in msgs])
        ln, st = codec.encode_v(e.ptrs, e.sizes, e.out_ptrs, e.caps)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0, name
        _same(e.outputs(ln), want, "encode_v " + name)
        d = _Scattered(want, [m.size for m in msgs])
        ln, st = codec.decode_v(d.ptrs, d.sizes, d.out_ptrs, d.caps)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0, name
        _same(d.outputs(ln), msgs, "decode_v " + name)
    assert codec.error_flags() == 0


def test_scattered_vw(ref):
    codec = make_codec(4)
    for name in ORDER:
        msgs = ref.msgs[name]
        widths = [4 if i % 2 == 0 else 12 for i in range(len(msgs))]
        e = _Scattered(msgs, [encode_bound(m.size, w) for m, w in zip(msgs, widths)])
        ln, st = codec.encode_vw(e.ptrs, e.sizes, i32(widths), mask_of(widths), e.out_ptrs, e.caps)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0, name
        _same(e.outputs(ln), ref.blobs(name, widths), "encode_vw " + name)
    assert codec.error_flags() == 0


def _packed(codec, ref, name, out=None, off=None, st=None):
    msgs = ref.msgs[name]
    e = _Scattered(msgs, [1] * len(msgs))  # (its own outputs are unused: the blobs go into `out`, packed)
    total = sum(m.size for m in msgs)
    if out is None:
        out = torch.zeros(sum(encode_bound(m.size, 4) for m in msgs), dtype=torch.uint8, device="cuda")
    off, st = codec.encode_vp(e.ptrs, e.sizes, total, out, out_offsets=off, status=st)
    return e, out, off, st


def _check_packed(ref, name, out, off, st):
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0, name
    _same(_split(out.cpu().numpy(), off.cpu().numpy()), ref.blobs(name, 4), "encode_vp " + name)


def test_scattered_vp(ref):
    codec = make_codec(4)
    for name in ORDER:
        _, out, off, st = _packed(codec, ref, name)
        _check_packed(ref, name, out, off, st)
    assert codec.error_flags() == 0


def test_refused_capture_leaves_the_context_usable(ref):
    """A captured tdt_encode_batch_vp on a cold context is refused (its buffers would have to grow);
    the same batch then runs eagerly on that context, and a capture of it replays to the same bytes."""
    from psyne_amd._lib import TdtError
    codec = make_codec(4)
    msgs = ref.msgs["small"]
    e = _Scattered(msgs, [1] * len(msgs))
    total = sum(m.size for m in msgs)
    out = torch.zeros(sum(encode_bound(m.size, 4) for m in msgs), dtype=torch.uint8, device="cuda")
    off = torch.zeros(len(msgs) + 1, dtype=torch.int64, device="cuda")
    st = torch.zeros(len(msgs), dtype=torch.int32, device="cuda")

    def run():
        codec.encode_vp(e.ptrs, e.sizes, total, out, out_offsets=off, status=st)

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(TdtError) as ei:
        with torch.cuda.graph(g):
            run()
    assert ei.value.code == E_CAPTURE
    run()  # eager
    _check_packed(ref, "small", out, off, st)
    eager = (out.cpu().numpy().copy(), off.cpu().numpy().copy())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    out.zero_()
    off.zero_()
    g.replay()
    _check_packed(ref, "small", out, off, st)
    assert np.array_equal(off.cpu().numpy(), eager[1]) and np.array_equal(out.cpu().numpy(), eager[0])
    assert codec.error_flags() == 0


# ---------------------------------------------------------------------------- host pipeline
def test_host_pageable(ref):
    codec = make_codec(4)
    for name in ORDER:
        msgs, want = ref.msgs[name], ref.blobs(name, 4)
        data, off = _concat(msgs)
        out, ooff, st = codec.encode_host(data, off)
        assert int(np.abs(st).sum()) == 0, name
        _same(_split(out, ooff.astype(np.int64)), want, "encode_host " + name)
        blobs, boff = _concat(want)
        back, doff, st = codec.decode_host(blobs, boff, data.size)
        assert int(np.abs(st).sum()) == 0, name
        _same(_split(back, doff.astype(np.int64)), msgs, "decode_host " + name)
    assert codec.error_flags() == 0


def test_host_gather(ref):
    from psyne_amd._lib import check
    codec = make_codec(4)
    for name in ORDER:
        msgs = [np.ascontiguousarray(m) for m in ref.msgs[name]]
        n = len(msgs)
        ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in msgs])
        sz = np.array([m.size for m in msgs], np.uint64)
        cap = sum(encode_bound(m.size, 4) for m in msgs)
        out = np.empty(cap, np.uint8)
        ooff = np.zeros(n + 1, np.uint64)
        st = np.zeros(n, np.int32)
        check(codec._lib.tdt_encode_host_v(codec._h, C.addressof(ptrs), sz.ctypes.data, n, out.ctypes.data, cap,
                                           ooff.ctypes.data, st.ctypes.data))
        assert int(np.abs(st).sum()) == 0, name
        _same(_split(out, ooff.astype(np.int64)), ref.blobs(name, 4), "encode_host_v " + name)
    assert codec.error_flags() == 0
