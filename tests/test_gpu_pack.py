"""The packed wire buffer on the GPU: tdt_pack_v (TdtCodec.pack_v), which packs slotted or scattered
blobs back to back with an offset table, and tdt_encode_batch_vp (TdtCodec.encode_vp,
encode_tensors(packed=True)), the scattered and mixed-width encode into such a buffer.  pack_v is
checked against numpy's concatenation; the packed encode against the CPU oracle and against what
encode_v / encode_vw give for the same messages."""
import pathlib
import re

import numpy as np
import pytest

from oracle.oracle import encode_bound
from tests.support import CANARY, E_ARG, E_CAPACITY, E_CAPTURE, E_CONFIG, E_UNSUPPORTED, address_order, mask_of, offsets

torch = pytest.importorskip("torch")
from tests.gpu_support import (_gpu, canaries_intact, guarded, i32, i64, make_codec, orc, own,  # noqa: E402, F401
                               packed_blobs, ptrs)
from tests.mixed_ws_cases import WIDTHS, batch, oracle_blob, records, run_vw  # noqa: E402, F401

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
# the piece of the packed output one workgroup copies: taken from the build, not restated here
P = int(re.search(r"kPackPiece\s*=\s*(\d+)\s*;", (ROOT / "psyne_amd" / "csrc" / "tdt_pack.h").read_text()).group(1))
# below, at and above the 16-byte store and the piece; a blob of several pieces; a run of empty blobs
# (equal neighbouring offsets); and one long enough for many workgroups
LENGTHS = [0, 1, 15, 16, 17, 4095, P - 1, P, P + 1, 3 * P + 5, 0, 0, 0, 0, 0, (1 << 20) + 3]


def guarded_at(cap, phase):
    """guarded(), with the output starting `phase` bytes past a 16-byte boundary."""
    t = torch.full((64 + 16 + cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t, t[64 + phase:64 + phase + cap]


def canaries_around(t, view):
    h = t.cpu().numpy()
    b = view.data_ptr() - t.data_ptr()
    return bool((h[:b] == CANARY).all() and (h[b + view.numel():] == CANARY).all())


@pytest.fixture(scope="module")
def blobs():
    """Every length twice, so that the non-empty blobs start at every phase 0..15 of a 16-byte group."""
    rng = np.random.default_rng(20262)
    host, dev = [], []
    for r in range(2):
        for k, n in enumerate(LENGTHS):
            host.append(rng.integers(0, 256, n, dtype=np.uint8))
            dev.append(own(host[-1], (k + 8 * r) % 16))
    assert {t.data_ptr() % 16 for t in dev if t.numel()} == set(range(16))
    return host, dev


# ------------------------------------------------------------------------------- 1: pack_v against numpy
@pytest.mark.parametrize("order", ["ascending", "shuffled"])
@pytest.mark.parametrize("phase", [0, 1, 8])
def test_pack_v_equals_concatenation(blobs, phase, order):
    host, dev = blobs
    idx = address_order(dev, order)
    want = np.concatenate([host[i] for i in idx])
    t, out = guarded_at(want.size, phase)
    codec = make_codec(4)
    off = torch.full((len(idx) + 1,), 77, dtype=torch.int64, device="cuda")
    st = torch.full((len(idx),), 77, dtype=torch.int32, device="cuda")
    codec.pack_v(ptrs([dev[i] for i in idx]), i64(host[i].size for i in idx), out, out_offsets=off, status=st)
    torch.cuda.synchronize()
    assert off.cpu().numpy().tolist() == offsets([host[i].size for i in idx]).tolist()
    assert int(st.abs().sum()) == 0
    assert np.array_equal(out.cpu().numpy(), want)
    assert canaries_around(t, out)
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 2: pack_v capacity
def check_cut(out_full, off, st, want, cap):
    """After a packed call into the first `cap` bytes of the canary-filled out_full: the blobs that end
    at or before cap are intact, the others have TDT_E_CAPACITY (their own status kept where `want`
    gives one), and every byte from the last fitting blob's end on is unchanged."""
    off, st = np.asarray(off), np.asarray(st)
    fits = off[1:] <= cap
    fit = int(off[1:][fits].max()) if fits.any() else 0
    h = out_full.cpu().numpy()
    assert np.array_equal(h[:fit], want[:fit])
    assert (h[fit:] == CANARY).all()
    return fits


@pytest.mark.parametrize("where", ["inside a blob", "at a blob's end", "zero"])
def test_pack_v_capacity(blobs, where):
    host, dev = blobs
    n = len(LENGTHS)
    host, dev = host[:n], dev[:n]
    off_want = offsets([m.size for m in host])
    want = np.concatenate(host)
    # inside the blob of several pieces (and inside its second piece); at the end of the P-byte blob
    cap = {"inside a blob": int(off_want[9]) + P + 100, "at a blob's end": int(off_want[8]), "zero": 0}[where]
    t, out_full = guarded_at(want.size, 0)
    codec = make_codec(4)
    off, st = codec.pack_v(ptrs(dev), i64(m.size for m in host), out_full[:cap])
    torch.cuda.synchronize()
    off, st = off.cpu().numpy(), st.cpu().numpy()
    assert off.tolist() == off_want.tolist()  # complete, whatever the capacity
    fits = check_cut(out_full, off, st, want, cap)
    assert st.tolist() == [0 if f else E_CAPACITY for f in fits]
    assert canaries_around(t, out_full)
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 3: encode_vp, one width


@pytest.mark.parametrize("w", [4, 12])
def test_encode_vp_one_width(batch, w):
    idx = [i for i, x in enumerate(batch["ws"]) if x == w]
    tensors = [batch["tensors"][i] for i in idx]
    sizes = [t.numel() for t in tensors]
    cap = sum(batch["caps"][i] for i in idx)
    t, out = guarded(cap)
    codec = make_codec(w)
    off, st = codec.encode_vp(ptrs(tensors), i64(sizes), sum(sizes), out)
    torch.cuda.synchronize()
    got, offh = packed_blobs(out, off)
    st = st.cpu().numpy()
    for k, i in enumerate(idx):
        sb, sl, ss = batch["sub"][i]  # what encode_v gives with a slot of the encode bound
        assert (got[k], int(st[k])) == (sb, ss), "message %d (%d bytes)" % (i, sizes[k])
        assert got[k] == batch["blobs"][i] and st[k] == 0, "message %d (%d bytes)" % (i, sizes[k])
    assert canaries_intact(t, cap)
    # and back, from the packed buffer as it is
    back = [torch.full((max(n, 1),), 1, dtype=torch.uint8, device="cuda")[:n] for n in sizes]
    dl, ds = codec.decode_tensors(out, off, off[1:] - off[:-1], back)
    torch.cuda.synchronize()
    assert int(ds.abs().sum()) == 0 and dl.cpu().numpy()[: len(idx)].tolist() == sizes
    for k, i in enumerate(idx):
        assert np.array_equal(back[k].cpu().numpy(), batch["msgs"][i]), "message %d" % i
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 4: encode_vp, mixed widths
@pytest.mark.parametrize("order", ["ascending", "shuffled"])
def test_encode_vp_mixed_equals_encode_vw(batch, order):
    idx, outs, ln, vst, _ = run_vw(batch, order)
    tensors = [batch["tensors"][i] for i in idx]
    sizes = [t.numel() for t in tensors]
    cap = sum(batch["caps"][i] for i in idx)
    t, out = guarded(cap)
    codec = make_codec(2)  # (the context's own width plays no part)
    off, st = codec.encode_vp(ptrs(tensors), i64(sizes), sum(sizes), out, word_sizes=i32(batch["ws"][i] for i in idx),
                              width_mask=mask_of(WIDTHS))
    torch.cuda.synchronize()
    got, offh = packed_blobs(out, off)
    assert np.diff(offh).tolist() == ln[: len(idx)].tolist()
    assert st.cpu().numpy()[: len(idx)].tolist() == vst[: len(idx)].tolist()
    for k, i in enumerate(idx):
        assert got[k] == outs[k][: ln[k]].cpu().numpy().tobytes() == batch["blobs"][i], "message %d" % i
    assert canaries_intact(t, cap)
    assert codec.error_flags() == 0


def test_encode_vp_rejected_widths_occupy_nothing(orc):
    rng = np.random.default_rng(41)
    #        ok  <=0  ok  <=0  >64  not in mask  ok  ok
    widths = [4, 0, 2, -1, 65, 8, 4, 2]
    sizes = [4096, 4096, 32768, 1024, 65536, 4096, 32768, 1000]
    msgs = [records(rng, w if 1 <= w <= 64 else 4, n) for w, n in zip(widths, sizes)]
    tensors = [own(m) for m in msgs]
    caps = [encode_bound(n, 8) for n in sizes]
    outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    codec = make_codec(4)
    ln, vst = codec.encode_vw(ptrs(tensors), i64(sizes), i32(widths), mask_of([2, 4]), ptrs(outs), i64(caps))
    torch.cuda.synchronize()
    ln, vst = ln.cpu().numpy(), vst.cpu().numpy()
    assert vst.tolist() == [0, E_CONFIG, 0, E_CONFIG, E_UNSUPPORTED, E_ARG, 0, 0]
    t, out = guarded(sum(caps))
    off, st = codec.encode_vp(ptrs(tensors), i64(sizes), sum(sizes), out, word_sizes=i32(widths),
                              width_mask=mask_of([2, 4]))
    torch.cuda.synchronize()
    got, offh = packed_blobs(out, off)
    assert st.cpu().numpy().tolist() == vst.tolist()
    assert np.diff(offh).tolist() == ln.tolist()
    for k, (m, w) in enumerate(zip(msgs, widths)):
        if vst[k]:
            assert offh[k + 1] == offh[k], "message %d" % k  # no bytes
        else:
            assert got[k] == outs[k][: ln[k]].cpu().numpy().tobytes() == oracle_blob(orc, m, w), "message %d" % k
    assert (out[int(offh[-1]):].cpu().numpy() == CANARY).all() and canaries_intact(t, sum(caps))
    assert codec.error_flags() == 0


def test_encode_vp_call_level_errors():
    from psyne_amd._lib import TdtError
    t = own(records(np.random.default_rng(42), 4, 1024))
    out = torch.zeros(encode_bound(1024, 4), dtype=torch.uint8, device="cuda")
    codec = make_codec(4)
    for mask in (0, 0x1ff):  # no width; nine widths
        with pytest.raises(TdtError) as ei:
            codec.encode_vp(ptrs([t]), i64([1024]), 1024, out, word_sizes=i32([4]), width_mask=mask)
        assert ei.value.code == E_ARG
    # a batch without messages touches nothing
    e = torch.empty(0, dtype=torch.int64, device="cuda")
    off = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    codec.encode_vp(e, e, 0, out, out_offsets=off)
    codec.pack_v(e, e, out, out_offsets=off)
    torch.cuda.synchronize()
    assert int(off[0]) == 77


# ------------------------------------------------------------------------------- 5: capacities, understated totals
@pytest.mark.parametrize("where", ["inside a blob", "at a blob's end"])
def test_encode_vp_out_cap_cuts_the_batch(batch, where):
    idx = [i for i, x in enumerate(batch["ws"]) if x == 4]
    tensors = [batch["tensors"][i] for i in idx]
    sizes = [t.numel() for t in tensors]
    off_want = offsets([len(batch["blobs"][i]) for i in idx])
    want = np.frombuffer(b"".join(batch["blobs"][i] for i in idx), np.uint8)
    k = len(idx) // 2
    cap = int(off_want[k + 1]) if where == "at a blob's end" else int(off_want[k] + off_want[k + 1]) // 2
    t, out_full = guarded(int(off_want[-1]))
    codec = make_codec(4)
    off, st = codec.encode_vp(ptrs(tensors), i64(sizes), sum(sizes), out_full[:cap])
    torch.cuda.synchronize()
    off, st = off.cpu().numpy(), st.cpu().numpy()
    assert off.tolist() == off_want.tolist()  # (off[n]: what the whole batch needs)
    fits = check_cut(out_full, off, st, want, cap)
    assert 0 < fits.sum() < len(idx)
    assert st[: len(idx)].tolist() == [0 if f else E_CAPACITY for f in fits]
    assert canaries_intact(t, int(off_want[-1]))
    assert codec.error_flags() == 0


def test_encode_vp_understated_total_is_clamped(batch):
    """total_bytes at half the true sum: the scratch holds the slots of the first messages only, and
    every message whose slot would end past it gets TDT_E_CAPACITY (its slot's capacity is 0), the
    earlier ones their exact blobs."""
    idx = [i for i, x in enumerate(batch["ws"]) if x == 4]
    tensors = [batch["tensors"][i] for i in idx]
    sizes = [t.numel() for t in tensors]
    n, half = len(idx), sum(sizes) // 2
    scratch = 2 * half + n * (28 + 4 * 4)  # (a fresh context: the scratch is exactly this)
    slot_end = np.cumsum([encode_bound(s, 4) for s in sizes])
    inside = slot_end <= scratch
    assert 0 < inside.sum() < n
    lens = [len(batch["blobs"][i]) if ok else 0 for i, ok in zip(idx, inside)]
    cap = sum(batch["caps"][i] for i in idx)
    t, out = guarded(cap)
    codec = make_codec(4)
    off, st = codec.encode_vp(ptrs(tensors), i64(sizes), half, out)
    torch.cuda.synchronize()
    got, offh = packed_blobs(out, off)
    assert offh.tolist() == offsets(lens).tolist()
    assert st.cpu().numpy()[:n].tolist() == [0 if ok else E_CAPACITY for ok in inside]
    for k, i in enumerate(idx):
        assert got[k] == (batch["blobs"][i] if inside[k] else b""), "message %d" % i
    assert (out[int(offh[-1]):].cpu().numpy() == CANARY).all() and canaries_intact(t, cap)
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 6: capture
class _Packed:
    """encode_vp over fixed tensors of widths 2, 4 and 12 (mixed), or all at width 12 (one width)."""
    WS = [2, 4, 12, 4, 2, 12, 4, 2]
    NS = [1000, 4096, 4104, 32768, 65536, 32784, 100000, 262208]

    def __init__(self, mixed):
        self.ws = self.WS if mixed else [12] * len(self.NS)
        self.c = make_codec(4 if mixed else 12)
        self.msgs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in self.NS]
        self.out = torch.zeros(sum(encode_bound(n, w) for n, w in zip(self.NS, self.ws)), dtype=torch.uint8, device="cuda")
        self.tab = [ptrs(self.msgs), i64(self.NS), i32(self.ws) if mixed else None]
        self.mask = mask_of(self.ws) if mixed else 0
        self.off = torch.zeros(len(self.NS) + 1, dtype=torch.int64, device="cuda")
        self.st = torch.zeros(len(self.NS), dtype=torch.int32, device="cuda")

    def fill(self, seed):
        rng = np.random.default_rng(seed)
        host = [records(rng, w, n) for w, n in zip(self.ws, self.NS)]
        for t, m in zip(self.msgs, host):
            t.copy_(torch.from_numpy(m))
        return host

    def run(self):
        p, n, w = self.tab
        self.c.encode_vp(p, n, sum(self.NS), self.out, word_sizes=w, width_mask=self.mask, out_offsets=self.off,
                         status=self.st)

    def check(self, orc, host):
        torch.cuda.synchronize()
        got, _ = packed_blobs(self.out, self.off)
        assert int(self.st.abs().sum()) == 0
        for i, m in enumerate(host):
            assert got[i] == oracle_blob(orc, m, self.ws[i]), i


@pytest.mark.parametrize("mixed", [False, True])
def test_packed_capture_on_cold_context_is_refused(mixed):
    from psyne_amd._lib import TdtError
    s = _Packed(mixed)
    s.fill(4)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with pytest.raises(TdtError) as ei:
        with torch.cuda.graph(gr):
            s.run()
    assert ei.value.code == E_CAPTURE


@pytest.mark.parametrize("mixed", [False, True])
def test_packed_capture_replays(orc, mixed):
    s = _Packed(mixed)
    host = s.fill(1)
    s.run()  # eager: the scratch, the tables and the workspaces of this batch exist from here on
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
def test_encode_tensors_packed(orc):
    g = torch.Generator(device="cuda")
    g.manual_seed(13)

    def sparse(n):
        return torch.randn(n, device="cuda", generator=g) * (torch.rand(n, device="cuda", generator=g) > 0.7)

    f32 = [sparse(n) for n in (1024, 16384, 80000)]
    tensors = f32 + [f32[1].to(torch.bfloat16), f32[2].to(torch.bfloat16), f32[1].to(torch.float64),
                     torch.zeros(0, dtype=torch.bfloat16, device="cuda"),
                     torch.rand(16384, device="cuda", generator=g)]  # dense mantissas: a blob above its size
    raw = [t.contiguous().view(torch.uint8).cpu().numpy() if t.numel() else np.zeros(0, np.uint8) for t in tensors]
    want = [oracle_blob(orc, r, t.element_size()) for r, t in zip(raw, tensors)]
    # why `out` defaults to the sum of the encode bounds and not to the sizes plus a margin
    assert len(want[-1]) > raw[-1].size + 4 + 64
    codec = make_codec(4)
    out, off, st = codec.encode_tensors(tensors, word_sizes="dtype", packed=True)
    torch.cuda.synchronize()
    assert off.numel() == len(tensors) + 1 and off.is_cuda
    assert int(st.abs().sum()) == 0
    got, offh = packed_blobs(out, off)
    assert offh.tolist() == offsets([len(b) for b in want]).tolist()
    assert got == want
    fresh = [torch.full_like(t, 1) for t in tensors]
    dl, ds = codec.decode_tensors(out, off, off[1:] - off[:-1], fresh)  # the docstring's round trip
    torch.cuda.synchronize()
    assert int(ds.abs().sum()) == 0
    for a, b in zip(tensors, fresh):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # every tensor at the context's width
    out4, off4, st4 = codec.encode_tensors(tensors, packed=True)
    torch.cuda.synchronize()
    assert int(st4.abs().sum()) == 0
    assert packed_blobs(out4, off4)[0] == [oracle_blob(orc, r, 4) for r in raw]
    # a caller's smaller buffer: capacity statuses, and the need in offsets[n]
    small = torch.zeros(int(offh[3]), dtype=torch.uint8, device="cuda")
    _, offs, sts = codec.encode_tensors(tensors, out=small, word_sizes="dtype", packed=True)
    torch.cuda.synchronize()
    assert offs.cpu().numpy().tolist() == offh.tolist()
    assert sts.cpu().numpy()[: len(tensors)].tolist() == [0 if e <= small.numel() else E_CAPACITY for e in offh[1:]]
    # packed=False: the slotted form, as before
    outs, slots, ln, sst = codec.encode_tensors(tensors, word_sizes="dtype")
    torch.cuda.synchronize()
    assert int(sst.abs().sum()) == 0
    oh, sl, lh = outs.cpu().numpy(), slots.cpu().numpy(), ln.cpu().numpy()
    assert sl.tolist() == offsets([encode_bound(r.size, t.element_size()) for r, t in zip(raw, tensors)]).tolist()
    assert [oh[sl[i]:sl[i] + lh[i]].tobytes() for i in range(len(tensors))] == want
    assert codec.error_flags() == 0
