"""The shared funnel-shift copy (psyne_amd/csrc/tdt_copy.h) at its own edge shapes, through every
route that owns one of its call sites: the UNCP passthrough lists of the slotted and the scattered
encode and decode, the two-phase compaction gather, the host pipeline's output copies (encode below
the look-back limit, the slotted chunk's gather, decode; pageable and pinned caller buffers) and
pack_v.  One batch of about 200 short messages whose lengths sweep the 16-byte store's edges, with
sources and destinations at every residue of a 16-byte group; every output is compared byte for
byte with the oracle's blobs (or the plain concatenation) inside a canary-filled buffer, so a byte
written before or after any output shows."""
import ctypes as C

import numpy as np
import pytest

from oracle.oracle import Oracle, encode_bound
from tests.support import CANARY, gradient, offsets, phased_slots

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, dev, i64  # noqa: E402, F401

pytestmark = pytest.mark.gpu

# below, at and above one, two, ... five 16-byte chunks, and around a wave's and the 4 KiB boundary
EDGES = [255, 256, 257, 4095, 4096, 4097]
LENGTHS = list(range(81)) + EDGES + list(range(80, -1, -1)) + EDGES + [13, 29, 47, 61, 5, 77, 3, 19, 1, 0]
BIG = 70000 * 4  # one message above 64 KiB: the two-phase compaction, the host pipeline's slotted chunk
ALL16 = set(range(16))


def make_codec(policy=True):
    from psyne_amd import TDTConfig, TdtCodec
    c = TdtCodec(TDTConfig(sample_fraction=1.0))
    c.set_metrics(10.0 if policy else 1e6, 1.0, 0.5)  # (a bandwidth above the threshold: every message stays UNCP)
    return c


@pytest.fixture(scope="module")
def ref():
    """The batch, the oracle's blobs with the policy on and off, and the batch with the big message."""
    rng = np.random.default_rng(20263)
    orc = Oracle()
    msgs = [rng.integers(1, 256, n, dtype=np.uint8) for n in LENGTHS]
    uncp = [orc.encode(m, bandwidth=1e6) for m in msgs]
    assert all(b[4:] == m.tobytes() and b[:4] == uncp[0][:4] for b, m in zip(uncp, msgs))  # marker + payload
    k = len(msgs) // 2
    mixed = msgs[:k] + [gradient(rng, BIG)] + msgs[k:]
    blobs = [orc.encode(m, bandwidth=10.0) for m in mixed]
    assert len(blobs[k]) != BIG + 4  # (the big one is transformed)
    return {"msgs": msgs, "uncp": uncp, "mixed": mixed, "blobs": blobs}


def canary_buffer(nbytes):
    t = torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t


def image(nbytes, places, parts):
    """What a canary-filled buffer holds once parts[i] lies at places[i]."""
    want = np.full(nbytes, CANARY, np.uint8)
    for p, b in zip(places, parts):
        want[p:p + len(b)] = np.frombuffer(bytes(b), np.uint8)
    return want


# ------------------------------------------------------------------ 1: UNCP passthrough, slotted
def test_passthrough_slotted(ref):
    """encode_into / decode_into with the policy off and a caller-built slot table: the 16-lane copy
    lists (tdt_encode_copy_kernel, tdt_decode_copy_kernel) with sources at the running offsets and
    destinations at every residue."""
    msgs, uncp = ref["msgs"], ref["uncp"]
    n = len(msgs)
    off = offsets([m.size for m in msgs])
    slots, end = phased_slots([len(b) for b in uncp], lead=0)
    assert {int(s + 4) % 16 for s in slots[:-1]} == ALL16 and {int(o) % 16 for o in off[:-1]} == ALL16
    codec = make_codec(policy=False)
    out = canary_buffer(end)
    _, _, ln, st = codec.encode_into(dev(np.concatenate(msgs)), dev(off), slots=dev(slots), out=out)
    torch.cuda.synchronize()
    assert int(st[:n].abs().sum()) == 0 and ln.cpu().numpy()[:n].tolist() == [len(b) for b in uncp]
    assert np.array_equal(out.cpu().numpy(), image(end, slots[:-1], uncp))
    # and back: the blobs back to back (payloads at the running offsets + 4), slots at every residue
    boff = offsets([len(b) for b in uncp])
    dslots, dend = phased_slots([m.size for m in msgs], lead=3)
    assert {int(s) % 16 for s in dslots[:-1]} == ALL16 and {int(o + 4) % 16 for o in boff[:-1]} == ALL16
    back = canary_buffer(dend)
    _, _, dl, ds = codec.decode_into(dev(np.frombuffer(b"".join(uncp), np.uint8)), dev(boff), slots=dev(dslots), out=back)
    torch.cuda.synchronize()
    assert int(ds[:n].abs().sum()) == 0 and dl.cpu().numpy()[:n].tolist() == [m.size for m in msgs]
    assert np.array_equal(back.cpu().numpy(), image(dend, dslots[:-1], msgs))
    assert codec.error_flags() == 0


# ------------------------------------------------------------------ 2: UNCP passthrough, scattered
def test_passthrough_scattered(ref):
    """encode_v / decode_v with the policy off: the pair-table instances of the copy lists, every
    message at a pointer of its own — source residue 7 i, destination residue 5 i (mod 16)."""
    msgs, uncp = ref["msgs"], ref["uncp"]
    n = len(msgs)
    codec = make_codec(policy=False)

    def run(call, srcs, outs, src_lead, out_lead):
        sp, send = phased_slots([len(s) for s in srcs], lead=src_lead, step=7)
        op, oend = phased_slots([len(o) for o in outs], lead=out_lead)
        src = dev(image(send, sp[:-1], srcs))
        out = canary_buffer(oend)
        assert src.data_ptr() % 16 == 0 and {int(a) % 16 for a in sp[:-1]} == ALL16 == {int(a) % 16 for a in op[:-1]}
        ln, st = call(i64(src.data_ptr() + a for a in sp[:-1]), i64(len(s) for s in srcs),
                      i64(out.data_ptr() + a for a in op[:-1]), i64(len(o) for o in outs))
        torch.cuda.synchronize()
        assert int(st[:n].abs().sum()) == 0 and ln.cpu().numpy()[:n].tolist() == [len(o) for o in outs]
        assert np.array_equal(out.cpu().numpy(), image(oend, op[:-1], outs))

    run(codec.encode_v, msgs, uncp, 0, 12)   # (the payload lands 4 bytes into the slot)
    run(codec.decode_v, uncp, msgs, 12, 0)   # (and is read 4 bytes into the blob)
    assert codec.error_flags() == 0


# ------------------------------------------------------------------ 3: two-phase compacted encode
@pytest.mark.parametrize("phase", [0, 9])
def test_two_phase_gather(ref, phase):
    """encode_batch with one message above 64 KiB: the slotted kernels, the scan, and cp_gather_kernel
    moving every blob from its slot to its compacted place — places of every residue by construction."""
    mixed, blobs = ref["mixed"], ref["blobs"]
    n = len(mixed)
    want_off = offsets([len(b) for b in blobs])
    total = int(want_off[-1])
    t = canary_buffer(64 + 16 + total + 64)
    out = t[64 + phase:64 + phase + total]
    assert {(out.data_ptr() + int(o)) % 16 for o in want_off[:-1]} == ALL16
    codec = make_codec()
    _, eoff, st = codec.encode_batch(dev(np.concatenate(mixed)), dev(offsets([m.size for m in mixed])), out=out)
    torch.cuda.synchronize()
    assert int(st[:n].abs().sum()) == 0 and eoff.cpu().numpy().tolist() == want_off.tolist()
    assert np.array_equal(t.cpu().numpy(), image(t.numel(), [64 + phase], [b"".join(blobs)]))
    assert codec.error_flags() == 0


# ------------------------------------------------------------------ 4: the host pipeline
class Pinned:
    """tdt_host_alloc memory, canary-filled."""

    def __init__(self, lib, nbytes):
        self.lib, self.p = lib, C.c_void_p()
        from psyne_amd._lib import check
        check(lib.tdt_host_alloc(nbytes, C.byref(self.p)))
        assert self.p.value % 16 == 0
        self.a = np.ctypeslib.as_array(C.cast(self.p, C.POINTER(C.c_uint8)), shape=(nbytes,))
        self.a[:] = CANARY

    def close(self):
        self.a = None
        self.lib.tdt_host_free(self.p)


def host_call(codec, fn, pinned, phase, data, off, cap):
    """tdt_encode_host / tdt_decode_host into `cap` bytes, `phase` bytes past a 16-byte boundary of a
    canary-filled pinned or pageable buffer: (the whole buffer, out offsets, statuses)."""
    from psyne_amd._lib import check
    nbytes = 64 + 16 + cap + 64
    pin = Pinned(codec._lib, nbytes) if pinned else None
    buf = pin.a if pinned else np.full(nbytes + 16, CANARY, np.uint8)
    base = 0 if pinned else (-buf.ctypes.data) % 16
    n = off.size - 1
    data, off = np.ascontiguousarray(data, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64)
    ooff, st = np.zeros(n + 1, np.uint64), np.zeros(n, np.int32)
    try:
        check(fn(codec._h, data.ctypes.data, off.ctypes.data, n, buf.ctypes.data + base + 64 + phase, cap,
                 ooff.ctypes.data, st.ctypes.data))
        return buf[base:base + nbytes].copy(), ooff, st
    finally:
        if pin:
            pin.close()


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_encode_slotted_chunk(ref, pinned):
    """One message above 64 KiB: the chunk is slotted and host_gather_kernel moves every blob to its
    compacted place in the caller's pinned buffer (or the staging)."""
    mixed, blobs = ref["mixed"], ref["blobs"]
    want_off = offsets([len(b) for b in blobs])
    cap = sum(encode_bound(m.size) for m in mixed)
    codec = make_codec()
    for phase in ([0, 5, 15] if pinned else [0]):  # (the staging is aligned whatever the caller's buffer)
        got, ooff, st = host_call(codec, codec._lib.tdt_encode_host, pinned, phase, np.concatenate(mixed),
                                  offsets([m.size for m in mixed]), cap)
        assert int(np.abs(st).sum()) == 0 and ooff.tolist() == want_off.tolist()
        assert np.array_equal(got, image(got.size, [64 + phase], [b"".join(blobs)])), "phase %d" % phase
    assert codec.error_flags() == 0


@pytest.fixture(scope="module")
def lookback(ref):
    """Batches the host encode takes in one pass (every message <= 64 KiB, 16 KiB or more on average), so
    that host_out_kernel copies the chunk's compacted output as one range: a 64 KiB message, then a
    short one — sixteen totals with different tails."""
    rng = np.random.default_rng(20264)
    orc = Oracle()
    g = gradient(rng, 65536)
    gb = orc.encode(g, bandwidth=10.0)
    shorts = [0, 1, 2, 3, 5, 7, 8, 11, 13, 15, 16, 17, 64, 255, 4096, 4097]
    out = []
    for n in shorts:
        m = rng.integers(1, 256, n, dtype=np.uint8) if n != 4096 else gradient(rng, n)
        out.append(([g, m], [gb, orc.encode(m, bandwidth=10.0)]))
    assert len({sum(len(b) for b in bl) % 16 for _, bl in out}) >= 8  # (tails of many lengths)
    return out


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_encode_below_lookback_limit(lookback, pinned):
    codec = make_codec()
    for phase, (msgs, blobs) in enumerate(lookback):
        want_off = offsets([len(b) for b in blobs])
        got, ooff, st = host_call(codec, codec._lib.tdt_encode_host, pinned, phase, np.concatenate(msgs),
                                  offsets([m.size for m in msgs]), sum(encode_bound(m.size) for m in msgs))
        assert int(np.abs(st).sum()) == 0 and ooff.tolist() == want_off.tolist()
        assert np.array_equal(got, image(got.size, [64 + phase], [b"".join(blobs)])), "phase %d" % phase
    assert codec.error_flags() == 0


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_decode(ref, lookback, pinned):
    """host_dout_kernel: a chunk's decoded output as one range into the caller's pinned buffer at every
    phase (or the staging) — the whole batch, and the sixteen two-message batches for their totals."""
    codec = make_codec()
    cases = [(0, ref["mixed"], ref["blobs"])] + [(p, m, b) for p, (m, b) in enumerate(lookback)]
    for phase, msgs, blobs in cases:
        want_off = offsets([m.size for m in msgs])
        got, ooff, st = host_call(codec, codec._lib.tdt_decode_host, pinned, phase, np.frombuffer(b"".join(blobs), np.uint8),
                                  offsets([len(b) for b in blobs]), int(want_off[-1]))
        assert int(np.abs(st).sum()) == 0 and ooff.tolist() == want_off.tolist()
        assert np.array_equal(got, image(got.size, [64 + phase], [np.concatenate(msgs)])), "phase %d, %d messages" % (phase, len(msgs))
    assert codec.error_flags() == 0


# ------------------------------------------------------------------ 5: pack_v
def test_pack_v_every_phase(ref):
    """The same blobs, each in a place of its own (residue 7 i), packed at output phases 0..15."""
    blobs = ref["uncp"]
    n = len(blobs)
    sp, send = phased_slots([len(b) for b in blobs], lead=0, step=7)
    sp = sp[:-1]
    src = dev(image(send, sp, blobs))
    assert src.data_ptr() % 16 == 0 and {int(a) % 16 for a in sp} == ALL16
    want_off = offsets([len(b) for b in blobs])
    total = int(want_off[-1])
    codec = make_codec()
    ptr, ln = i64(src.data_ptr() + a for a in sp), i64(len(b) for b in blobs)
    for phase in range(16):
        t = canary_buffer(64 + 16 + total + 64)
        off, st = codec.pack_v(ptr, ln, t[64 + phase:64 + phase + total])
        torch.cuda.synchronize()
        assert int(st[:n].abs().sum()) == 0 and off.cpu().numpy().tolist() == want_off.tolist()
        assert np.array_equal(t.cpu().numpy(), image(t.numel(), [64 + phase], [b"".join(blobs)])), "phase %d" % phase
    assert codec.error_flags() == 0
