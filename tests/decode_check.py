"""The checking half of the differential decode tests on the GPU, shared by the fuzz, edge and tiled
generic-width suites: a case with what the library must report, inputs packed at a byte phase with
0xFF behind them, outputs between 0xA5 guard bytes, and the comparison that collects every mismatch
by case name.  A test module imports it after its own `torch = pytest.importorskip("torch")` line."""
import numpy as np
import torch

GUARD, FILL, TAIL, GAP = 0xA5, 0xFF, 4096, 16


class Expect:
    """One case with what the library must report: status, decoded length, bytes."""

    def __init__(self, case, status, out):
        self.name, self.ws, self.family, self.blob = case
        self.status, self.out = status, out
        self.size = len(out)


def packed_input(exp, phase):
    """The blobs back to back `phase` bytes past a 64-byte boundary, TAIL bytes of 0xFF behind the
    last: (the device view that starts at the first blob, offsets as a device tensor, offsets)."""
    off = np.zeros(len(exp) + 1, np.int64)
    off[1:] = np.cumsum([len(e.blob) for e in exp])
    lead = 64 + phase
    buf = np.full(lead + int(off[-1]) + TAIL, FILL, np.uint8)
    buf[lead:lead + int(off[-1])] = np.frombuffer(b"".join(e.blob for e in exp), np.uint8)
    d = torch.from_numpy(buf).cuda()
    return d[lead:], torch.from_numpy(off).cuda(), off


def guarded_output(nbytes, phase):
    """`nbytes` of output `phase` bytes past a 64-byte boundary inside an allocation of 0xA5."""
    lead = 64 + phase
    t = torch.full((lead + nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    return t, t[lead:lead + nbytes], lead


def compare(exp, got_st, got_len, region, bad, tag, where=None):
    """region(i) → the bytes the route gave case i, GAP guard bytes behind them included.
    where(e, at) → optional words on where byte `at` of case e's output lies."""
    for i, e in enumerate(exp):
        if int(got_st[i]) != e.status:
            bad.append("%s %s: status %d, expected %d" % (tag, e.name, got_st[i], e.status))
            continue
        if got_len is not None and int(got_len[i]) != e.size:
            bad.append("%s %s: length %d, expected %d" % (tag, e.name, got_len[i], e.size))
            continue
        r = region(i)
        if r[: e.size].tobytes() != e.out:
            diff = np.flatnonzero(r[: e.size] != np.frombuffer(e.out, np.uint8))
            bad.append("%s %s: %d bytes differ, the first at %d%s" % (tag, e.name, diff.size, diff[0],
                                                                      " (%s)" % where(e, int(diff[0])) if where else ""))
        elif not (r[e.size:] == GUARD).all():
            bad.append("%s %s: wrote past its %d bytes" % (tag, e.name, e.size))


def run_slotted(codec, exp, in_phase, out_phase, tag, bad, where=None):
    n = len(exp)
    d, o, _ = packed_input(exp, in_phase)
    sizes = np.array([e.size for e in exp], np.int64)
    slots = np.zeros(n + 1, np.int64)
    slots[1:] = np.cumsum(sizes + GAP)  # caller-chosen: a write past a blob's bytes lands on guard bytes
    whole, out, lead = guarded_output(int(slots[-1]), out_phase)
    out, _, ln, st = codec.decode_into(d, o, slots=torch.from_numpy(slots).cuda(), out=out)
    torch.cuda.synchronize()
    h = whole.cpu().numpy()
    st, ln = st.cpu().numpy()[:n], ln.cpu().numpy()[:n]
    compare(exp, st, ln, lambda i: h[lead + slots[i]:lead + slots[i + 1]], bad, tag, where)
    if not ((h[:lead] == GUARD).all() and (h[lead + slots[-1]:] == GUARD).all()):
        bad.append("%s: wrote outside the output buffer" % tag)
    return h[lead:lead + slots[-1]].copy(), st, ln


def check_sizes(codec, exp, in_phase, bad):
    n = len(exp)
    d, o, _ = packed_input(exp, in_phase)
    want = np.array([e.size for e in exp], np.int64)
    want_st = np.array([e.status for e in exp], np.int32)
    sz, st = codec.decoded_sizes(d, o)
    dst = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    sl = codec.decode_slots(d, o, status=dst)
    torch.cuda.synchronize()
    sz, st, sl, dst = sz.cpu().numpy(), st.cpu().numpy(), sl.cpu().numpy(), dst.cpu().numpy()
    for i, e in enumerate(exp):
        if (sz[i], st[i], dst[i]) != (want[i], want_st[i], want_st[i]):
            bad.append("sizes %s: size %d status %d / %d, expected %d and %d" % (e.name, sz[i], st[i], dst[i], want[i],
                                                                               want_st[i]))
    if not np.array_equal(sl, np.concatenate([[0], np.cumsum(want)])):
        bad.append("decode_slots: not the prefix sum of the decoded sizes")
