"""Differential decode on the GPU at the decode kernels' own boundaries: the blobs of
tests/decode_edge_cases.py (a counted pair on, before and behind every lane, round, window,
generation, tile, one-blob tile, share, pair-lane, block and chunk edge; dense, 255-only and
count-0 streams; streams that end at every such edge) through every decode route of the C ABI,
status for status, length for length and byte for byte against the CPU oracle (pinned in
tests/golden/decode_edges.json, tests/test_decode_edges.py).  There is no tolerance.

As in tests/test_gpu_decode_fuzz.py, whose route helpers this module uses: outputs lie between 0xA5
guard bytes, inputs end with 4 KiB of 0xFF, and the codec's device invariant flags stay 0.  Each test
collects every mismatch and reports the first eight with the case's nearest deliberate edge.

Not covered: decode_fast's rebase of its held pair starts every 2^28 positions of one call
(PSY_DEC_REBASE_LOG2): it needs a blob that decodes to 256 MiB on the one-wave path."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import decode_edge_cases as ec
from tests.support import report

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, i64, make_codec  # noqa: E402, F401
from tests.decode_check import (Expect, FILL, GUARD, TAIL, check_sizes, compare, guarded_output,  # noqa: E402
                                packed_input, run_slotted)

pytestmark = pytest.mark.gpu


class EdgeExpect(Expect):
    def __init__(self, case, out):
        super().__init__(case[:4], 0, out)
        self.case = case
        self.path = ec.shape_of(case).path


def build_batch(cases):
    orc = Oracle()
    exp = []
    for c in cases:
        st, out = orc.decode(c.blob)
        assert st == 0, c.name
        exp.append(EdgeExpect(c, out))
    return exp


@pytest.fixture(scope="module")
def batch():
    return build_batch(ec.all_cases())  # (the oracle runs once for every route)


def where(e, at):
    return ec.locate(e.case, at)


# ------------------------------------------------------------------ a, b: slotted, two thresholds
def route_a(batch, bad, in_phases=(0, 1, 2, 3)):
    """Default thresholds; every byte phase of the input (load_block's shift), output phases 0 and 9."""
    codec = make_codec()
    for in_phase in in_phases:
        for out_phase in (0, 9):
            run_slotted(codec, batch, in_phase, out_phase, "slotted(%d,%d)" % (in_phase, out_phase), bad, where)
        check_sizes(codec, batch, in_phase, bad)
    assert codec.error_flags() == 0


def route_b(batch, bad):
    """TDT_OPT_LARGE_MIN = 16,384: the prep, block, scan and tile passes; the same bytes as route a."""
    from psyne_amd._lib import TDT_OPT_LARGE_MIN
    plain = make_codec()
    base, bst, bln = run_slotted(plain, batch, 0, 0, "slotted", bad, where)
    codec = make_codec()
    codec.set_option(TDT_OPT_LARGE_MIN, 16384)
    for in_phase, out_phase in ((0, 0), (5, 9)):
        got, st, ln = run_slotted(codec, batch, in_phase, out_phase, "large(%d,%d)" % (in_phase, out_phase), bad, where)
        if not (np.array_equal(got, base) and np.array_equal(st, bst) and np.array_equal(ln, bln)):
            bad.append("large(%d,%d): differs from the default threshold's result" % (in_phase, out_phase))
    assert codec.error_flags() == 0 and plain.error_flags() == 0


@pytest.mark.parametrize("in_phase", [0, 1, 2, 3])
def test_route_a_slotted(batch, in_phase):
    bad = []
    route_a(batch, bad, (in_phase,))
    report(bad)


def test_route_b_slotted_large_passes(batch):
    bad = []
    route_b(batch, bad)
    report(bad)


# ------------------------------------------------------------------ c: compacted
@pytest.mark.parametrize("path", ["two_phase", "lookback"])
def test_route_c_compacted(batch, path):
    from psyne_amd._lib import TDT_OPT_NO_TWO_PHASE
    bad = []
    n = len(batch)
    codec = make_codec()
    codec.set_option(TDT_OPT_NO_TWO_PHASE, 1 if path == "lookback" else 0)
    want_off = np.concatenate([[0], np.cumsum([e.size for e in batch])]).astype(np.int64)
    for in_phase, out_phase in ((0, 0), (3, 7)):
        d, o, _ = packed_input(batch, in_phase)
        whole, out, lead = guarded_output(int(want_off[-1]), out_phase)
        _, doff, st = codec.decode_batch(d, o, out=out)
        torch.cuda.synchronize()
        h, doff, st = whole.cpu().numpy(), doff.cpu().numpy(), st.cpu().numpy()[:n]
        tag = "%s(%d,%d)" % (path, in_phase, out_phase)
        if not np.array_equal(doff, want_off):
            k = int(np.flatnonzero(doff != want_off)[0])
            bad.append("%s: offsets differ from entry %d (%s)" % (tag, k, batch[max(k - 1, 0)].name))
            continue
        compare(batch, st, None, lambda i: h[lead + want_off[i]:lead + want_off[i + 1]], bad, tag, where)
        if not ((h[:lead] == GUARD).all() and (h[lead + want_off[-1]:] == GUARD).all()):
            bad.append("%s: wrote outside the output buffer" % tag)
    assert codec.error_flags() == 0
    report(bad)


# ------------------------------------------------------------------ d: scattered
@pytest.fixture(scope="module")
def scattered(batch):
    """Every blob in an allocation of its own at byte phase k % 4 (0xFF behind it), in shuffled order."""
    order = [int(i) for i in np.random.default_rng(4243).permutation(len(batch))]
    exp = [batch[i] for i in order]
    blobs = []
    for k, e in enumerate(exp):
        t = torch.full((k % 4 + len(e.blob) + TAIL,), FILL, dtype=torch.uint8, device="cuda")
        v = t[k % 4:k % 4 + len(e.blob)]
        v.copy_(torch.from_numpy(np.frombuffer(e.blob, np.uint8).copy()))
        blobs.append((t, v))
    return exp, blobs


@pytest.mark.parametrize("large_min", [0, 16384])
def test_route_d_scattered(scattered, large_min):
    """large_min 16,384: the PAIR instances of the large passes."""
    from psyne_amd._lib import TDT_OPT_LARGE_MIN
    exp, blobs = scattered
    bad = []
    codec = make_codec()
    if large_min:
        codec.set_option(TDT_OPT_LARGE_MIN, large_min)
    outs = [torch.full((64 + e.size + 64,), GUARD, dtype=torch.uint8, device="cuda") for e in exp]
    ln, st = codec.decode_v(i64(v.data_ptr() for _, v in blobs), i64(len(e.blob) for e in exp),
                            i64(t.data_ptr() + 64 for t in outs), i64(e.size for e in exp))
    torch.cuda.synchronize()
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    for i, e in enumerate(exp):
        h = outs[i].cpu().numpy()
        compare([e], st[i:i + 1], ln[i:i + 1], lambda _: h[64:], bad, "scattered", where)
        if not (h[:64] == GUARD).all():
            bad.append("scattered %s: wrote before its output" % e.name)
    assert codec.error_flags() == 0
    report(bad)


# ------------------------------------------------------------------ e, f: the host calls
def route_e(batch, bad):
    """tdt_decode_host with one blob per call: every tuned-width case up to kOneMax (the one-wave
    kernel up to 4 KiB, above it tdt_decode_one_kernel's tiles of TG groups: the `onetile` edges)."""
    from psyne_amd._lib import check
    codec = make_codec()
    lib, h = codec._lib, codec._h
    sub = [e for e in batch if e.path != "any" and e.size <= ec.geometry()["one_max"]]
    assert len(sub) >= 1000
    for e in sub:
        src = np.full(len(e.blob) + TAIL, FILL, np.uint8)
        src[: len(e.blob)] = np.frombuffer(e.blob, np.uint8)
        out = np.full(64 + e.size + 64, GUARD, np.uint8)
        off = np.array([0, len(e.blob)], np.uint64)
        ooff = np.zeros(2, np.uint64)
        st = np.full(1, -1, np.int32)
        check(lib.tdt_decode_host(h, src.ctypes.data, off.ctypes.data, 1, out.ctypes.data + 64, e.size, ooff.ctypes.data,
                                  st.ctypes.data))
        compare([e], st, [int(ooff[1])], lambda i: out[64:], bad, "host", where)
        if not (out[:64] == GUARD).all():
            bad.append("host %s: wrote before its output" % e.name)
    assert codec.error_flags() == 0


def test_route_e_host_one_blob_per_call(batch):
    bad = []
    route_e(batch, bad)
    report(bad)


def test_route_f_host_batch_generic_widths(batch):
    bad = []
    codec = make_codec()
    gen = [e for e in batch if e.path == "any"]
    assert len(gen) >= 300
    data = np.frombuffer(b"".join(e.blob for e in gen), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(e.blob) for e in gen])]).astype(np.uint64)
    want_off = np.concatenate([[0], np.cumsum([e.size for e in gen])]).astype(np.uint64)
    dec, doff, st = codec.decode_host(data, off, int(want_off[-1]))
    if not np.array_equal(doff, want_off):
        bad.append("host batch: output offsets differ")
    else:
        compare(gen, st, None, lambda i: dec[int(want_off[i]):int(want_off[i + 1])], bad, "host batch", where)
    assert codec.error_flags() == 0
    report(bad)
