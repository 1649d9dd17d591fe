"""The tiled generic-width decode on the GPU (psyne_amd/csrc/tdt_anyws.h: long blobs as 32 KiB output
tiles): every case of tests/anyws_dec_tiled_cases.py through every decode route, under
TDT_OPT_ANY_DEC_TILED = 1 (the tile pipeline) and = 0 (one workgroup per blob).  Every test requires
identical output, lengths and statuses under both values, equality with the CPU oracle, untouched
0xA5 guard bytes around every slot — and, through TdtCodec.stat(), that under option 1 the plan
claimed exactly the long blobs and tiles the numpy model counts, so that identical bytes are not a
quiet fall-back to the one-workgroup kernel.  There is no tolerance."""
import struct

import numpy as np
import pytest

from tests import anyws_dec_tiled_cases as tc
from tests import anyws_tiled_cases as enc_cases
from tests import decode_cases as dc
from tests.support import E_CAPACITY, report

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, canaries_intact, guarded, i64, orc  # noqa: E402, F401
from tests.decode_check import (Expect, FILL, GAP, GUARD, TAIL, compare, guarded_output, packed_input,  # noqa: E402
                                run_slotted)

pytestmark = pytest.mark.gpu

OPT_LARGE_MIN, OPT_TILE_CAP, OPT_NO_TWO_PHASE, OPT_ANY_DEC_TILED = 1, 2, 5, 9
TILE = tc.kernel_tile()
SWITCH = (1, 0)  # TDT_OPT_ANY_DEC_TILED: the tile pipeline, then the one-workgroup kernel


def make_codec(tiled, large_min=TILE, ws=4):
    from psyne_amd import TDTConfig, TdtCodec
    codec = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws))  # (blobs of generic widths: the deferred list)
    codec.set_metrics(10.0, 1.0, 0.5)
    codec.set_option(OPT_LARGE_MIN, large_min)
    codec.set_option(OPT_ANY_DEC_TILED, tiled)  # (a library without the option: TDT_E_ARG "unknown option")
    return codec


def expect_of(orc, name, ws, blob):
    st, out = orc.decode(blob)
    assert st == 0, name
    return Expect((name, ws, "tiled", blob), 0, out)


@pytest.fixture(scope="module")
def batch(orc):
    """Every case but the 2^32 one with the oracle's output (the oracle runs once for every route)."""
    return [expect_of(orc, c.name, c.ws, c.blob) for c in tc.all_cases()]


def is_long(e, thr=TILE):
    """The plan's rule for a blob that fits: a generic width, decoded size above the threshold, one or
    two referenced streams."""
    if e.blob[:4] != struct.pack("<I", dc.MAGIC_TDT):
        return False  # (a passthrough blob)
    orig, _, ws, _, mapping, _ = dc.parse(e.blob)
    return ws not in dc.TUNED and orig > thr and len(set(mapping)) <= 2


def tiles_of(e):
    return tc.ntiles_of(e.size, e.ws, TILE)


def check_stats(codec, exp, bad, tag, thr=TILE):
    torch.cuda.synchronize()
    long_ = [e for e in exp if is_long(e, thr)]
    got = (codec.stat("ANY_DEC_LARGE"), codec.stat("ANY_DEC_TILES"))
    want = (len(long_), sum(tiles_of(e) for e in long_))
    if got != want:
        bad.append("%s: the plan claimed %r long blobs and tiles, the model counts %r" % (tag, got, want))


# ------------------------------------------------------------------ routes
def test_slotted(batch):
    bad, res = [], []
    for tiled in SWITCH:
        codec = make_codec(tiled)
        res.append(run_slotted(codec, batch, 0, 0, "slotted[%d]" % tiled, bad))
        if tiled:
            check_stats(codec, batch, bad, "slotted")
            assert codec.stat("ANY_DEC_BLOCKS") > 0
        assert codec.error_flags() == 0
    assert all(np.array_equal(a, b) for a, b in zip(res[0], res[1]))
    report(bad)


def test_alignment_of_blob_and_slot(batch):
    """The input and the output buffer each at every offset 0..15 modulo 16, independently (the slots
    inside the buffer lie GAP guard bytes apart, so the tiles start at every alignment anyway)."""
    bad = []
    sub = batch[::11]
    codecs = [make_codec(t) for t in SWITCH]
    phases = [(p, (7 * p + 3) % 16) for p in range(16)]
    assert {a for a, _ in phases} == {b for _, b in phases} == set(range(16))
    for in_phase, out_phase in phases:
        res = [run_slotted(c, sub, in_phase, out_phase, "aligned(%d,%d)[%d]" % (in_phase, out_phase, t), bad)
               for c, t in zip(codecs, SWITCH)]
        assert all(np.array_equal(a, b) for a, b in zip(res[0], res[1]))
        check_stats(codecs[0], sub, bad, "aligned(%d,%d)" % (in_phase, out_phase))
    report(bad)


def run_scattered(codec, exp, caps, bad, tag):
    """decode_v in shuffled address order, every output between 64 guard bytes; caps[i] < size: one byte short."""
    order = [int(i) for i in np.random.default_rng(4244).permutation(len(exp))]
    blobs = {}
    for k in order:  # (allocation order = shuffled: the pointer table is in no address order)
        e = exp[k]
        t = torch.full((k % 16 + len(e.blob) + TAIL,), FILL, dtype=torch.uint8, device="cuda")
        v = t[k % 16:k % 16 + len(e.blob)]
        v.copy_(torch.from_numpy(np.frombuffer(e.blob, np.uint8).copy()))
        blobs[k] = (t, v)
    outs = [guarded(c) for c in caps]
    ln, st = codec.decode_v(i64(blobs[k][1].data_ptr() for k in range(len(exp))), i64(len(e.blob) for e in exp),
                            i64(v.data_ptr() for _, v in outs), i64(caps))
    torch.cuda.synchronize()
    ln, st = ln.cpu().numpy()[:len(exp)], st.cpu().numpy()[:len(exp)]
    got = []
    for i, e in enumerate(exp):
        t, v = outs[i]
        if not canaries_intact(t, caps[i]):
            bad.append("%s %s: wrote outside its output" % (tag, e.name))
        h = v.cpu().numpy()
        if caps[i] < e.size:
            if (st[i], ln[i]) != (E_CAPACITY, 0) or not (h == 0xA5).all():
                bad.append("%s %s: one byte short gave status %d, length %d" % (tag, e.name, st[i], ln[i]))
        else:
            compare([e], st[i:i + 1], ln[i:i + 1], lambda _: h, bad, tag)
        got.append(h.tobytes())
    return got, ln, st


def test_scattered_shuffled(batch):
    bad, res = [], []
    for tiled in SWITCH:
        codec = make_codec(tiled)
        res.append(run_scattered(codec, batch, [e.size for e in batch], bad, "scattered[%d]" % tiled))
        if tiled:
            check_stats(codec, batch, bad, "scattered")
        assert codec.error_flags() == 0
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    report(bad)


def run_compacted(codec, exp, cap_short, bad, tag):
    n = len(exp)
    want_off = np.concatenate([[0], np.cumsum([e.size for e in exp])]).astype(np.int64)
    d, o, _ = packed_input(exp, 3)
    whole, out, lead = guarded_output(int(want_off[-1]) - cap_short, 7)
    _, doff, st = codec.decode_batch(d, o, out=out)
    torch.cuda.synchronize()
    h, doff, st = whole.cpu().numpy(), doff.cpu().numpy(), st.cpu().numpy()[:n]
    if not ((h[:lead] == GUARD).all() and (h[lead + out.numel():] == GUARD).all()):
        bad.append("%s: wrote outside the output buffer" % tag)
    return h[lead:lead + out.numel()].copy(), doff, st, want_off


@pytest.mark.parametrize("path", ["lookback", "two_phase"])
def test_compacted(batch, path):
    """decode_batch: the compacted look-back route (the plan reads out_off and out_cap), and the two phases."""
    bad, res = [], []
    sub = batch[::3]
    for tiled in SWITCH:
        codec = make_codec(tiled)
        codec.set_option(OPT_NO_TWO_PHASE, 1 if path == "lookback" else 0)
        h, doff, st, want_off = run_compacted(codec, sub, 0, bad, "%s[%d]" % (path, tiled))
        assert np.array_equal(doff, want_off)
        compare(sub, st, None, lambda i: np.concatenate([h[want_off[i]:want_off[i + 1]], np.full(1, GUARD, np.uint8)]), bad, path)
        if tiled:
            check_stats(codec, sub, bad, path)
        res.append((h, doff, st))
        assert codec.error_flags() == 0
    assert all(np.array_equal(a, b) for a, b in zip(res[0], res[1]))
    report(bad)


def test_counts_past_2_32(orc):
    """One stream whose counts sum past 2^32 (the clamped prefix): against the oracle only."""
    c = tc.all_cases(with_big=True)[-1]
    assert c.oracle_only
    exp = [expect_of(orc, c.name, c.ws, c.blob)]
    bad, res = [], []
    for tiled in SWITCH:
        codec = make_codec(tiled)
        res.append(run_slotted(codec, exp, 0, 5, "past_2_32[%d]" % tiled, bad))
        if tiled:
            check_stats(codec, exp, bad, "past_2_32")
    assert all(np.array_equal(a, b) for a, b in zip(res[0], res[1]))
    report(bad)


# ------------------------------------------------------------------ round trip, other entry points
def test_round_trip_with_the_tiled_encode():
    from psyne_amd import TDTConfig, TdtCodec
    bad = []
    for ws, mk in ((12, "interleaved"), (3, "low"), (40, "high")):
        msgs = [m for _, m in enc_cases.cases_for(ws, mk, enc_cases.kernel_tile())]
        off = np.concatenate([[0], np.cumsum([m.size for m in msgs])]).astype(np.int64)
        data, o = torch.from_numpy(np.concatenate(msgs)).cuda(), torch.from_numpy(off).cuda()
        res = []
        for tiled in SWITCH:
            codec = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws))
            codec.set_metrics(10.0, 1.0, 0.5)
            codec.set_option(OPT_LARGE_MIN, TILE)
            codec.set_option(OPT_ANY_DEC_TILED, tiled)
            enc, slots, lens, st = codec.encode_into(data, o)
            torch.cuda.synchronize()
            assert int(st.abs().sum()) == 0
            sizes = np.array([m.size for m in msgs], np.int64)
            dslots = np.concatenate([[0], np.cumsum(sizes + GAP)]).astype(np.int64)
            whole, out, lead = guarded_output(int(dslots[-1]), 5)
            _, _, dl, dst = codec.decode_into(enc, slots, in_lengths=lens, slots=torch.from_numpy(dslots).cuda(), out=out)
            torch.cuda.synchronize()
            h = whole.cpu().numpy()
            for i, m in enumerate(msgs):
                r = h[lead + dslots[i]:lead + dslots[i + 1]]
                if int(dst[i]) != 0 or int(dl[i]) != m.size or not np.array_equal(r[:m.size], m) or not (r[m.size:] == GUARD).all():
                    bad.append("round trip ws %d message %d [%d]" % (ws, i, tiled))
            if tiled:
                torch.cuda.synchronize()
                if codec.stat("ANY_DEC_LARGE") != len(msgs):
                    bad.append("round trip ws %d: %d of %d blobs tiled" % (ws, codec.stat("ANY_DEC_LARGE"), len(msgs)))
            res.append(h)
            assert codec.error_flags() == 0
        assert np.array_equal(res[0], res[1])
    report(bad)


def test_other_entry_points(batch):
    """decode_tensors, decode_host and the one-message decode() on long width-12 blobs: the same bytes;
    the host pipeline is untiled, so its calls leave the claims unchanged."""
    bad = []
    sub = [e for e in batch if e.ws == 12][:4]
    res = []
    for tiled in SWITCH:
        codec = make_codec(tiled)
        d, o, off = packed_input(sub, 0)
        outs = [guarded(e.size) for e in sub]
        ln, st = codec.decode_tensors(d, o[:-1], i64(len(e.blob) for e in sub), [v for _, v in outs])
        torch.cuda.synchronize()
        ln, st = ln.cpu().numpy(), st.cpu().numpy()
        for i, e in enumerate(sub):
            compare([e], st[i:i + 1], ln[i:i + 1], lambda _: outs[i][1].cpu().numpy(), bad, "tensors[%d]" % tiled)
            if not canaries_intact(outs[i][0], e.size):
                bad.append("tensors[%d] %s: wrote outside its tensor" % (tiled, e.name))
        if tiled:
            check_stats(codec, sub, bad, "tensors")
        before = (codec.stat("ANY_DEC_LARGE"), codec.stat("ANY_DEC_TILES"))
        data = np.frombuffer(b"".join(e.blob for e in sub), np.uint8)
        want_off = np.concatenate([[0], np.cumsum([e.size for e in sub])]).astype(np.uint64)
        dec, doff, hst = codec.decode_host(data, off.astype(np.uint64), int(want_off[-1]))
        assert np.array_equal(doff, want_off)
        compare(sub, hst, None, lambda i: np.concatenate([dec[int(want_off[i]):int(want_off[i + 1])], np.full(1, GUARD, np.uint8)]),
                bad, "host[%d]" % tiled)
        from psyne_amd.tdt import TDTCompressionProtocol
        proto = TDTCompressionProtocol()  # the one-message decode(): tdt_decode_host with one blob
        proto.codec.set_option(OPT_LARGE_MIN, TILE)
        proto.codec.set_option(OPT_ANY_DEC_TILED, tiled)
        one = bytes(proto.decode(sub[0].blob))
        if one != sub[0].out:
            bad.append("decode()[%d]: bytes differ" % tiled)
        torch.cuda.synchronize()
        if (codec.stat("ANY_DEC_LARGE"), codec.stat("ANY_DEC_TILES")) != before:
            bad.append("the host calls changed the claims")
        res.append((dec.tobytes(), one))
        assert codec.error_flags() == 0
    assert res[0] == res[1]
    report(bad)


# ------------------------------------------------------------------ mixed batches
def uncp_blob(payload: bytes) -> bytes:
    return struct.pack("<I", 0x554E4350) + payload


def test_mixed_batch(orc, batch):
    """Long and short blobs of widths 12, 3 and 4 and a passthrough blob in one call: both tile
    pipelines run.  Then, with enough small blobs that 1/4096 of the batch's bytes exceeds
    TDT_OPT_LARGE_MIN, the long blobs are those the share rule names."""
    rng = np.random.default_rng(77)
    bad = []
    mixed = [next(e for e in batch if e.ws == 12), next(e for e in batch if e.ws == 3)]
    mixed += [expect_of(orc, "short12", 12, dc.craft(rng, 3000, 12, "exact", 2, 0, 3, False)),
              expect_of(orc, "short3", 3, dc.craft(rng, 3000, 3, "long", 2, 1, 255, False)),
              expect_of(orc, "long4", 4, dc.craft(rng, 100000, 4, "exact", 2, 0, 3, False, mapping=[0, 0, 1, 1])),
              expect_of(orc, "short4", 4, dc.craft(rng, 3000, 4, "exact", 2, 0, 3, False, mapping=[0, 1, 1, 1])),
              expect_of(orc, "uncp", 4, uncp_blob(bytes(rng.integers(0, 256, 5000, dtype=np.uint8))))]
    res = []
    for tiled in SWITCH:
        codec = make_codec(tiled)
        res.append(run_slotted(codec, mixed, 1, 9, "mixed[%d]" % tiled, bad))
        if tiled:
            check_stats(codec, mixed, bad, "mixed")
            assert codec.stat("ANY_DEC_LARGE") == 2
        assert codec.error_flags() == 0
    assert all(np.array_equal(a, b) for a, b in zip(res[0], res[1]))
    # ---- the share rule
    large_min = 2048
    small = [expect_of(orc, "small%d" % i, (12, 3, 5)[i % 3], dc.craft(rng, 2300 + 40 * i, (12, 3, 5)[i % 3], "exact", 2, 0, 1, False))
             for i in range(20)]
    # as many copies of the small blobs as put 1/4096 of the batch's bytes in the middle of their sizes (2,300 .. 3,060)
    reps = -(-(2680 * 4096 - sum(len(e.blob) for e in batch[::2])) // sum(len(e.blob) for e in small))
    many = batch[::2] + small * reps
    total = sum(len(e.blob) for e in many)
    thr = max(large_min, total // 4096)
    assert thr > large_min and any(large_min < e.size <= thr for e in small) and any(e.size > thr for e in small)
    res = []
    for tiled in SWITCH:
        codec = make_codec(tiled, large_min=large_min)
        res.append(run_slotted(codec, many, 0, 0, "share[%d]" % tiled, bad))
        if tiled:
            check_stats(codec, many, bad, "share", thr)
        assert codec.error_flags() == 0
    assert all(np.array_equal(a, b) for a, b in zip(res[0], res[1]))
    report(bad)


def test_plan_starts_with_the_first_generic_blob(orc, batch):
    """A context that has decoded tuned widths only launches no plan; the call that first lists a generic
    blob runs on the old kernel, and from then on every call is planned — a tuned-only call in between
    does not switch the plan off again.  The bytes are the oracle's every time."""
    rng = np.random.default_rng(99)
    bad = []
    tuned = [expect_of(orc, "t%d" % i, 4, dc.craft(rng, 20000, 4, "exact", 2, 0, 3, False, mapping=[0, 0, 1, 1])) for i in range(3)]
    generic = [e for e in batch if e.ws == 12][:3]
    codec = make_codec(1)
    for _ in range(2):
        run_slotted(codec, tuned, 0, 0, "tuned", bad)
    run_slotted(codec, generic, 0, 0, "first generic", bad)
    torch.cuda.synchronize()
    assert codec.stat("ANY_DEC_LARGE") == 0  # (no plan ran yet)
    run_slotted(codec, tuned, 0, 0, "tuned again", bad)
    run_slotted(codec, generic, 0, 0, "second generic", bad)
    check_stats(codec, generic, bad, "second generic")
    report(bad)


# ------------------------------------------------------------------ capacity, budgets
def test_capacity_one_byte_short(batch):
    """A slot (decode_v) or out_cap (decode_batch) one byte short: TDT_E_CAPACITY, length 0, nothing
    written; the neighbours decode."""
    bad = []
    sub = batch[:6]
    for tiled in SWITCH:
        codec = make_codec(tiled)
        caps = [e.size - (1 if i in (1, 4) else 0) for i, e in enumerate(sub)]
        run_scattered(codec, sub, caps, bad, "short slot[%d]" % tiled)
        if tiled:
            torch.cuda.synchronize()
            assert codec.stat("ANY_DEC_LARGE") == 4  # (the plan leaves a blob that does not fit to the old kernel)
        codec = make_codec(tiled)
        codec.set_option(OPT_NO_TWO_PHASE, 1)
        h, doff, st, want_off = run_compacted(codec, sub, 1, bad, "short out_cap[%d]" % tiled)
        if st.tolist() != [0] * 5 + [E_CAPACITY]:
            bad.append("short out_cap[%d]: statuses %r" % (tiled, st.tolist()))
        compare(sub[:5], st, None, lambda i: np.concatenate([h[want_off[i]:want_off[i + 1]], np.full(1, GUARD, np.uint8)]), bad,
                "short out_cap[%d]" % tiled)
        if not (h[want_off[5]:] == GUARD).all():
            bad.append("short out_cap[%d]: the blob that does not fit was written" % tiled)
    report(bad)


def test_tile_cap_falls_back(batch):
    """TDT_OPT_TILE_CAP = 3: blobs that find no tiles fall back to one workgroup; the claims count past the cap."""
    bad, res = [], []
    sub = batch[:8]
    for tiled in SWITCH:
        codec = make_codec(tiled)
        codec.set_option(OPT_TILE_CAP, 3)
        res.append(run_slotted(codec, sub, 0, 0, "cap3[%d]" % tiled, bad))
        if tiled:
            check_stats(codec, sub, bad, "cap3")
            assert codec.stat("ANY_DEC_TILES") > 3
    assert all(np.array_equal(a, b) for a, b in zip(res[0], res[1]))
    report(bad)


def test_budget_grows_from_the_claims(orc):
    """65 long blobs of two tiles each on a cold context: the first call decodes all of them with a
    budget of 64 records (one on the old kernel), the second call's budget has grown."""
    rng = np.random.default_rng(65)
    blobs = [dc.craft(rng, 40000 + 12 * i, 12, "exact", 2, 0, 3, False) for i in range(5)]
    exp = [expect_of(orc, "b%d" % i, 12, blobs[i % 5]) for i in range(65)]
    assert all(tiles_of(e) == 2 for e in exp)
    bad = []
    codec = make_codec(1)
    first = run_slotted(codec, exp, 0, 0, "cold", bad)
    torch.cuda.synchronize()
    assert (codec.stat("ANY_DEC_LARGE"), codec.stat("ANY_DEC_TILES"), codec.stat("ANY_DEC_BUDGET_LARGE")) == (65, 130, 64)
    second = run_slotted(codec, exp, 0, 0, "warm", bad)
    torch.cuda.synchronize()
    assert codec.stat("ANY_DEC_BUDGET_LARGE") > 64 and codec.stat("ANY_DEC_LARGE") == 65
    plain = run_slotted(make_codec(0), exp, 0, 0, "plain", bad)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(first, second, plain))
    report(bad)


# ------------------------------------------------------------------ capture
def captured_decode(codec, exp, eager_calls):
    n = len(exp)
    d, o, _ = packed_input(exp, 0)
    slots = np.concatenate([[0], np.cumsum([e.size + GAP for e in exp])]).astype(np.int64)
    whole, out, lead = guarded_output(int(slots[-1]), 0)
    sl = torch.from_numpy(slots).cuda()
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    for _ in range(eager_calls):
        codec.decode_into(d, o, slots=sl, out=out, lengths=lens, status=st)
        torch.cuda.synchronize()
    whole.fill_(GUARD)
    lens.zero_()
    st.fill_(-1)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        codec.decode_into(d, o, slots=sl, out=out, lengths=lens, status=st)  # (raises unless TDT_OK)
    gr.replay()
    torch.cuda.synchronize()
    h = whole.cpu().numpy()
    bad = []
    compare(exp, st.cpu().numpy(), lens.cpu().numpy(), lambda i: h[lead + slots[i]:lead + slots[i + 1]], bad, "captured")
    del gr
    return h, bad


def test_captured_call_replays(batch):
    """Two eager calls on a warm context, then the call captured and replayed: the eager bytes."""
    sub = [e for e in batch if e.ws in (12, 64)][:6]
    res = []
    for tiled in SWITCH:
        codec = make_codec(tiled)
        h, bad = captured_decode(codec, sub, 2)
        report(bad)
        res.append(h)
        assert codec.error_flags() == 0
    assert np.array_equal(res[0], res[1])


def test_captured_call_without_a_budget(batch):
    """Warmed with a threshold no blob exceeds (so the history knows no long blob and the capture gets
    no tile budget), then captured with the long-blob threshold: TDT_OK and the right bytes."""
    sub = [e for e in batch if e.ws in (5, 40)][:6]
    codec = make_codec(1, large_min=1 << 30)
    d, o, _ = packed_input(sub, 0)
    for _ in range(2):
        codec.decode_into(d, o)
        torch.cuda.synchronize()
    assert codec.stat("ANY_DEC_LARGE") == 0
    codec.set_option(OPT_LARGE_MIN, TILE)
    h, bad = captured_decode(codec, sub, 0)
    report(bad)
    assert codec.error_flags() == 0
