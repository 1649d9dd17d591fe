"""Known mappings on the GPU: tdt_mappings_v (every message's mapping as one word, beside its exact
size), tdt_encode_mapped_v / _vp (the scattered, mixed-width and packed encodes with a caller mapping
per message) and TDT_OPT_PACK_SIZES_FIRST = 2 (the sizes-first packed encode reusing the mappings its
own size pass decided).  Expected bytes are the CPU oracle's (Oracle.encode(mapping=...)), the pinned
digests of tests/golden/encode_runs.json, or what the existing routes give; there is no tolerance.
Outputs lie between 0xA5 guard bytes that must stay intact, and the codec's device invariant flags
must stay 0."""
import json

import numpy as np
import pytest

from oracle.oracle import encode_bound
from tests import encode_run_cases as ec
from tests import mapping_band_cases as mb
from tests.golden_cases import GOLDEN
from tests.support import (CANARY, E_ARG, E_BAD_MAPPING, E_CAPACITY, E_CAPTURE, E_CONFIG, E_UNSUPPORTED, address_order,
                           bits_of, digest, mask_of)

torch = pytest.importorskip("torch")
from tests.gpu_support import (_gpu, canaries_intact, guarded, i32, i64, make_codec, orc, own,  # noqa: E402, F401
                               packed_blobs, ptrs, u64)
from tests.mixed_ws_cases import WIDTHS, batch, oracle_blob, records, run_vw  # noqa: E402, F401

pytestmark = pytest.mark.gpu

OPT_LARGE_MIN, OPT_TILE_CAP, OPT_PACK_SIZES_FIRST = 1, 2, 7
KINDS = ("analysed", "complement", "zeros", "ones", "random")


def compresses(n, ws):
    """should_transform under the tests' metrics and compress_tdt's size guard: not the UNCP route."""
    return n >= 1024 and n % 4 == 0 and n % ws == 0


def mapped_blob(orc, m, w, mapping):
    return orc.encode(m, cfg=orc.config(sample_fraction=1.0, word_size=w), mapping=[int(x) for x in mapping])


@pytest.fixture(scope="module")
def mapped(batch, orc):
    """Five mappings per message of the SIZES x WIDTHS batch and the oracle's blob under each (a
    message on the UNCP route keeps its ordinary blob: its mapping is ignored)."""
    rng = np.random.default_rng(20262)
    maps = {k: [] for k in KINDS}
    blobs = {k: [] for k in KINDS}
    for m, w, plain in zip(batch["msgs"], batch["ws"], batch["blobs"]):
        live = compresses(len(m), w)
        an = [int(x) for x in orc.analyze(m, w)[2]] if live else [0] * w
        five = dict(analysed=an, complement=[1 - x for x in an], zeros=[0] * w, ones=[1] * w,
                    random=[int(x) for x in rng.integers(0, 2, w)])
        for k in KINDS:
            maps[k].append(five[k])
            blobs[k].append(mapped_blob(orc, m, w, five[k]) if live else plain)
    assert blobs["analysed"] == batch["blobs"]
    return dict(maps=maps, blobs=blobs, runs={})


def run_mapped(batch, mapped, kind, order):
    """One mixed-width encode_vw(mapbits=...) call over the whole batch, every output between guards."""
    key = (kind, order)
    if key not in mapped["runs"]:
        idx = address_order(batch["tensors"], order)
        tensors = [batch["tensors"][i] for i in idx]
        caps = [batch["caps"][i] for i in idx]
        outs = [guarded(c) for c in caps]
        codec = make_codec(4)
        ln, st = codec.encode_vw(ptrs(tensors), i64(t.numel() for t in tensors), i32(batch["ws"][i] for i in idx),
                                 mask_of(WIDTHS), ptrs([v for _, v in outs]), i64(caps),
                                 mapbits=u64(bits_of(mapped["maps"][kind][i]) for i in idx))
        torch.cuda.synchronize()
        mapped["runs"][key] = (idx, outs, caps, ln.cpu().numpy(), st.cpu().numpy(), codec.error_flags())
    return mapped["runs"][key]


# ------------------------------------------------------------------------------- 1: every class, width, mapping
@pytest.mark.parametrize("order", ["ascending", "shuffled"])
def test_mapped_vw_every_class_every_width_five_mappings(batch, mapped, order):
    for kind in KINDS:
        idx, outs, caps, ln, st, flags = run_mapped(batch, mapped, kind, order)
        for k, i in enumerate(idx):
            what = "%s mapping, message %d (width %d, %d bytes)" % (kind, i, batch["ws"][i], len(batch["msgs"][i]))
            want = mapped["blobs"][kind][i]
            h = outs[k][0].cpu().numpy()
            assert st[k] == 0 and ln[k] == len(want), what
            assert h[64:64 + len(want)].tobytes() == want, what
            assert (h[:64] == CANARY).all() and (h[64 + len(want):] == CANARY).all(), what
        assert flags == 0


def test_decode_v_restores_complement_mapping_blobs(batch, mapped):
    idx, outs, caps, ln, st, _ = run_mapped(batch, mapped, "complement", "ascending")
    sizes = [len(batch["msgs"][i]) for i in idx]
    back = [torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda") for n in sizes]
    codec = make_codec(4)
    dl, ds = codec.decode_v(ptrs([v for _, v in outs]), i64(ln[: len(idx)]), ptrs(back), i64(sizes))
    torch.cuda.synchronize()
    assert int(ds.abs().sum()) == 0 and dl.cpu().numpy().tolist() == sizes
    for k, i in enumerate(idx):
        assert np.array_equal(back[k].cpu().numpy()[: sizes[k]], batch["msgs"][i]), "message %d" % i
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 2: the existing mapped route
@pytest.mark.parametrize("w", [4, 2, 16, 12])
def test_agrees_with_encode_with_mapping_batch(batch, mapped, w):
    """The width's sub-batch on a context of that width (no word sizes) against encode_batch(mapping=...)
    over the same messages laid back to back."""
    idx = [i for i, x in enumerate(batch["ws"]) if x == w]
    n = len(idx)
    for kind in ("random", "complement"):
        maps = [mapped["maps"][kind][i] for i in idx]
        codec = make_codec(w)
        data = np.concatenate([batch["msgs"][i] for i in idx])
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(batch["msgs"][i]) for i in idx])
        mp = torch.from_numpy(np.concatenate(maps).astype(np.int32)).cuda()
        enc, eoff, est = codec.encode_batch(torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda(), mapping=mp)
        tensors, caps = [batch["tensors"][i] for i in idx], [batch["caps"][i] for i in idx]
        outs = [guarded(c) for c in caps]
        ln, st = codec.encode_v(ptrs(tensors), i64(t.numel() for t in tensors), ptrs([v for _, v in outs]), i64(caps),
                                mapbits=u64(bits_of(m) for m in maps))
        torch.cuda.synchronize()
        enc, eoff, est = enc.cpu().numpy(), eoff.cpu().numpy(), est.cpu().numpy()
        ln, st = ln.cpu().numpy(), st.cpu().numpy()
        for k, i in enumerate(idx):
            what = "%s mapping, message %d (width %d)" % (kind, i, w)
            ref = enc[eoff[k]:eoff[k + 1]].tobytes()
            assert (int(st[k]), int(ln[k])) == (int(est[k]), len(ref)) and st[k] == 0, what
            assert outs[k][1][: ln[k]].cpu().numpy().tobytes() == ref == mapped["blobs"][kind][i], what
            assert canaries_intact(outs[k][0], caps[k]), what
        assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 3: the mapping's round trip
def test_mappings_v_round_trip(batch, mapped):
    idx, vw_outs, vw_ln, vw_st, _ = run_vw(batch, "ascending")
    tensors = [batch["tensors"][i] for i in idx]
    n = len(idx)
    codec = make_codec(4)
    args = (ptrs(tensors), i64(t.numel() for t in tensors))
    kw = dict(word_sizes=i32(batch["ws"][i] for i in idx), width_mask=mask_of(WIDTHS))
    es, est = codec.encoded_sizes_v(*args, **kw)
    ms, bits, mst = codec.mappings_v(*args, **kw)
    caps = [batch["caps"][i] for i in idx]
    outs = [guarded(c) for c in caps]
    ln, st = codec.encode_vw(*args, kw["word_sizes"], kw["width_mask"], ptrs([v for _, v in outs]), i64(caps), mapbits=bits)
    torch.cuda.synchronize()
    assert torch.equal(es[:n], ms[:n]) and torch.equal(est[:n], mst[:n]) and int(mst.abs().sum()) == 0
    assert ms.cpu().numpy()[:n].tolist() == [len(batch["blobs"][i]) for i in idx]
    want_bits = [bits_of(mapped["maps"]["analysed"][i]) if compresses(len(batch["msgs"][i]), batch["ws"][i]) else 0
                 for i in idx]
    assert bits.cpu().numpy().view(np.uint64)[:n].tolist() == want_bits
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    assert st[:n].tolist() == vw_st[:n].tolist() == [0] * n and ln[:n].tolist() == vw_ln[:n].tolist()
    for k in range(n):
        got = outs[k][1][: ln[k]].cpu().numpy().tobytes()
        assert got == vw_outs[k][: vw_ln[k]].cpu().numpy().tobytes() == batch["blobs"][idx[k]], "message %d" % idx[k]
        assert canaries_intact(outs[k][0], caps[k])
    assert codec.error_flags() == 0


@pytest.fixture(scope="module")
def bands(orc):
    """The mapping-band fixtures (near ties on both sides of the fast margin, and the exact ties) at
    each width's three smallest sizes, with the oracle's mapping and blob."""
    cases = [c for c in mb.load_cases() if c["ws"] in WIDTHS and c["size"] in mb.sizes_for(c["ws"])[:3]]
    assert len({c["ws"] for c in cases}) == len(WIDTHS)
    assert {c.get("sign") for c in cases if c["kind"] != "tie"} >= {"+", "-"}
    for c in cases:
        c["mapping"] = [int(x) for x in orc.analyze(c["input"], c["ws"])[2]]
        c["blob"] = oracle_blob(orc, c["input"], c["ws"])
        assert c["size"] >= 1024 and c["blob"][:4] == b"DTDT"
    return cases


def test_mappings_v_on_the_near_ties(bands):
    n = len(bands)
    tensors = [own(c["input"]) for c in bands]
    caps = [encode_bound(c["size"], c["ws"]) for c in bands]
    outs = [torch.zeros(x, dtype=torch.uint8, device="cuda") for x in caps]
    codec = make_codec(4)
    args = (ptrs(tensors), i64(c["size"] for c in bands))
    ws, mask = i32(c["ws"] for c in bands), mask_of(WIDTHS)
    sz, bits, st = codec.mappings_v(*args, word_sizes=ws, width_mask=mask)
    ln, est = codec.encode_vw(*args, ws, mask, ptrs(outs), i64(caps), mapbits=bits)
    torch.cuda.synchronize()
    sz, bits, ln = sz.cpu().numpy(), bits.cpu().numpy().view(np.uint64), ln.cpu().numpy()
    assert int(st.abs().sum()) == 0 and int(est.abs().sum()) == 0
    for k, c in enumerate(bands):
        assert int(bits[k]) == bits_of(c["mapping"]), c["name"]
        assert sz[k] == ln[k] == len(c["blob"]), c["name"]
        got = outs[k][: ln[k]].cpu().numpy().tobytes()
        assert np.frombuffer(got, np.int32, c["ws"], 20).tolist() == c["mapping"], c["name"]
        assert got == c["blob"], c["name"]
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 4: run arithmetic under a given mapping


@pytest.fixture(scope="module")
def runs():
    """The run-structured cases with their pinned blob digests (read, not rewritten), each message in
    a device allocation of its own, 0..3 bytes into it."""
    meta = json.loads((GOLDEN / "encode_runs.json").read_text())
    want = {r["name"]: r["blob"] for r in meta["cases"]}
    cases = [c for c in ec.all_cases() if c.name not in meta["dropped"]]
    assert len(cases) == len(want)
    dev = []
    for k, c in enumerate(cases):
        t = torch.full((k % 4 + c.n + 16,), 0xFF, dtype=torch.uint8, device="cuda")
        v = t[k % 4:k % 4 + c.n]
        v.copy_(torch.from_numpy(c.message.copy()))
        dev.append(v)
    return dict(cases=cases, want=want, dev=dev)


VW_WIDTHS = (1, 2, 4, 8, 16, 3, 12)


def test_run_cases_mapped_scattered(runs):
    """Every case with its intended mapping: one mixed-width call over the widths a call takes, and
    width 40 on a context of its own."""
    bad = []
    for widths in (VW_WIDTHS, (40,)):
        sel = [k for k, c in enumerate(runs["cases"]) if c.ws in widths]
        cs = [runs["cases"][k] for k in sel]
        caps = [encode_bound(c.n, c.ws) for c in cs]
        outs = [torch.zeros(x, dtype=torch.uint8, device="cuda") for x in caps]
        args = (i64(runs["dev"][k].data_ptr() for k in sel), i64(c.n for c in cs))
        bits = u64(bits_of(c.mapping) for c in cs)
        if len(widths) > 1:
            codec = make_codec(4)
            ln, st = codec.encode_vw(*args, i32(c.ws for c in cs), mask_of(widths), ptrs(outs), i64(caps), mapbits=bits)
        else:
            codec = make_codec(widths[0])
            ln, st = codec.encode_v(*args, ptrs(outs), i64(caps), mapbits=bits)
        torch.cuda.synchronize()
        ln, st = ln.cpu().numpy(), st.cpu().numpy()
        for k, c in enumerate(cs):
            if st[k] != 0 or digest(outs[k][: ln[k]].cpu().numpy().tobytes()) != runs["want"][c.name]:
                bad.append("%s: status %d, length %d" % (c.name, st[k], ln[k]))
        assert codec.error_flags() == 0
    assert not bad, "%d mismatches, the first: %s" % (len(bad), "; ".join(bad[:8]))


def test_run_cases_mapped_packed(runs):
    sel = [k for k, c in enumerate(runs["cases"]) if c.ws in VW_WIDTHS]
    sel = [sel[i] for i in np.random.default_rng(ec.SEED).permutation(len(sel))]
    cs = [runs["cases"][k] for k in sel]
    n = len(cs)
    out = torch.zeros(sum(encode_bound(c.n, c.ws) for c in cs), dtype=torch.uint8, device="cuda")
    codec = make_codec(4)
    off, st = codec.encode_vp(i64(runs["dev"][k].data_ptr() for k in sel), i64(c.n for c in cs), sum(c.n for c in cs), out,
                              word_sizes=i32(c.ws for c in cs), width_mask=mask_of(VW_WIDTHS),
                              mapbits=u64(bits_of(c.mapping) for c in cs))
    torch.cuda.synchronize()
    h, off = out.cpu().numpy(), off.cpu().numpy()
    assert int(st.abs().sum()) == 0
    bad = [c.name for k, c in enumerate(cs) if digest(h[off[k]:off[k + 1]].tobytes()) != runs["want"][c.name]]
    assert not bad, "%d mismatches, the first: %s" % (len(bad), "; ".join(bad[:8]))
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 5: messages above the tiled-path threshold
def test_large_messages(batch, mapped, orc, runs):
    """TDT_OPT_LARGE_MIN at 64 KiB (65,552 .. 262,208-byte messages are then large), the 589,840-byte
    case across a span, the speculated mapping and two others, a large passthrough message, a large
    message with a bad mapping, and a tile budget that one message exceeds."""
    rng = np.random.default_rng(5)
    big = [i for i, m in enumerate(batch["msgs"]) if len(m) >= 65552 and batch["ws"][i] in (2, 4, 8, 16)]
    msgs = [batch["msgs"][i] for i in big]
    ws = [batch["ws"][i] for i in big]
    maps = [mapped["maps"]["complement"][i] for i in big]
    want = [mapped["blobs"]["complement"][i] for i in big]
    tensors = [batch["tensors"][i] for i in big]
    spans = [k for k, c in enumerate(runs["cases"]) if c.n == ec.SIZE_SPAN and c.ws in (4, 8)]
    assert spans
    for k in spans:
        c = runs["cases"][k]
        spec = [1] * (c.ws - c.ws // 4) + [0] * (c.ws // 4)  # [1,1,1,0] / [1,1,1,1,1,1,0,0]
        for m in (spec, list(c.mapping), [int(x) for x in rng.integers(0, 2, c.ws)]):
            msgs.append(c.message)
            ws.append(c.ws)
            maps.append(m)
            want.append(mapped_blob(orc, c.message, c.ws, m))
            tensors.append(runs["dev"][k])
    passthrough = records(rng, 1, 262210)  # n % 4 != 0
    msgs.append(passthrough)
    ws.append(4)
    maps.append([1, 0, 1, 0])
    want.append(oracle_blob(orc, passthrough, 4))
    tensors.append(own(passthrough))
    bad_at = len(msgs)
    msgs.append(batch["msgs"][big[-1]])
    ws.append(batch["ws"][big[-1]])
    maps.append(None)
    want.append(b"")
    tensors.append(batch["tensors"][big[-1]])
    n = len(msgs)
    bits = [1 << 20 if m is None else bits_of(m) for m in maps]
    caps = [encode_bound(len(m), w) for m, w in zip(msgs, ws)]
    for tile_cap in (None, 16):  # 16 tiles: a 589,840-byte message (9 tiles) and a few more fit, the rest stay medium
        codec = make_codec(4)
        codec.set_option(OPT_LARGE_MIN, 65536)
        if tile_cap:
            codec.set_option(OPT_TILE_CAP, tile_cap)
        outs = [guarded(c) for c in caps]
        for rep in range(2):  # (the second call plans with the first one's counts)
            ln, st = codec.encode_vw(ptrs(tensors), i64(len(m) for m in msgs), i32(ws), mask_of([2, 4, 8, 16]),
                                     ptrs([v for _, v in outs]), i64(caps), mapbits=u64(bits))
        torch.cuda.synchronize()
        ln, st = ln.cpu().numpy(), st.cpu().numpy()
        for k in range(n):
            what = "message %d (width %d, %d bytes, tile cap %s)" % (k, ws[k], len(msgs[k]), tile_cap)
            h = outs[k][0].cpu().numpy()
            if k == bad_at:
                assert st[k] == E_BAD_MAPPING and ln[k] == 0 and (h == CANARY).all(), what
                continue
            assert st[k] == 0 and ln[k] == len(want[k]), what
            assert h[64:64 + ln[k]].tobytes() == want[k], what
            assert (h[:64] == CANARY).all() and (h[64 + ln[k]:] == CANARY).all(), what
        # an ordinary encode of the same batch on the same context (its tiles on) still gives its bytes
        plain = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
        pl, ps = codec.encode_vw(ptrs(tensors), i64(len(m) for m in msgs), i32(ws), mask_of([2, 4, 8, 16]), ptrs(plain),
                                 i64(caps))
        torch.cuda.synchronize()
        pl = pl.cpu().numpy()
        assert int(ps.abs().sum()) == 0
        for k in range(n):
            assert plain[k][: pl[k]].cpu().numpy().tobytes() == oracle_blob(orc, msgs[k], ws[k]), "plain message %d" % k
        assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 6: statuses
def test_bad_mappings_capacity_and_rejected_widths(orc):
    rng = np.random.default_rng(61)
    rows = []  # (width, size, mapping bits, capacity or None, wanted status)
    for w in (1, 4, 12):
        rows.append((w, 4104 if w == 12 else 4096, 1 << w, None, E_BAD_MAPPING))
        rows.append((w, 32784 if w == 12 else 32768, (1 << 63) | 1, None, E_BAD_MAPPING))
        rows.append((w, 1000, 1 << w, None, 0))              # UNCP: the bad mapping is ignored
        rows.append((w, 4104 if w == 12 else 4096, (1 << w) - 1, None, 0))
    rows.append((4, 32768, 0x5, -1, E_CAPACITY))            # one byte short
    # the rejected-width table of test_rejected_widths_and_short_capacity
    rows += [(0, 4096, 0, None, E_CONFIG), (-1, 1024, 0, None, E_CONFIG), (65, 65536, 0, None, E_UNSUPPORTED),
             (8, 4096, 0x3f, None, E_ARG)]
    msgs = [records(rng, w if 1 <= w <= 64 else 4, n) for w, n, _, _, _ in rows]
    want = []
    for (w, n, bits, cap, status), m in zip(rows, msgs):
        if status in (0, E_CAPACITY):
            mapping = [(bits >> p) & 1 for p in range(w)]
            want.append(mapped_blob(orc, m, w, mapping) if compresses(n, w) else oracle_blob(orc, m, w))
        else:
            want.append(b"")
    caps = [encode_bound(n, 16) if cap is None else len(b) + cap for (w, n, _, cap, _), b in zip(rows, want)]
    tensors = [own(m) for m in msgs]
    outs = [guarded(c) for c in caps]
    codec = make_codec(4)
    k = len(rows)
    ln = torch.full((k,), 77, dtype=torch.int64, device="cuda")
    st = torch.full((k,), 77, dtype=torch.int32, device="cuda")
    codec.encode_vw(ptrs(tensors), i64(r[1] for r in rows), i32(r[0] for r in rows), mask_of([1, 4, 12]),
                    ptrs([v for _, v in outs]), i64(caps), lengths=ln, status=st, mapbits=u64(r[2] for r in rows))
    torch.cuda.synchronize()
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    assert st.tolist() == [r[4] for r in rows]
    for i, (t, v) in enumerate(outs):
        assert canaries_intact(t, caps[i]), "message %d" % i
        if rows[i][4]:
            assert ln[i] == 0 and (v.cpu().numpy() == CANARY).all(), "message %d" % i
        else:
            assert v[: ln[i]].cpu().numpy().tobytes() == want[i], "message %d" % i
    assert codec.error_flags() == 0


def test_null_mapping_and_empty_batch():
    from psyne_amd._lib import TdtError
    lib_codec = make_codec(4)
    t = own(records(np.random.default_rng(62), 4, 4096))
    out = torch.zeros(encode_bound(4096, 4), dtype=torch.uint8, device="cuda")
    ln = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = lib_codec._stream(None)
    lib, h = lib_codec._lib, lib_codec._h
    p, n, o, c = ptrs([t]), i64([4096]), ptrs([out]), i64([out.numel()])
    off = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert lib.tdt_encode_mapped_v(h, p.data_ptr(), n.data_ptr(), None, 0, 1, None, o.data_ptr(), c.data_ptr(),
                                   ln.data_ptr(), st.data_ptr(), s) == E_ARG
    assert lib.tdt_encode_mapped_vp(h, p.data_ptr(), n.data_ptr(), None, 0, 1, 4096, None, out.data_ptr(), out.numel(),
                                    off.data_ptr(), st.data_ptr(), s) == E_ARG
    assert lib.tdt_mappings_v(h, p.data_ptr(), n.data_ptr(), None, 0, 1, ln.data_ptr(), None, st.data_ptr(), s) == E_ARG
    # call-level mask errors, as for encode_vw
    for mask in (0, 0x1ff):
        with pytest.raises(TdtError) as ei:
            lib_codec.encode_vw(p, n, i32([4]), mask, o, c, mapbits=u64([7]))
        assert ei.value.code == E_ARG
        with pytest.raises(TdtError) as ei:
            lib_codec.mappings_v(p, n, word_sizes=i32([4]), width_mask=mask)
        assert ei.value.code == E_ARG
    # a batch without messages touches nothing (null arrays included)
    assert lib.tdt_encode_mapped_v(h, None, None, None, 0, 0, None, None, None, None, None, s) == 0
    assert lib.tdt_encode_mapped_vp(h, None, None, None, 0, 0, 0, None, None, 0, None, None, s) == 0
    assert lib.tdt_mappings_v(h, None, None, None, 0, 0, None, None, None, s) == 0
    torch.cuda.synchronize()
    assert int(out.sum()) == 0 and lib_codec.error_flags() == 0


# ------------------------------------------------------------------------------- 7: packed


def test_encode_vp_mapped_is_the_concatenation(batch, mapped):
    idx = address_order(batch["tensors"], "shuffled")
    n = len(idx)
    tensors = [batch["tensors"][i] for i in idx]
    sizes = [t.numel() for t in tensors]
    for kind in ("random", "zeros"):
        want = [mapped["blobs"][kind][i] for i in idx]
        total = sum(len(b) for b in want)
        bits = u64(bits_of(mapped["maps"][kind][i]) for i in idx)
        kw = dict(word_sizes=i32(batch["ws"][i] for i in idx), width_mask=mask_of(WIDTHS), mapbits=bits)
        for first in (0, 1):  # (the mapped packed call takes the two phases whatever the option says)
            codec = make_codec(4)
            codec.set_option(OPT_PACK_SIZES_FIRST, first)
            t, out = guarded(total)
            off, st = codec.encode_vp(ptrs(tensors), i64(sizes), sum(sizes), out, **kw)
            torch.cuda.synchronize()
            got, o = packed_blobs(out, off)
            assert o.tolist() == np.concatenate([[0], np.cumsum([len(b) for b in want])]).tolist()
            assert st.cpu().numpy()[:n].tolist() == [0] * n and got == want and canaries_intact(t, total)
            assert codec.error_flags() == 0
        # out_cap short: the blobs that end past it are refused and not written, the need is still reported
        short = total - len(want[-1]) - len(want[-2]) + 1
        t, out = guarded(short)
        off, st = codec.encode_vp(ptrs(tensors), i64(sizes), sum(sizes), out, **kw)
        torch.cuda.synchronize()
        o, st = off.cpu().numpy(), st.cpu().numpy()[:n]
        assert int(o[n]) == total and canaries_intact(t, short)
        for k in range(n):
            fits = o[k + 1] <= short
            assert st[k] == (0 if fits else E_CAPACITY), k
            if fits:
                assert out[o[k]:o[k + 1]].cpu().numpy().tobytes() == want[k], k
    # a bad mapping occupies no bytes
    bad = bits.clone()
    live = next(k for k, i in enumerate(idx) if compresses(len(batch["msgs"][i]), batch["ws"][i]))
    bad[live] = -1
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    off, st = codec.encode_vp(ptrs(tensors), i64(sizes), sum(sizes), out, **dict(kw, mapbits=bad))
    torch.cuda.synchronize()
    o, st = off.cpu().numpy(), st.cpu().numpy()[:n]
    assert st[live] == E_BAD_MAPPING and o[live + 1] == o[live] and int(o[n]) == total - len(want[live])
    assert [int(x) for k, x in enumerate(st) if k != live] == [0] * (n - 1)


def test_pack_sizes_first_values_agree(batch, bands):
    """tdt_encode_batch_vp at option values 0, 1 and 2: identical output, offsets and statuses on the
    mixed-width batch and on the near ties; value 2, like value 1, uses no scratch (total_bytes = 0)."""
    sets = []
    idx = address_order(batch["tensors"], "shuffled")
    sets.append(([batch["tensors"][i] for i in idx], [batch["ws"][i] for i in idx], [batch["blobs"][i] for i in idx]))
    sets.append(([own(c["input"]) for c in bands], [c["ws"] for c in bands], [c["blob"] for c in bands]))
    for tensors, ws, want in sets:
        n = len(tensors)
        sizes = [t.numel() for t in tensors]
        total = sum(len(b) for b in want)
        got = {}
        for value in (0, 1, 2):
            codec = make_codec(4)
            codec.set_option(OPT_PACK_SIZES_FIRST, value)
            t, out = guarded(total)
            off, st = codec.encode_vp(ptrs(tensors), i64(sizes), sum(sizes) if value == 0 else 0, out, word_sizes=i32(ws),
                                      width_mask=mask_of(WIDTHS))
            torch.cuda.synchronize()
            assert canaries_intact(t, total) and codec.error_flags() == 0
            got[value] = (out.cpu().numpy().tobytes(), off.cpu().numpy().tolist(), st.cpu().numpy()[:n].tolist())
        assert got[0][0] == b"".join(want) and got[0][2] == [0] * n
        assert got[1] == got[0] and got[2] == got[0]
    # value 2 on a context of one width (no word sizes), the capacity short by the last blob
    w = 4
    sub = [i for i in idx if batch["ws"][i] == w]
    tensors, want = [batch["tensors"][i] for i in sub], [batch["blobs"][i] for i in sub]
    total = sum(len(b) for b in want)
    codec = make_codec(w)
    codec.set_option(OPT_PACK_SIZES_FIRST, 2)
    short = total - 1
    t, out = guarded(short)
    off, st = codec.encode_vp(ptrs(tensors), i64(x.numel() for x in tensors), 0, out)
    torch.cuda.synchronize()
    o, st = off.cpu().numpy(), st.cpu().numpy()[: len(sub)]
    assert int(o[-1]) == total and canaries_intact(t, short)
    assert st.tolist() == [0] * (len(sub) - 1) + [E_CAPACITY]
    assert out[: o[-2]].cpu().numpy().tobytes() == b"".join(want[:-1])
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- 8: capture
class _Mapped:
    """encode_vw(mapbits=...) over fixed tensors of widths 2, 4 and 12."""
    WS = [2, 4, 12, 4, 2, 12, 4, 2]
    NS = [1000, 4096, 4104, 32768, 65536, 32784, 100000, 262208]

    def __init__(self):
        self.c = make_codec(4)
        self.msgs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in self.NS]
        caps = [encode_bound(n, w) for n, w in zip(self.NS, self.WS)]
        self.enc = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
        self.tab = [ptrs(self.msgs), i64(self.NS), i32(self.WS), ptrs(self.enc), i64(caps)]
        self.bits = torch.zeros(len(self.NS), dtype=torch.int64, device="cuda")
        self.elen = torch.zeros(len(self.NS), dtype=torch.int64, device="cuda")
        self.est = torch.zeros(len(self.NS), dtype=torch.int32, device="cuda")

    def fill(self, seed):
        rng = np.random.default_rng(seed)
        host = [records(rng, w, n) for w, n in zip(self.WS, self.NS)]
        for t, m in zip(self.msgs, host):
            t.copy_(torch.from_numpy(m))
        maps = [[int(x) for x in rng.integers(0, 2, w)] for w in self.WS]
        self.bits.copy_(u64(bits_of(m) for m in maps))
        return host, maps

    def run(self, mapped=True):
        p, n, w, e, cap = self.tab
        self.c.encode_vw(p, n, w, mask_of(self.WS), e, cap, lengths=self.elen, status=self.est,
                         mapbits=self.bits if mapped else None)

    def check(self, orc, host, maps):
        torch.cuda.synchronize()
        ln = self.elen.cpu().numpy()
        assert int(self.est.abs().sum()) == 0
        for i, m in enumerate(host):
            w = self.WS[i]
            want = mapped_blob(orc, m, w, maps[i]) if compresses(len(m), w) else oracle_blob(orc, m, w)
            assert self.enc[i][: ln[i]].cpu().numpy().tobytes() == want, i


def test_capture_on_cold_context_is_refused():
    from psyne_amd._lib import TdtError
    s = _Mapped()
    s.fill(4)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with pytest.raises(TdtError) as ei:
        with torch.cuda.graph(gr):
            s.run()
    assert ei.value.code == E_CAPTURE


def test_capture_replays_with_the_mappings_of_the_moment(orc):
    s = _Mapped()
    host, maps = s.fill(1)
    s.run(mapped=False)  # an eager ORDINARY encode of this n_msgs and mask warms the context
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        s.run()
    gr.replay()
    s.check(orc, host, maps)
    for seed in (2, 3):  # new bytes and new mappings in the same arrays
        host, maps = s.fill(seed)
        gr.replay()
        s.check(orc, host, maps)
    maps = [[1 - x for x in m] for m in maps]  # the mapping array alone overwritten
    s.bits.copy_(u64(bits_of(m) for m in maps))
    gr.replay()
    s.check(orc, host, maps)
    assert s.c.error_flags() == 0


# ------------------------------------------------------------------------------- 9: histories
def test_histories_per_width_and_context_history_untouched(orc):
    rng = np.random.default_rng(55)
    codec = make_codec(4)

    def vw(widths, sizes):
        msgs = [records(rng, w, n) for w, n in zip(widths, sizes)]
        maps = [[int(x) for x in rng.integers(0, 2, w)] for w in widths]
        tensors = [own(m) for m in msgs]
        caps = [encode_bound(n, w) for w, n in zip(widths, sizes)]
        outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
        ln, st = codec.encode_vw(ptrs(tensors), i64(sizes), i32(widths), mask_of([2, 4, 8]), ptrs(outs), i64(caps),
                                 mapbits=u64(bits_of(m) for m in maps))
        torch.cuda.synchronize()
        ln = ln.cpu().numpy()
        assert int(st.abs().sum()) == 0
        for i, (m, w) in enumerate(zip(msgs, widths)):
            want = mapped_blob(orc, m, w, maps[i]) if compresses(len(m), w) else oracle_blob(orc, m, w)
            assert outs[i][: ln[i]].cpu().numpy().tobytes() == want, "message %d (width %d)" % (i, w)

    plain_msgs = [records(rng, 4, n) for n in (1000, 2048, 20000, 65536, 70000)]
    plain = [own(m) for m in plain_msgs]
    pcaps = [encode_bound(t.numel(), 4) for t in plain]

    def v():
        outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in pcaps]
        ln, st = codec.encode_v(ptrs(plain), i64(t.numel() for t in plain), ptrs(outs), i64(pcaps))
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0
        ln = ln.cpu().numpy()
        return [o[: ln[k]].cpu().numpy().tobytes() for k, o in enumerate(outs)]

    before = v()
    assert before == [oracle_blob(orc, m, 4) for m in plain_msgs]
    a_w, a_n = [2] * 6 + [4] * 4, [1024, 2048, 4096, 1024, 2048, 4096] + [65536] * 4
    vw(a_w, a_n)  # A: only small width-2 and only 64 KiB width-4 messages
    vw(a_w, a_n)  # A again: every other class, and width 8, are recorded empty
    # B: width 8 appears, and the size classes swap between widths 2 and 4
    vw([2] * 4 + [4] * 6 + [8] * 3, [65536] * 4 + [1024, 2048, 4096, 1024, 2048, 4096] + [1024, 20000, 65536])
    assert v() == before
    assert codec.error_flags() == 0


# ------------------------------------------------------------------------------- tensors
def test_encode_tensors_with_known_mappings(orc):
    g = torch.Generator(device="cuda")
    g.manual_seed(12)

    def sparse(n):
        return torch.randn(n, device="cuda", generator=g) * (torch.rand(n, device="cuda", generator=g) > 0.7)

    f32 = [sparse(n) for n in (1024, 16384, 80000)]
    tensors = f32 + [f32[1].to(torch.bfloat16), f32[2].to(torch.float64), torch.zeros(0, dtype=torch.float16, device="cuda"),
                     f32[0].to(torch.bfloat16)[:1001]]
    raw = [t.contiguous().view(torch.uint8).cpu().numpy() if t.numel() else np.zeros(0, np.uint8) for t in tensors]
    n = len(tensors)
    codec = make_codec(4)
    out, slots, ln, st, bits = codec.encode_tensors(tensors, word_sizes="dtype", return_mappings=True)
    out0, slots0, ln0, st0 = codec.encode_tensors(tensors, word_sizes="dtype")
    out1, _, ln1, st1 = codec.encode_tensors(tensors, word_sizes="dtype", mapbits=bits)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0 and int(st1.abs().sum()) == 0
    assert torch.equal(ln[:n], ln0[:n]) and torch.equal(ln1[:n], ln0[:n])
    oh, o0, o1, sl, lh = out.cpu().numpy(), out0.cpu().numpy(), out1.cpu().numpy(), slots.cpu().numpy(), ln.cpu().numpy()
    bh = bits.cpu().numpy().view(np.uint64)
    for i, (r, t) in enumerate(zip(raw, tensors)):
        w = t.element_size()
        want = oracle_blob(orc, r, w)
        assert oh[sl[i]:sl[i] + lh[i]].tobytes() == o0[sl[i]:sl[i] + lh[i]].tobytes() == want, "tensor %d" % i
        assert o1[sl[i]:sl[i] + lh[i]].tobytes() == want, "tensor %d" % i
        assert int(bh[i]) == (bits_of(orc.analyze(r, w)[2]) if compresses(r.size, w) else 0), "tensor %d" % i
    # packed, with the mappings kept from the slotted call
    pk, off, pst = codec.encode_tensors(tensors, word_sizes="dtype", packed=True, mapbits=bits)
    pk0, off0, _ = codec.encode_tensors(tensors, word_sizes="dtype", packed=True)
    torch.cuda.synchronize()
    total = int(off0[n])
    assert torch.equal(off, off0) and int(pst.abs().sum()) == 0 and torch.equal(pk[:total], pk0[:total])
    with pytest.raises(ValueError):
        codec.encode_tensors(tensors, mapbits=bits, return_mappings=True)
    assert codec.error_flags() == 0
