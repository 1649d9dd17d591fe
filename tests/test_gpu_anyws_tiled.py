"""The tiled encode of long generic-width messages (psyne_amd/csrc/tdt_anyws.h) on the GPU: every
blob, length and status against the CPU oracle byte for byte, between 0xA5 guard bytes, and the same
with TDT_OPT_ANY_TILED at 1 and at 0 (the option is the A/B switch: a library without the tile
pipeline does not know it, and every test here raises there).  TDT_OPT_LARGE_MIN is one tile, so
messages of two to five tiles run the plan, histogram, mapping, count, scan and emit kernels."""
import numpy as np
import pytest

from oracle.oracle import encode_bound
from tests import anyws_tiled_cases as tc
from tests.support import E_CAPACITY, bits_of, mask_of, offsets_of

torch = pytest.importorskip("torch")
from tests.gpu_support import (canaries_intact, decode_slotted, encode_slotted, guarded, i32, i64,  # noqa: E402, F401
                               orc, own, ptrs, u64)

pytestmark = pytest.mark.gpu

OPT_LARGE_MIN, OPT_TILE_CAP, OPT_PACK_SIZES_FIRST, OPT_ANY_TILED = 1, 2, 7, 8
TILE = tc.kernel_tile()
SWITCH = (1, 0)  # TDT_OPT_ANY_TILED: the tile pipeline, then the one-workgroup kernel


def make_codec(ws, tiled, large_min=TILE, bandwidth=10.0):
    from psyne_amd import TDTConfig, TdtCodec
    codec = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws))
    codec.set_metrics(bandwidth, 1.0, 0.5)  # bandwidth < 100 Mbps: compression on
    codec.set_option(OPT_LARGE_MIN, large_min)
    codec.set_option(OPT_ANY_TILED, tiled)
    return codec


def plain(orc, m, ws, **kw):
    return orc.encode(m, cfg=orc.config(sample_fraction=1.0, word_size=ws), **kw)


def same_under_both(run, ws, **kw):
    """run(codec) with the option at 1 and at 0: identical results (blobs, lengths, statuses), returned once."""
    got = []
    for tiled in SWITCH:
        codec = make_codec(ws, tiled, **kw)
        got.append(run(codec))
        assert codec.error_flags() == 0
        codec.close()
    assert got[0] == got[1], "TDT_OPT_ANY_TILED changes the result"
    return got[0]


def scattered(codec, msgs, caps, call, order=None):
    """One scattered call over `msgs` (own allocations, guarded outputs) in `order`: (blobs, statuses, lengths)
    by message."""
    idx = list(range(len(msgs))) if order is None else list(order)
    tensors = [own(msgs[i], lead=(3 * i) % 16) for i in idx]
    outs = [guarded(caps[i]) for i in idx]
    ln, st = call(codec, ptrs(tensors), i64(t.numel() for t in tensors), ptrs([v for _, v in outs]), i64(caps[i] for i in idx), idx)
    torch.cuda.synchronize()
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    blobs, sts, lens = [None] * len(msgs), [None] * len(msgs), [None] * len(msgs)
    for k, i in enumerate(idx):
        assert canaries_intact(outs[k][0], caps[i]), "message %d: a byte outside the slot was written" % i
        blobs[i] = outs[k][1][: ln[k]].cpu().numpy().tobytes()
        sts[i], lens[i] = int(st[k]), int(ln[k])
    return blobs, sts, lens


@pytest.fixture(scope="module")
def structures(orc):
    """Per (width, mapping kind): the structured messages, their blobs under that mapping and analysed."""
    memo = {}

    def get(ws, mkind):
        if (ws, mkind) not in memo:
            mapping = tc.mapping_of(ws, mkind)
            named = tc.cases_for(ws, mkind, TILE)
            msgs = [m for _, m in named]
            memo[ws, mkind] = dict(names=[k for k, _ in named], msgs=msgs, mapping=mapping,
                                   mapped=[plain(orc, m, ws, mapping=mapping) for m in msgs],
                                   analysed=[plain(orc, m, ws) for m in msgs])
        return memo[ws, mkind]
    return get


# ------------------------------------------------------------------------------- 1: run structures, both streams
@pytest.mark.parametrize("ws", tc.WIDTHS)
def test_structures_with_the_callers_mapping(orc, structures, ws):
    """Boundary runs, crossing runs of 254 .. 765, runs over one and three whole tiles, constant
    streams — in both streams, under mappings that put stream 1 low, high and interleaved:
    encode_v(mapbits=...), shuffled, and decode_v back."""
    for mkind in tc.MAPPINGS:
        S = structures(ws, mkind)
        msgs, n = S["msgs"], len(S["msgs"])
        caps = [encode_bound(m.size, ws) for m in msgs]
        order = np.random.default_rng(5).permutation(n)
        bits = bits_of(S["mapping"])

        def run(codec):
            return scattered(codec, msgs, caps, lambda c, p, s, op, oc, idx: c.encode_v(p, s, op, oc, mapbits=u64([bits] * n)),
                             order)
        blobs, st, lens = same_under_both(run, ws)
        for k, name in enumerate(S["names"]):
            assert st[k] == 0 and blobs[k] == S["mapped"][k], (ws, mkind, name)
        codec = make_codec(ws, 1)
        back = [torch.zeros(m.size, dtype=torch.uint8, device="cuda") for m in msgs]
        held = [own(b) for b in blobs]  # (alive until the call has run)
        dl, ds = codec.decode_v(ptrs(held), i64(lens), ptrs(back), i64(m.size for m in msgs))
        torch.cuda.synchronize()
        assert int(ds.abs().sum()) == 0
        for k, m in enumerate(msgs):
            assert np.array_equal(back[k].cpu().numpy(), m), (ws, mkind, S["names"][k])


@pytest.mark.parametrize("ws", tc.WIDTHS)
def test_structures_analysed_slotted(orc, structures, ws):
    """The same messages through the slotted encode (histograms and mapping on the device) and back."""
    for mkind in tc.MAPPINGS:
        S = structures(ws, mkind)
        blobs, st, lens = same_under_both(lambda codec: encode_slotted(codec, S["msgs"]), ws)
        for k, name in enumerate(S["names"]):
            assert st[k] == 0 and blobs[k] == S["analysed"][k], (ws, mkind, name)
        if mkind == "interleaved":
            back, dst, _ = decode_slotted(make_codec(ws, 1), blobs)
            assert not any(dst) and back == [m.tobytes() for m in S["msgs"]]


def test_compacted_with_mapping(orc, structures):
    """tdt_encode_with_mapping_batch: the contiguous known-mapping route (one int32 per position)."""
    ws = 12
    S = structures(ws, "low")
    msgs = S["msgs"][:4]
    data = torch.from_numpy(np.concatenate(msgs)).cuda()
    off = torch.from_numpy(offsets_of(msgs)).cuda()
    mp = torch.tensor([S["mapping"]] * len(msgs), dtype=torch.int32, device="cuda")

    def run(codec):
        enc, eoff, st = codec.encode_batch(data, off, mapping=mp)
        torch.cuda.synchronize()
        e, eo = enc.cpu().numpy(), eoff.cpu().numpy()
        return [e[eo[i]:eo[i + 1]].tobytes() for i in range(len(msgs))], st.cpu().numpy()[: len(msgs)].tolist()
    blobs, st = same_under_both(run, ws)
    assert st == [0] * len(msgs) and blobs == S["mapped"][:4]


# ------------------------------------------------------------------------------- 2: one stream, zeros, thresholds
def test_one_stream_and_all_zeros(orc):
    """Every position alike (no entropy above the mean: one stream, stream 1 absent) and all zeros."""
    for ws in (3, 12, 64):
        wc = tc.round_up(2 * TILE, ws) // ws + 77 * (tc.unit(ws) // ws)
        col = (np.arange(wc) // 300 % 7 + 1).astype(np.uint8)
        alike = np.repeat(col, ws)
        msgs = [alike, np.zeros(wc * ws, np.uint8)]
        blobs, st, _ = same_under_both(lambda codec: encode_slotted(codec, msgs), ws)
        for m, b, s in zip(msgs, blobs, st):
            assert s == 0 and b == plain(orc, m, ws), ws
            assert np.frombuffer(b[8:12], "<u4")[0] == 1, "one stream"


@pytest.mark.parametrize("ws", [12, 64])
def test_at_and_just_above_the_threshold(orc, ws):
    """A message of exactly TDT_OPT_LARGE_MIN bytes stays on one workgroup, one unit longer is tiled:
    the same bytes either way."""
    rng = np.random.default_rng(ws)
    msgs = [tc.structured(ws, "interleaved", 1, k, ("edges", "dense"), TILE, seed=21 + k) for k in (1, 2)]
    n = msgs[0].size
    assert n > TILE and msgs[1].size == n + tc.unit(ws)
    msgs.append(rng.integers(0, 4, n, dtype=np.uint8))
    blobs, st, _ = same_under_both(lambda codec: encode_slotted(codec, msgs), ws, large_min=n)
    assert st == [0] * 3 and blobs == [plain(orc, m, ws) for m in msgs]


# ------------------------------------------------------------------------------- 3: passthrough by tiles
@pytest.mark.parametrize("pi,po", [(0, 0), (3, 3), (5, 9)])
def test_uncp_by_tiles(orc, pi, po):
    """A long message that is no whole number of words, and one with the policy off: "UNCP" + the
    payload, copied tile by tile, at every byte phase."""
    ws = 12
    rng = np.random.default_rng(3)
    odd = rng.integers(0, 256, 3 * TILE + 1000 * 12 + 4, dtype=np.uint8)  # (a multiple of 4, not of 12)
    assert odd.size % 4 == 0 and odd.size % ws
    blobs, st, _ = same_under_both(lambda codec: encode_slotted(codec, [odd], pi, po), ws)
    assert st == [0] and blobs[0] == b"PCNU" + odd.tobytes() == plain(orc, odd, ws)
    whole = rng.integers(0, 3, tc.round_up(2 * TILE, ws) + 120, dtype=np.uint8)
    blobs, st, _ = same_under_both(lambda codec: encode_slotted(codec, [whole, odd[:1000]], pi, po), ws, bandwidth=1000.0)
    assert st == [0, 0] and blobs == [b"PCNU" + whole.tobytes(), b"PCNU" + odd[:1000].tobytes()]
    back, dst, _ = decode_slotted(make_codec(ws, 1), blobs, pi, po)
    assert not any(dst) and back[0] == whole.tobytes()


# ------------------------------------------------------------------------------- 4: batches, budgets, capacity
def test_long_beside_short(orc, structures):
    ws = 12
    rng = np.random.default_rng(11)
    S = structures(ws, "high")
    msgs = [rng.integers(0, 5, 1020, dtype=np.uint8), S["msgs"][4], rng.integers(0, 2, 48 * 1024, dtype=np.uint8),
            S["msgs"][1], np.zeros(0, np.uint8)]
    blobs, st, _ = same_under_both(lambda codec: encode_slotted(codec, msgs), ws)
    assert st == [0] * len(msgs) and blobs == [plain(orc, m, ws) for m in msgs]


def test_tile_budget_fallback(orc, structures):
    """Two long messages, a tile budget with room for one: the other stays on the one-workgroup kernel."""
    ws = 5
    S = structures(ws, "interleaved")
    msgs = [S["msgs"][2], S["msgs"][3]]
    tiles = [-(-m.size // TILE) for m in msgs]

    def run(codec):
        codec.set_option(OPT_TILE_CAP, max(tiles))
        first = encode_slotted(codec, msgs)
        return first, encode_slotted(codec, msgs)  # (again, with the first call's counts known)
    (blobs, st, _), again = same_under_both(run, ws)
    assert st == [0, 0] and blobs == S["analysed"][2:4] and again[0] == blobs


def test_capacity_one_byte_short(orc, structures):
    """A slot one byte short of the blob: TDT_E_CAPACITY, length 0, nothing outside the slot; the
    message beside it is untouched by that."""
    ws = 40
    S = structures(ws, "low")
    msgs, want = S["msgs"][1:3], S["analysed"][1:3]
    slots = np.cumsum([0, len(want[0]) - 1, len(want[1])])
    blobs, st, lens = same_under_both(lambda codec: encode_slotted(codec, msgs, 3, 5, slots=slots), ws)
    assert st == [E_CAPACITY, 0] and lens == [0, len(want[1])] and blobs[1] == want[1]
    big = np.zeros(tc.round_up(2 * TILE, ws) + 4, np.uint8)  # a passthrough message (no whole number of words)
    assert big.size % ws
    blobs, st, lens = same_under_both(lambda codec: encode_slotted(codec, [big], slots=[0, big.size + 3]), ws)
    assert st == [E_CAPACITY] and lens == [0]


# ------------------------------------------------------------------------------- 5: routes
def test_compacted_two_phase(orc, structures):
    ws = 3
    S = structures(ws, "interleaved")
    msgs = S["msgs"][:5] + [np.arange(600, dtype=np.uint8)]
    data, off = np.concatenate(msgs), offsets_of(msgs)
    want, woff = orc.encode_batch(data, off, cfg=orc.config(sample_fraction=1.0, word_size=ws), bandwidth=10.0)

    def run(codec):
        enc, eoff, st = codec.encode_batch(torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda())
        dec, doff, dst = codec.decode_batch(enc, eoff)
        torch.cuda.synchronize()
        assert int(dst.abs().sum()) == 0 and np.array_equal(dec.cpu().numpy()[: data.size], data)
        eo = eoff.cpu().numpy()
        return enc.cpu().numpy()[: int(eo[-1])].tobytes(), eo.tolist(), st.cpu().numpy()[: len(msgs)].tolist()
    blob, eo, st = same_under_both(run, ws)
    assert st == [0] * len(msgs) and eo == woff.astype(np.int64).tolist() and blob == want


def test_encode_v_shuffled_sizes_and_mappings(orc, structures):
    """encode_v in shuffled address order; encoded_sizes_v and mappings_v give its lengths and the
    mappings it decided; encode_v with those mappings gives its bytes."""
    ws = 12
    S = structures(ws, "interleaved")
    rng = np.random.default_rng(2)
    msgs = S["msgs"] + [rng.integers(0, 3, 2400, dtype=np.uint8), rng.integers(0, 256, TILE + 10, dtype=np.uint8)]
    want = S["analysed"] + [plain(orc, m, ws) for m in msgs[-2:]]
    caps = [encode_bound(m.size, ws) for m in msgs]
    order = np.random.default_rng(9).permutation(len(msgs))

    def run(codec):
        enc = scattered(codec, msgs, caps, lambda c, p, s, op, oc, idx: c.encode_v(p, s, op, oc), order)
        tensors = [own(m) for m in msgs]
        args = (ptrs(tensors), i64(t.numel() for t in tensors))
        es, est = codec.encoded_sizes_v(*args)
        ms, bits, mst = codec.mappings_v(*args)
        torch.cuda.synchronize()
        sizes = (es.cpu().numpy().tolist(), est.cpu().numpy().tolist(), ms.cpu().numpy().tolist(), mst.cpu().numpy().tolist())
        again = scattered(codec, msgs, caps, lambda c, p, s, op, oc, idx: c.encode_v(p, s, op, oc, mapbits=bits))
        return enc, sizes, bits.cpu().numpy().tolist(), again
    (blobs, st, lens), (es, est, ms, mst), bits, again = same_under_both(run, ws)
    n = len(msgs)
    assert st == [0] * n and blobs == want
    assert es == ms == lens and est == mst == [0] * n
    for k, m in enumerate(msgs):
        live = m.size % ws == 0 and m.size % 4 == 0 and m.size >= 1024
        assert bits[k] == (bits_of(orc.analyze(m, ws)[2]) if live else 0), k
    assert again == (blobs, st, lens)


def test_encode_vw_widths_12_and_4(orc, structures):
    """Mixed widths in one call: long messages at width 12 (tiles of the generic pipeline) and at
    width 4 (the tuned one), short ones of both between them."""
    S = structures(12, "low")
    rng = np.random.default_rng(4)
    f = rng.normal(0, 0.01, (3 * TILE + 4096) // 4).astype(np.float32)
    f[rng.random(f.size) < 0.6] = 0
    msgs = [S["msgs"][0], f.view(np.uint8), rng.integers(0, 3, 1200, dtype=np.uint8), S["msgs"][5],
            rng.integers(0, 3, 2048, dtype=np.uint8), S["msgs"][3]]
    widths = [12, 4, 12, 12, 4, 12]
    want = [plain(orc, m, w) for m, w in zip(msgs, widths)]
    caps = [encode_bound(m.size, w) for m, w in zip(msgs, widths)]

    def run(codec):
        return scattered(codec, msgs, caps,
                         lambda c, p, s, op, oc, idx: c.encode_vw(p, s, i32(widths[i] for i in idx), mask_of(widths), op, oc),
                         [5, 1, 3, 0, 4, 2])
    blobs, st, _ = same_under_both(run, 4)
    assert st == [0] * len(msgs) and blobs == want


@pytest.mark.parametrize("first", [0, 1, 2])
def test_encode_vp(orc, structures, first):
    """The packed encode at every value of TDT_OPT_PACK_SIZES_FIRST."""
    ws = 5
    S = structures(ws, "high")
    msgs = S["msgs"][:6] + [np.full(900, 7, np.uint8)]
    want = S["analysed"][:6] + [plain(orc, msgs[-1], ws)]
    total = sum(len(b) for b in want)

    def run(codec):
        codec.set_option(OPT_PACK_SIZES_FIRST, first)
        tensors = [own(m, lead=5 * k % 16) for k, m in enumerate(msgs)]
        raw, out = guarded(total)
        off, st = codec.encode_vp(ptrs(tensors), i64(t.numel() for t in tensors), sum(m.size for m in msgs), out)
        torch.cuda.synchronize()
        assert canaries_intact(raw, total)
        return out.cpu().numpy().tobytes(), off.cpu().numpy().tolist(), st.cpu().numpy()[: len(msgs)].tolist()
    packed, off, st = same_under_both(run, ws)
    assert st == [0] * len(msgs) and off == np.cumsum([0] + [len(b) for b in want]).tolist()
    assert packed == b"".join(want)


# ------------------------------------------------------------------------------- 6: capture
def test_captured_slotted_call_replays(orc, structures):
    """A warm slotted call reads nothing back on the host: captured, it replays to the eager bytes."""
    ws = 12
    S = structures(ws, "interleaved")
    msgs, n = S["msgs"][:4], 4
    data = torch.from_numpy(np.concatenate(msgs)).cuda()
    off = torch.from_numpy(offsets_of(msgs)).cuda()
    got = []
    for tiled in SWITCH:
        codec = make_codec(ws, tiled)
        slots = codec.encode_slots(off)
        out = torch.zeros(int(slots[-1].item()), dtype=torch.uint8, device="cuda")
        lens = torch.zeros(n, dtype=torch.int64, device="cuda")
        st = torch.zeros(n, dtype=torch.int32, device="cuda")
        for _ in range(2):  # eager: the workspaces grow, and the second call knows the first one's counts
            codec.encode_into(data, off, slots=slots, out=out, lengths=lens, status=st)
            torch.cuda.synchronize()
        out.zero_()
        lens.zero_()
        st.fill_(-1)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            codec.encode_into(data, off, slots=slots, out=out, lengths=lens, status=st)
        gr.replay()
        torch.cuda.synchronize()
        o, sl, l = out.cpu().numpy(), slots.cpu().numpy(), lens.cpu().numpy()
        got.append(([o[sl[i]:sl[i] + l[i]].tobytes() for i in range(n)], st.cpu().numpy().tolist()))
        assert codec.error_flags() == 0
        del gr
    assert got[0] == got[1] == (S["analysed"][:4], [0] * n)
