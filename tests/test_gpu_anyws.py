"""Generic word sizes (every width in 1..64 the tuned kernels do not take) on the GPU: context
creation, slotted and compacted round trips, analysis, caller mappings, decode routing inside a
mixed batch, the encode kernel's chunk boundaries, slot capacity and the host paths — each
compared with the CPU oracle byte for byte and status for status."""
import numpy as np
import pytest

from tests.anyws_cases import WIDTHS, from_streams, intended_mapping, kernel_chunk, load_anyws, low_pattern
from tests.support import E_CAPACITY, E_CONFIG, E_UNSUPPORTED, offsets_of

torch = pytest.importorskip("torch")
from tests.gpu_support import decode_slotted, encode_slotted, make_codec, orc  # noqa: E402, F401

pytestmark = pytest.mark.gpu

PHASES = ((0, 0), (3, 3), (5, 9), (16, 0))  # input / output byte phases (as test_gpu_parity's copy test)


@pytest.fixture(scope="module")
def cases():
    return load_anyws()


def test_context_creation():
    from psyne_amd import TDTConfig, TdtCodec
    from psyne_amd._lib import TdtError
    for ws in WIDTHS:
        c = make_codec(ws)
        assert c.error_flags() == 0
        c.close()
    with pytest.raises(TdtError) as e:
        TdtCodec(TDTConfig(word_size=65))
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(TdtError) as e:
        TdtCodec(TDTConfig(word_size=0))
    assert e.value.code == E_CONFIG


@pytest.mark.parametrize("ws", WIDTHS)
def test_slotted_round_trip_every_phase(cases, ws):
    sub = [c for c in cases if c.op == "encode" and c.ws == ws]
    assert len(sub) >= 4
    msgs = [c.input for c in sub]
    codec = make_codec(ws)
    for pi, po in PHASES:
        blobs, st, lens = encode_slotted(codec, msgs, pi, po)
        for c, b, s in zip(sub, blobs, st):
            assert s == 0 and b == c.expected.tobytes(), (c.name, pi, po, s)
        back, dst, dl = decode_slotted(codec, blobs, pi, po)
        for c, m, s in zip(sub, back, dst):
            assert s == 0 and m == c.input.tobytes(), (c.name, pi, po, s)
    assert codec.error_flags() == 0


@pytest.mark.parametrize("ws", WIDTHS)
def test_analyze(orc, cases, ws):
    sub = [c for c in cases if c.op == "encode" and c.ws == ws and c.input.size % ws == 0]
    codec = make_codec(ws)
    data = torch.from_numpy(np.concatenate([c.input for c in sub])).cuda()
    off = torch.from_numpy(offsets_of([c.input for c in sub])).cuda()
    hist, ent, mp, st = codec.analyze_batch(data, off)
    torch.cuda.synchronize()
    for i, c in enumerate(sub):
        wh, we, wm = orc.analyze(c.input, word_size=ws)
        assert int(st[i]) == 0, c.name
        assert np.array_equal(hist[i].cpu().numpy().astype(np.uint32), wh), c.name
        assert np.array_equal(mp[i].cpu().numpy(), wm), c.name
        assert np.array_equal(ent[i].cpu().numpy().view(np.uint64), we.view(np.uint64)), c.name  # bit patterns
    assert codec.error_flags() == 0


@pytest.mark.parametrize("ws", [5, 12, 40])
def test_encode_with_caller_mapping(orc, cases, ws):
    """tdt_encode_with_mapping_batch (compacted) with {0, 1} mappings other than the analysed one:
    the inverse of it, all ones (stream 0 empty) and all zeros (one stream)."""
    msgs = [c.input for c in cases if c.ws == ws and c.family in ("constructed", "uniform")]
    codec = make_codec(ws)
    inv = [1 - m for m in intended_mapping(ws)]
    maps = [inv, [1] * ws, [0] * ws]
    batch = [(m, mp) for m in msgs for mp in maps]
    data = torch.from_numpy(np.concatenate([m for m, _ in batch])).cuda()
    off = torch.from_numpy(offsets_of([m for m, _ in batch])).cuda()
    mapping = torch.tensor([mp for _, mp in batch], dtype=torch.int32, device="cuda")
    enc, eoff, st = codec.encode_batch(data, off, mapping=mapping)
    torch.cuda.synchronize()
    e, eo = enc.cpu().numpy(), eoff.cpu().numpy()
    for i, (m, mp) in enumerate(batch):
        want = orc.encode(m, cfg=orc.config(word_size=ws), bandwidth=10.0, mapping=mp)
        assert int(st[i]) == 0 and e[eo[i]:eo[i + 1]].tobytes() == want, (i, mp)
    # an entry outside {0, 1}: TDT_E_BAD_MAPPING and an empty output, the other messages intact
    mapping[1, ws - 1] = 2
    enc, eoff, st = codec.encode_batch(data, off, mapping=mapping)
    torch.cuda.synchronize()
    e, eo = enc.cpu().numpy(), eoff.cpu().numpy()
    assert int(st[1]) == 4 and eo[2] == eo[1]
    assert e[eo[0]:eo[1]].tobytes() == orc.encode(batch[0][0], cfg=orc.config(word_size=ws), bandwidth=10.0,
                                                  mapping=batch[0][1])
    assert codec.error_flags() == 0


def test_compacted_ws12(orc, cases):
    msgs = [c.input for c in cases if c.op == "encode" and c.ws == 12]
    codec = make_codec(12)
    data = np.concatenate(msgs)
    off = offsets_of(msgs)
    want, woff = orc.encode_batch(data, off, cfg=orc.config(word_size=12), bandwidth=10.0)
    enc, eoff, st = codec.encode_batch(torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda())
    dec, doff, dst = codec.decode_batch(enc, eoff)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0 and int(dst.abs().sum()) == 0
    assert np.array_equal(eoff.cpu().numpy().astype(np.uint64), woff)
    assert enc.cpu().numpy()[: int(woff[-1])].tobytes() == want
    assert np.array_equal(doff.cpu().numpy(), off) and np.array_equal(dec.cpu().numpy()[: data.size], data)
    assert codec.error_flags() == 0


def mixed_blobs(cases, golden):
    """(name, blob) of the routing test, interleaved: word-size-4 blobs and UNCP blobs (the tuned
    kernels' and the copy list's), blobs of word sizes 3, 12 and 40, every decode-only blob, one
    bad magic."""
    tuned = [(c.name, c.expected.tobytes()) for c in golden
             if c.op == "encode" and c.ws == 4 and c.input.size <= 4200][:10]
    generic = [(c.name, c.expected.tobytes()) for c in cases if c.op == "encode" and c.ws in (3, 12, 40)]
    crafted = [(c.name, c.input.tobytes()) for c in cases if c.op == "decode"]
    crafted.append(("bad_magic", b"ABCD" + bytes(60)))
    assert any(b[:4] == b"PCNU" for _, b in tuned) and any(b[:4] == b"DTDT" for _, b in tuned)
    lists = [tuned, generic, crafted]
    out = []
    for i in range(max(len(x) for x in lists)):
        out += [x[i] for x in lists if i < len(x)]
    return out


def test_mixed_decode_batch_routing(orc, cases, golden):
    blobs = mixed_blobs(cases, golden)
    lib_status = {c.name: c.lib_status for c in cases if "lib_status" in c}
    want = []
    for name, b in blobs:
        s, out = orc.decode(b)
        if name in lib_status:  # word size 65: valid for the reference, above the library's bound
            s, out = lib_status[name], b""
        want.append((s, out))
    assert sum(s == 0 for s, _ in want) >= 25 and {s for s, _ in want} >= {0, 2, 3, 4, 6}
    codec = make_codec(4)
    raw = [b for _, b in blobs]
    for pi, po in ((0, 0), (5, 9)):
        got, st, lens = decode_slotted(codec, raw, pi, po)
        for (name, _), (ws_, wout), g, s, l in zip(blobs, want, got, st, lens):
            assert s == ws_, (name, s, ws_)
            assert l == len(wout) and g == wout, name
    # compacted
    data = torch.from_numpy(np.frombuffer(b"".join(raw), np.uint8).copy()).cuda()
    off = torch.from_numpy(offsets_of(raw)).cuda()
    dec, doff, dst = codec.decode_batch(data, off)
    torch.cuda.synchronize()
    d, do = dec.cpu().numpy(), doff.cpu().numpy()
    for i, ((name, _), (ws_, wout)) in enumerate(zip(blobs, want)):
        assert int(dst[i]) == ws_, (name, int(dst[i]), ws_)
        assert do[i + 1] - do[i] == len(wout) and d[do[i]:do[i + 1]].tobytes() == wout, name
    # compacted, one pass (the look-back kernel places the deferred blobs): the output is one byte
    # short, so the last blob that decodes reports TDT_E_CAPACITY and the ones before it decode
    total = int(do[-1])
    last_ok = max(i for i, (s, o) in enumerate(want) if s == 0 and len(o))
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    dec, doff, dst = codec.decode_batch(data, off, out=out, out_capacity=total - 1)
    torch.cuda.synchronize()
    d = dec.cpu().numpy()
    assert np.array_equal(doff.cpu().numpy(), do)
    for i, ((name, _), (ws_, wout)) in enumerate(zip(blobs, want)):
        end_fits = do[i + 1] <= total - 1
        assert int(dst[i]) == (ws_ if ws_ or end_fits else E_CAPACITY), (name, int(dst[i]))
        if ws_ == 0 and end_fits:
            assert d[do[i]:do[i + 1]].tobytes() == wout, name
    assert int(dst[last_ok]) == E_CAPACITY and int((out[total:] != 0xA5).sum()) == 0
    assert codec.error_flags() == 0


def boundary_message(ws, n_target, rng, chunk):
    """A message whose low stream has runs ending exactly at, one before and one after the stream
    positions of the message bytes at multiples of `chunk`, and at stream positions that are
    themselves such multiples; every other boundary closes a run longer than 255."""
    mp = intended_mapping(ws)
    k = mp.count(0)
    wc = (n_target // ws + 3) // 4 * 4
    before = np.concatenate([[0], np.cumsum([1 - m for m in mp])])  # low positions below p
    S = wc * k
    marks = set()
    step = max(1, (wc * ws // chunk) // 96)  # at most ~100 chunk edges of a long message
    for m in range(1, wc * ws // chunk + 1, step):
        for d in (-1, 0, 1):
            j = m * chunk + d
            if 0 < j < wc * ws:
                marks.add(int((j // ws) * k + before[j % ws]))
            if 0 < m * chunk + d < S:
                marks.add(m * chunk + d)
    runs, pos, val, flip = [], 0, 0, 0
    for b in sorted(marks) + [S]:
        gap = b - pos
        if gap <= 0:
            continue
        flip ^= 1
        tail = min(gap, int(rng.choice([256, 300, 511, 600, 766]))) if flip else min(gap, int(rng.integers(1, 6)))
        left = gap - tail
        while left > 0:
            r = min(left, int(rng.integers(1, 60)))
            val = (val + 1 + int(rng.integers(0, 3))) % 7
            runs.append((r, val))
            left -= r
        val = (val + 1 + int(rng.integers(0, 3))) % 7
        runs.append((tail, val))
        pos = b
    low = np.repeat(np.array([v for _, v in runs], np.uint8), [r for r, _ in runs])
    assert low.size == S
    return from_streams(ws, wc, low, rng)


@pytest.mark.parametrize("ws", [3, 12])
def test_chunk_boundaries(orc, ws):
    chunk = kernel_chunk()
    assert chunk % 16 == 0
    rng = np.random.default_rng(4096 + ws)
    msgs = [boundary_message(ws, 3 << 19, rng, chunk), boundary_message(ws, 20 * 1024, rng, chunk),
            # a constant low stream: one run across every chunk, closed only at the stream's end
            from_streams(ws, 4096, np.full(4096 * intended_mapping(ws).count(0), 9, np.uint8), rng)]
    cfg = orc.config(word_size=ws)
    for m in msgs[:2]:
        assert list(orc.analyze(m, word_size=ws)[2]) == intended_mapping(ws)
    codec = make_codec(ws)
    for pi, po in ((0, 0), (5, 9)):
        blobs, st, _ = encode_slotted(codec, msgs, pi, po)
        for i, m in enumerate(msgs):
            assert st[i] == 0 and blobs[i] == orc.encode(m, cfg=cfg, bandwidth=10.0), (i, pi, po)
        back, dst, _ = decode_slotted(codec, blobs, pi, po)
        for i, m in enumerate(msgs):
            assert dst[i] == 0 and back[i] == m.tobytes(), (i, pi, po)
    assert codec.error_flags() == 0


def test_capacity(orc, cases):
    by = {c.name: c for c in cases}
    a, b = by["constructed_ws12"], by["uniform_ws12"]
    la, lb = a.expected.size, b.expected.size
    codec = make_codec(12)
    # encode: message 0's slot is one byte too small, message 1's is exact
    blobs, st, lens = encode_slotted(codec, [a.input, b.input], slots=[0, la - 1, la - 1 + lb])
    assert st == [E_CAPACITY, 0] and lens == [0, lb] and blobs[1] == b.expected.tobytes()
    blobs, st, lens = encode_slotted(codec, [a.input, b.input], 3, 3, slots=[0, la, la + lb])
    assert st == [0, 0] and blobs == [a.expected.tobytes(), b.expected.tobytes()]
    # decode of generic blobs, on a context of another width
    codec4 = make_codec(4)
    raw = [a.expected.tobytes(), b.expected.tobytes()]
    na, nb = a.input.size, b.input.size
    back, st, lens = decode_slotted(codec4, raw, slots=[0, na - 1, na - 1 + nb])
    assert st == [E_CAPACITY, 0] and lens == [0, nb] and back[1] == b.input.tobytes()
    back, st, lens = decode_slotted(codec4, raw, 5, 9, slots=[0, na, na + nb])
    assert st == [0, 0] and back == [a.input.tobytes(), b.input.tobytes()]
    assert codec.error_flags() == 0 and codec4.error_flags() == 0


def test_host_paths(orc, cases):
    from psyne_amd import TDTCompressionProtocol, TDTConfig
    sub = [c for c in cases if c.op == "encode" and c.ws == 12]
    p = TDTCompressionProtocol(TDTConfig(word_size=12, sample_fraction=1.0))
    p.update_network_metrics(10.0, 1.0)
    for c in sub:  # one message per call
        blob = p.encode(c.input.tobytes())
        assert blob == c.expected.tobytes(), c.name
        assert p.decode(blob) == c.input.tobytes(), c.name
    p.analyze_data(sub[0].input.tobytes(), sub[0].input.size)
    assert p.get_average_entropy() == float(sum(float(e) for e in orc.analyze(sub[0].input, word_size=12)[1])) / 12
    # a batch of 8 messages through the pipeline
    rng = np.random.default_rng(8)
    msgs = [c.input for c in sub]
    while len(msgs) < 8:
        msgs.append(from_streams(12, 128 + 4 * len(msgs), low_pattern((128 + 4 * len(msgs)) * 8, rng), rng))
    msgs = msgs[:8]
    data, off = np.concatenate(msgs), offsets_of(msgs).astype(np.uint64)
    enc, eoff, st = p.codec.encode_host(data, off)
    want, woff = orc.encode_batch(data, off.astype(np.int64), cfg=orc.config(word_size=12), bandwidth=10.0)
    assert not st.any() and np.array_equal(eoff, woff) and enc.tobytes() == want
    dec, doff, dst = p.codec.decode_host(enc, eoff, data.size)
    assert not dst.any() and np.array_equal(doff, off) and dec.tobytes() == data.tobytes()
    # ... and the generic blobs through another width's context (the blob's header decides)
    dec, doff, dst = make_codec(4).decode_host(enc, eoff, data.size)
    assert not dst.any() and dec.tobytes() == data.tobytes()
    assert p.codec.error_flags() == 0


def test_slotted_calls_under_graph_capture(cases):
    """The slotted entry points read nothing back: a captured encode + decode of a generic width
    replays to the eager bytes.  The compacted encode needs the batch size on the host: without
    the two-phase route it reports TDT_E_UNSUPPORTED."""
    from psyne_amd._lib import TDT_OPT_NO_TWO_PHASE, TdtError
    sub = [c for c in cases if c.op == "encode" and c.ws == 12]
    msgs = [c.input for c in sub]
    n = len(msgs)
    codec = make_codec(12)
    data = torch.from_numpy(np.concatenate(msgs)).cuda()
    off = torch.from_numpy(offsets_of(msgs)).cuda()
    slots = codec.encode_slots(off)
    out = torch.zeros(int(slots[-1].item()), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    back = torch.zeros(data.numel(), dtype=torch.uint8, device="cuda")
    blens = torch.zeros(n, dtype=torch.int64, device="cuda")
    dst = torch.zeros(n, dtype=torch.int32, device="cuda")

    def run():
        codec.encode_into(data, off, slots=slots, out=out, lengths=lens, status=st)
        codec.decode_into(out, slots, in_lengths=lens, slots=off, out=back, lengths=blens, status=dst)

    run()  # eager: warms the workspaces
    torch.cuda.synchronize()
    for t in (out, lens, back, blens):
        t.zero_()
    st.fill_(-1)
    dst.fill_(-1)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        run()
    gr.replay()
    torch.cuda.synchronize()
    o, sl, l = out.cpu().numpy(), slots.cpu().numpy(), lens.cpu().numpy()
    for i, c in enumerate(sub):
        assert int(st[i]) == 0 and o[sl[i]:sl[i] + l[i]].tobytes() == c.expected.tobytes(), c.name
    assert int(dst.abs().sum()) == 0 and torch.equal(back, data)
    codec.set_option(TDT_OPT_NO_TWO_PHASE, 1)
    with pytest.raises(TdtError) as e:
        codec.encode_batch(data, off)
    assert e.value.code == E_UNSUPPORTED
    assert codec.error_flags() == 0
