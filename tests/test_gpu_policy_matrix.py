"""The routing decision on the GPU: TDT blob or "UNCP" plus the raw bytes, for the cases of
tests/policy_cases.py — every term of the decision flipped alone, on either side of its edge, at the
tuned widths and at 3, 12 and 40, in every message class (and the 64-byte floor at width 32) — through
every route that restates the decision by hand.  Expected blobs are the CPU oracle's, computed once per module (pinned to the
reference's record by tests/test_policy_matrix.py); every comparison is bit-exact.

  A  compacted encode_batch: one pass and two phases (TDT_OPT_NO_TWO_PHASE 0 / 1; the generic widths know
     the two phases only), size hints 1024 / 65536
  B  slotted encode_into into caller-built slots of a canary-filled buffer (a message both copied and
     encoded, or a header in a raw slot, shows as a stray byte): TDT_OPT_LARGE_MIN at its default and
     at 65536, where every message above 64 KiB takes the tiles; generic widths also with
     TDT_OPT_ANY_TILED = 0.  No plan counter of the encode is public (TdtCodec.stat() names the decode's
     and the fallback counts only), so that the tiles are taken rests on the plan's rule, restated in
     `tiled_by_rule`: n > max(large_min, batch bytes / 4096) on a fresh context, whose budgets are not yet
     sized by a history.
  C  encode_v, every message in an allocation of its own
  D  one encode_vw call over widths 2, 4, 8, 16, 3, 12 in which the same n occurs at every width and
     routes differently (1032: TDT at 2, 4, 8, 12, raw at 16)
  E  encode_vp with TDT_OPT_PACK_SIZES_FIRST 0, 1, 2: offsets are the scan of the oracle's lengths
  F  encoded_sizes, encoded_sizes_v, mappings_v: the oracle's lengths; mapping word 0 for a raw case
  G  encode_v / encode_vp (mapbits=...): raw cases carry an invalid mapping word and come out as UNCP with
     status 0 ("UNCP first", include/psyne_tdt.h), TDT cases carry the oracle's mapping
  H  B and C with raw_fallback=True: a raw-by-policy message is n + 4 bytes and no fallback; the
     RAW_FALLBACKS stat is the number of TDT cases of the call whose oracle blob exceeds n + 4 (the ten
     cases whose frame alone does, policy_cases.frame_exceeds)
  I  encode_host with the whole batch, one message per call, tdt_encode_host_v; again with
     host_raw_fallback=True
  J  TdtCodec.should_transform and TDTCompressionProtocol.should_transform against the record's `st`:
     the reference's predicate holds no word-size guard, so on the `modws` cases it says yes where the
     blob is raw; HipTDTCompressionProtocol::should_transform on 16 equality rows (tests/cpp/test_policy_rows.cpp)
  K  a warm context, metrics on / off (bandwidth) / on / off (cpu) / on over one fixed batch: the
     history-sized grids go from "everything on the copy list" to "nothing on it" and back
  L  the blobs of B and C decoded back (decode_into, decode_v)

Contexts are fresh per (width, min_tensor_size, thresholds); cases that share one and differ in their
metrics run as separate calls on it.  The helpers return the names of the cases that differ, so that a
run against a deliberately wrong build can count them: profiles/policy_matrix/mutation.txt."""
import ctypes as C
import json

import numpy as np
import pytest

from oracle.oracle import Oracle, encode_bound
from tests import policy_cases as pc
from tests.golden_cases import GOLDEN
from tests.support import CANARY, offsets_of, phased_slots

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, i64, on_gpu  # noqa: E402, F401

pytestmark = pytest.mark.gpu

UNCP = b"PCNU"
LARGE_MIN = 65536
TILE_SHARE = 4096  # a message is tiled above max(large_min, batch bytes / 4096) (encode plan, tdt_encode.h)
VW_WIDTHS = (2, 4, 8, 16, 3, 12)
VW_MIN_TENSOR = 512
FLIP_WIDTHS = (4, 12)
FLIPS = ((10.0, 0.5), (1000.0, 0.5), (10.0, 0.5), (10.0, 0.9), (10.0, 0.5))  # on, off, on, off (cpu), on


def oracle_config(orc, ws, min_tensor, bt, ct):
    return orc.config(word_size=ws, sample_fraction=1.0, bandwidth_threshold_mbps=bt, cpu_usage_threshold=ct,
                      min_tensor_size=min_tensor)


def blob_bits(blob, ws) -> int:
    """The mapping word of a blob: bit p = the stream of byte position p; 0 for a raw one."""
    if blob[:4] == UNCP:
        return 0
    mp = np.frombuffer(blob[20:20 + 4 * ws], np.int32)
    return sum(int(m) << p for p, m in enumerate(mp))


class Item:
    """A message with its configuration and the oracle's blob."""

    def __init__(self, name, ws, n, key, metrics, message, blob):
        self.name, self.ws, self.n, self.key, self.metrics, self.message, self.blob = name, ws, n, key, metrics, message, blob
        self.raw = blob[:4] == UNCP
        self.bits = blob_bits(blob, ws)

    def want(self, fallback=False) -> bytes:
        if fallback and len(self.blob) > self.n + 4:
            return UNCP + self.message.tobytes()
        return self.blob


@pytest.fixture(scope="module")
def items():
    orc = Oracle()
    out = []
    for c in pc.all_cases():
        cfg = oracle_config(orc, c.ws, c.min_tensor, c.bandwidth_threshold, c.cpu_threshold)
        blob = orc.encode(c.message, cfg=cfg, bandwidth=c.bandwidth, cpu=c.cpu)
        assert (blob[:4] == UNCP) == (c.side == "off") and (c.side == "on" or len(blob) == c.n + 4), c.name
        out.append(Item(c.name, c.ws, c.n, pc.config_key(c), pc.metrics_key(c), c.message, blob))
    return out


@pytest.fixture(scope="module")
def record():
    return {r["name"]: r for r in json.loads((GOLDEN / "policy_matrix.json").read_text())["cases"]}


def of_width(items, ws):
    return [c for c in items if c.ws == ws]


def grouped(sub):
    """[(config key, [(metrics, items)])] in first-seen order."""
    out = {}
    for c in sub:
        out.setdefault(c.key, {}).setdefault(c.metrics, []).append(c)
    return [(k, list(v.items())) for k, v in out.items()]


def make_codec(key, options=(), **kw):
    from psyne_amd import TDTConfig, TdtCodec
    ws, mt, bt, ct = key
    c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws, bandwidth_threshold_mbps=bt, cpu_usage_threshold=ct,
                           min_tensor_size=mt), **kw)
    for opt, val in options:
        c.set_option(opt, val)
    return c


def over_groups(sub, call, options=(), hint=None, **kw):
    """call(codec, items of one configuration and one pair of metrics) -> names, over fresh contexts."""
    bad = []
    for key, batches in grouped(sub):
        codec = make_codec(key, options, **kw)
        if hint is not None:
            codec.set_size_hint(hint)
        for (bw, cpu), part in batches:
            codec.set_metrics(bw, 1.0, cpu)
            bad += call(codec, part)
        assert codec.error_flags() == 0
        codec.close()
    return bad


def differing(sub, blobs, lengths, statuses, fallback=False):
    """Names of the cases whose blob, length or status is not the oracle's."""
    return [c.name for c, b, n, s in zip(sub, blobs, lengths, statuses)
            if int(s) != 0 or int(n) != len(c.want(fallback)) or b != c.want(fallback)]


def tiled_by_rule(sub, large_min):
    total = sum(c.n for c in sub)
    return [c for c in sub if c.n > max(large_min, total // TILE_SHARE)]


class Own:
    """Every message in a device allocation of its own, made once per test."""

    def __init__(self):
        self.t = {}

    def __call__(self, c):
        if c.name not in self.t:
            self.t[c.name] = torch.from_numpy(np.array(c.message)).cuda()
        return self.t[c.name]


# ---------------------------------------------------------------------------------- the routes
def run_compacted(codec, sub):
    d, o = on_gpu([c.message for c in sub])
    enc, eoff, st = codec.encode_batch(d, o)
    torch.cuda.synchronize()
    e, eo, s = enc.cpu().numpy(), eoff.cpu().numpy(), st.cpu().numpy()
    assert eo[0] == 0
    return differing(sub, [e[eo[i]:eo[i + 1]].tobytes() for i in range(len(sub))], np.diff(eo), s)


def run_slotted(codec, sub, fallback=False, counts=None):
    """encode_into into caller-built slots of a canary-filled buffer, then decode_into of what it
    wrote: names whose slot (the gap behind it included), length or status differ, whose blob does not
    decode back, and "stray bytes" for a byte outside every slot."""
    n = len(sub)
    d, o = on_gpu([c.message for c in sub])
    slots, end = phased_slots([codec.encode_bound(c.n) for c in sub])
    out = torch.full((end,), CANARY, dtype=torch.uint8, device="cuda")
    ds = torch.from_numpy(slots).cuda()
    _, _, ln, st = codec.encode_into(d, o, slots=ds, out=out)
    torch.cuda.synchronize()
    got, ln_h, st_h = out.cpu().numpy(), ln.cpu().numpy()[:n], st.cpu().numpy()[:n]
    want = np.full(end, CANARY, np.uint8)
    for c, p in zip(sub, slots):
        b = c.want(fallback)
        want[p:p + len(b)] = np.frombuffer(b, np.uint8)
    bad = [c.name for i, c in enumerate(sub)
           if st_h[i] != 0 or ln_h[i] != len(c.want(fallback)) or not np.array_equal(got[slots[i]:slots[i + 1]], want[slots[i]:slots[i + 1]])]
    if not (np.array_equal(got[:slots[0]], want[:slots[0]]) and np.array_equal(got[slots[-1]:], want[slots[-1]:])):
        bad.append("stray bytes")
    if counts is not None:
        counts.append((codec.stat("RAW_FALLBACKS"), sum(1 for c in sub if len(c.blob) > c.n + 4)))
    if bad:
        return bad  # (what a wrong length or status would make of the decode is not this test's matter)
    back, bsl, bln, bst = codec.decode_into(out, ds, in_lengths=ln[:n])
    torch.cuda.synchronize()
    bh, bs, bl, bt = back.cpu().numpy(), bsl.cpu().numpy(), bln.cpu().numpy(), bst.cpu().numpy()
    return [c.name + " (decode)" for i, c in enumerate(sub)
            if bt[i] != 0 or bl[i] != c.n or bh[bs[i]:bs[i] + bl[i]].tobytes() != c.message.tobytes()]


GUARD = 32


def scattered_outs(caps):
    outs = [torch.full((cap + GUARD,), CANARY, dtype=torch.uint8, device="cuda") for cap in caps]
    return outs, i64(t.data_ptr() for t in outs)


def check_scattered(sub, outs, ln, st, fallback=False):
    ln, st = ln.cpu().numpy(), st.cpu().numpy()
    bad = []
    for i, (c, o) in enumerate(zip(sub, outs)):
        h = o.cpu().numpy()
        b = c.want(fallback)
        if st[i] != 0 or ln[i] != len(b) or h[:len(b)].tobytes() != b or not (h[len(b):] == CANARY).all():
            bad.append(c.name)
    return bad


def run_scattered(codec, sub, own, fallback=False, counts=None, mapped=False):
    n = len(sub)
    tensors = [own(c) for c in sub]
    caps = [codec.encode_bound(c.n) for c in sub]
    outs, optr = scattered_outs(caps)
    bits = i64(1 << c.ws if c.raw else c.bits for c in sub) if mapped else None  # (raw: a bit at the word size, invalid)
    ln, st = codec.encode_v(i64(t.data_ptr() for t in tensors), i64(c.n for c in sub), optr, i64(caps), mapbits=bits)
    torch.cuda.synchronize()
    bad = check_scattered(sub, outs, ln, st, fallback)
    if counts is not None:
        counts.append((codec.stat("RAW_FALLBACKS"), sum(1 for c in sub if len(c.blob) > c.n + 4)))
    if bad or mapped:
        return bad
    backs = [torch.full((c.n + GUARD,), CANARY, dtype=torch.uint8, device="cuda") for c in sub]
    bl, bs = codec.decode_v(optr, ln[:n], i64(t.data_ptr() for t in backs), i64(c.n for c in sub))
    torch.cuda.synchronize()
    bl, bs = bl.cpu().numpy(), bs.cpu().numpy()
    for i, (c, t) in enumerate(zip(sub, backs)):
        h = t.cpu().numpy()
        if bs[i] != 0 or bl[i] != c.n or h[:c.n].tobytes() != c.message.tobytes() or not (h[c.n:] == CANARY).all():
            bad.append(c.name + " (decode)")
    return bad


def run_packed(codec, sub, own, mapped=False):
    tensors = [own(c) for c in sub]
    want_off = offsets_of([c.blob for c in sub])
    total = int(want_off[-1])
    t = torch.full((64 + total + 64,), CANARY, dtype=torch.uint8, device="cuda")
    bits = i64(1 << c.ws if c.raw else c.bits for c in sub) if mapped else None
    off, st = codec.encode_vp(i64(x.data_ptr() for x in tensors), i64(c.n for c in sub), sum(c.n for c in sub),
                              t[64:64 + total], mapbits=bits)
    torch.cuda.synchronize()
    h, off, st = t.cpu().numpy(), off.cpu().numpy(), st.cpu().numpy()
    bad = [c.name for i, c in enumerate(sub)
           if st[i] != 0 or off[i] != want_off[i] or off[i + 1] != want_off[i + 1]
           or h[64 + want_off[i]:64 + want_off[i + 1]].tobytes() != c.blob]
    if not ((h[:64] == CANARY).all() and (h[64 + total:] == CANARY).all()):
        bad.append("stray bytes")
    return bad


def run_sizes(codec, sub, own):
    n = len(sub)
    want = [len(c.blob) for c in sub]
    d, o = on_gpu([c.message for c in sub])
    sz, st = codec.encoded_sizes(d, o)
    tensors = [own(c) for c in sub]
    ptrs, sizes = i64(t.data_ptr() for t in tensors), i64(c.n for c in sub)
    szv, stv = codec.encoded_sizes_v(ptrs, sizes)
    szm, bits, stm = codec.mappings_v(ptrs, sizes)
    torch.cuda.synchronize()
    sz, st, szv, stv, szm, bits, stm = (x.cpu().numpy() for x in (sz, st, szv, stv, szm, bits, stm))
    bits = bits.view(np.uint64)
    return [c.name for i, c in enumerate(sub)
            if st[i] or stv[i] or stm[i] or not (sz[i] == szv[i] == szm[i] == want[i]) or int(bits[i]) != c.bits]


def host_call(codec, sub, mode, fallback):
    """mode: "batch" (tdt_encode_host, the pipeline), "each" (one message per call) or "v"."""
    if mode == "each":
        blobs, lens, sts = [], [], []
        for c in sub:
            enc, eoff, st = codec.encode_host(c.message, np.array([0, c.n], np.uint64))
            blobs.append(enc.tobytes())
            lens.append(int(eoff[1]))
            sts.append(int(st[0]))
        return differing(sub, blobs, lens, sts, fallback)
    n = len(sub)
    cap = sum(codec.host_encode_bound(c.n) for c in sub)
    buf = np.full(GUARD + cap + GUARD, CANARY, np.uint8)
    ooff, st = np.zeros(n + 1, np.uint64), np.zeros(n, np.int32)
    if mode == "v":
        keep = [np.array(c.message) for c in sub]
        ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in keep])
        sz = np.array([c.n for c in sub], np.uint64)
        r = codec._lib.tdt_encode_host_v(codec._h, C.addressof(ptrs), sz.ctypes.data, n, buf.ctypes.data + GUARD, cap,
                                         ooff.ctypes.data, st.ctypes.data)
    else:
        data = np.concatenate([c.message for c in sub])
        off = offsets_of([c.message for c in sub]).astype(np.uint64)
        r = codec._lib.tdt_encode_host(codec._h, data.ctypes.data, off.ctypes.data, n, buf.ctypes.data + GUARD, cap,
                                       ooff.ctypes.data, st.ctypes.data)
    assert r == 0
    eo = ooff.astype(np.int64)
    bad = differing(sub, [buf[GUARD + eo[i]:GUARD + eo[i + 1]].tobytes() for i in range(n)], np.diff(eo), st, fallback)
    if not ((buf[:GUARD] == CANARY).all() and (buf[GUARD + cap:] == CANARY).all()):
        bad.append("stray bytes")
    return bad


# ---------------------------------------------------------------------------------- the tests
# (the compacted encode of a generic width always takes the two phases: TDT_OPT_NO_TWO_PHASE is an error there)
@pytest.mark.parametrize("hint", [1024, 65536])
@pytest.mark.parametrize("ws,two_phase_off", [(ws, off) for ws in pc.WIDTHS for off in ((0, 1) if ws in pc.TUNED else (0,))])
def test_a_compacted(items, ws, two_phase_off, hint):
    from psyne_amd._lib import TDT_OPT_NO_TWO_PHASE
    assert over_groups(of_width(items, ws), run_compacted, [(TDT_OPT_NO_TWO_PHASE, two_phase_off)], hint=hint) == []


def slotted_variants():
    from psyne_amd._lib import TDT_OPT_ANY_TILED, TDT_OPT_LARGE_MIN
    out = []
    for ws in pc.WIDTHS:
        out.append(pytest.param(ws, (), id="ws%d-default" % ws))
        out.append(pytest.param(ws, ((TDT_OPT_LARGE_MIN, LARGE_MIN),), id="ws%d-tiles_above_64k" % ws))
        if ws not in pc.TUNED:
            out.append(pytest.param(ws, ((TDT_OPT_LARGE_MIN, LARGE_MIN), (TDT_OPT_ANY_TILED, 0)), id="ws%d-one_workgroup" % ws))
    return out


def check_tiled_premise(sub, options):
    """With TDT_OPT_LARGE_MIN = 65536 every case of 96 KiB and more is above the plan's threshold in
    each of its batches, and each term has a raw and a TDT one among them."""
    if not options or "mt" not in pc.terms_of(sub[0].ws):  # (width 32 has the 64-byte cases alone)
        return
    claimed = []
    for _, batches in grouped(sub):
        for _, part in batches:
            assert sum(c.n for c in part) // TILE_SHARE < LARGE_MIN
            claimed += tiled_by_rule(part, LARGE_MIN)
    assert {c.name for c in sub if c.n >= 98304 - 64} <= {c.name for c in claimed}
    assert {(c.n, c.raw) for c in claimed} >= {(pc._legal_at_or_below(131072, pc.lcm4(sub[0].ws)), True),
                                               (pc._legal_at_or_below(262144, pc.lcm4(sub[0].ws)), False)}
    for term in pc.terms_of(sub[0].ws):
        if "tiled" in pc.classes_of(term):
            assert {c.raw for c in claimed if "_%s_" % term in c.name} == {True, False}, term


@pytest.mark.parametrize("ws,options", slotted_variants())
def test_b_slotted_and_decoded_back(items, ws, options):
    sub = of_width(items, ws)
    check_tiled_premise(sub, options)
    assert over_groups(sub, run_slotted, options) == []


@pytest.mark.parametrize("ws", pc.WIDTHS)
def test_c_scattered_and_decoded_back(items, ws):
    own = Own()
    assert over_groups(of_width(items, ws), lambda codec, part: run_scattered(codec, part, own)) == []


@pytest.fixture(scope="module")
def mixed_width_batch():
    """Route D's batch: every n at every width of VW_WIDTHS under one configuration (min_tensor_size
    512, default thresholds, metrics on), the widths interleaved message by message."""
    orc = Oracle()
    sizes = [b + d for b in (1024, 4096) for d in (0, 2, 3, 4, 8, 12, 16, 24, 48)]
    sizes += [b + d for b in (32768, 65536, 131072) for d in (0, 4, 8, 16)]
    out = []
    for n in sizes:
        for ws in VW_WIDTHS:
            msg = pc.buffer(ws)[:n]
            blob = orc.encode(msg, cfg=oracle_config(orc, ws, VW_MIN_TENSOR, 100.0, 0.8), bandwidth=10.0, cpu=0.5)
            out.append(Item("vw_ws%d_n%d" % (ws, n), ws, n, None, None, msg, blob))
            assert (not out[-1].raw) == pc.compresses(ws, n, VW_MIN_TENSOR, 10.0, 0.5, 100.0, 0.8)
            assert out[-1].raw or len(blob) < n + 4
    return out


def test_d_scattered_mixed_widths(mixed_width_batch):
    from psyne_amd._lib import TDT_OPT_LARGE_MIN
    sub = mixed_width_batch
    routes = {}
    for c in sub:
        routes.setdefault(c.n, {})[c.ws] = c.raw
    assert routes[1032] == {2: False, 4: False, 8: False, 16: True, 3: False, 12: False}
    assert sum(1 for r in routes.values() if len(set(r.values())) == 2) >= 20  # one n, both routes
    assert sum(c.n for c in sub) // TILE_SHARE < LARGE_MIN and {c.raw for c in sub if c.n > 131072} == {True, False}
    codec = make_codec((4, VW_MIN_TENSOR, 100.0, 0.8), [(TDT_OPT_LARGE_MIN, LARGE_MIN)])
    codec.set_metrics(10.0, 1.0, 0.5)
    own = Own()
    tensors = [own(c) for c in sub]
    caps = [encode_bound(c.n, c.ws) for c in sub]
    outs, optr = scattered_outs(caps)
    widths = torch.tensor([c.ws for c in sub], dtype=torch.int32, device="cuda")
    ln, st = codec.encode_vw(i64(t.data_ptr() for t in tensors), i64(c.n for c in sub), widths,
                             codec.width_mask(VW_WIDTHS), optr, i64(caps))
    torch.cuda.synchronize()
    assert check_scattered(sub, outs, ln, st) == []
    assert codec.error_flags() == 0


@pytest.mark.parametrize("sizes_first", [0, 1, 2])
@pytest.mark.parametrize("ws", pc.WIDTHS)
def test_e_packed(items, ws, sizes_first):
    from psyne_amd._lib import TDT_OPT_PACK_SIZES_FIRST
    own = Own()
    assert over_groups(of_width(items, ws), lambda codec, part: run_packed(codec, part, own),
                       [(TDT_OPT_PACK_SIZES_FIRST, sizes_first)]) == []


@pytest.mark.parametrize("ws", pc.WIDTHS)
def test_f_sizes_and_mappings(items, ws):
    own = Own()
    assert over_groups(of_width(items, ws), lambda codec, part: run_sizes(codec, part, own)) == []


@pytest.mark.parametrize("large_min", [None, LARGE_MIN], ids=["default", "tiles_above_64k"])
@pytest.mark.parametrize("ws", pc.TUNED + pc.GENERIC)
def test_g_known_mappings(items, ws, large_min):
    """tdt_encode_lmap_kernel and tdt_encode_lcopy_kernel meet every term at the tiled sizes."""
    from psyne_amd._lib import TDT_OPT_LARGE_MIN
    own = Own()
    sub = of_width(items, ws)
    assert any(c.raw and c.n > 131000 for c in sub) and any(not c.raw and c.n > 131000 for c in sub)
    options = [(TDT_OPT_LARGE_MIN, large_min)] if large_min else []
    assert over_groups(sub, lambda codec, part: run_scattered(codec, part, own, mapped=True), options) == []
    assert over_groups(sub, lambda codec, part: run_packed(codec, part, own, mapped=True), options) == []


@pytest.mark.parametrize("ws", pc.WIDTHS)
def test_h_raw_fallback(items, ws):
    from psyne_amd._lib import TDT_OPT_LARGE_MIN
    sub = of_width(items, ws)
    own = Own()
    for options in ((), ((TDT_OPT_LARGE_MIN, LARGE_MIN),)):
        counts = []
        assert over_groups(sub, lambda codec, part: run_slotted(codec, part, True, counts), options, raw_fallback=True) == []
        assert over_groups(sub, lambda codec, part: run_scattered(codec, part, own, True, counts), options,
                           raw_fallback=True) == []
        assert all(got == want for got, want in counts), counts
        # (the premise, on the CPU: only the frame makes a TDT blob of these cases longer than n + 4)
        assert sum(want for _, want in counts) == 2 * sum(1 for c in sub if not c.raw and 26 + 4 * c.ws > c.n + 4)


@pytest.mark.parametrize("fallback", [False, True], ids=["plain", "host_raw_fallback"])
@pytest.mark.parametrize("ws", pc.WIDTHS)
def test_i_host_routes(items, ws, fallback):
    sub = of_width(items, ws)
    for mode in ("batch", "each", "v"):
        assert over_groups(sub, lambda codec, part: host_call(codec, part, mode, fallback), host_raw_fallback=fallback) == [], mode


@pytest.mark.parametrize("ws", pc.WIDTHS)
def test_j_public_predicate(items, record, ws):
    from psyne_amd import TDTConfig, TDTCompressionProtocol
    bad = []
    sub = of_width(items, ws)
    for key, batches in grouped(sub):
        codec = make_codec(key)
        proto = None
        if ws == 4:
            proto = TDTCompressionProtocol(TDTConfig(sample_fraction=1.0, word_size=4, bandwidth_threshold_mbps=key[2],
                                                     cpu_usage_threshold=key[3], min_tensor_size=key[1]))
        for (bw, cpu), part in batches:
            codec.set_metrics(bw, 1.0, cpu)
            if proto:
                proto.update_network_metrics(bw, 1.0)
                proto.update_system_metrics(cpu)
            for c in part:
                want = bool(record[c.name]["st"])
                if codec.should_transform(c.n) != want or (proto and proto.should_transform(c.message, c.n) != want):
                    bad.append(c.name)
        codec.close()
        if proto:
            proto.codec.close()
    assert bad == []
    # the predicate and the route part on exactly the `modws` cases: yes, and raw all the same
    apart = {c.name for c in sub if bool(record[c.name]["st"]) != (not c.raw)}
    assert apart == {c.name for c in sub if "_modws_" in c.name and c.raw}


def test_j_cpp_drop_in_class():
    """HipTDTCompressionProtocol::should_transform on 16 rows of the record (tests/cpp/test_policy_rows.cpp,
    built by psyne_amd.build.build_tests)."""
    import pathlib
    import subprocess
    binary = pathlib.Path(__file__).resolve().parent / "cpp" / "test_policy_rows"
    assert binary.exists(), "tests/cpp/test_policy_rows not built (python -m psyne_amd.build)"
    p = subprocess.run([str(binary)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "cpp policy rows OK rows=16" in p.stdout, p.stdout + p.stderr


@pytest.fixture(scope="module")
def flip_batches():
    """Route K's batch per width: the sizes of every width's cases up to 64 KiB, their legal neighbours and two tiled
    messages, with the oracle's blobs (metrics on; off, every blob is the marker and the message)."""
    orc = Oracle()
    out = {}
    for ws in FLIP_WIDTHS:
        q = pc.lcm4(ws)
        near = {c.n for c in pc.all_cases() if 64 <= c.n <= 66000}  # (every width's sizes: legal neighbours and raw ones)
        sizes = sorted(near | {n // q * q + j * q for n in near for j in (-1, 0, 1, 2)})
        sizes += [131072 // q * q, 196608 // q * q]
        cfg = oracle_config(orc, ws, VW_MIN_TENSOR, 100.0, 0.8)
        sub = []
        for n in sizes:
            msg = pc.buffer(ws)[:n]
            sub.append(Item("flip_ws%d_n%d" % (ws, n), ws, n, None, None, msg, orc.encode(msg, cfg=cfg, bandwidth=10.0, cpu=0.5)))
        assert 120 <= len(sub) <= 320 and sum(not c.raw for c in sub) > 40
        assert {pc.message_class(c.n) for c in sub if not c.raw} >= {"small", "mid", "medium", "tiled"}
        out[ws] = sub
    return out


@pytest.mark.parametrize("route", ["slotted", "scattered"])
@pytest.mark.parametrize("ws", FLIP_WIDTHS)
def test_k_warm_context_flips(flip_batches, ws, route):
    from psyne_amd._lib import TDT_OPT_LARGE_MIN
    on = flip_batches[ws]
    assert sum(c.n for c in on) // TILE_SHARE < LARGE_MIN and sum(1 for c in tiled_by_rule(on, LARGE_MIN) if c.n > 131000) == 2
    off = [Item(c.name, c.ws, c.n, None, None, c.message, UNCP + c.message.tobytes()) for c in on]
    codec = make_codec((ws, VW_MIN_TENSOR, 100.0, 0.8), [(TDT_OPT_LARGE_MIN, LARGE_MIN)])
    own = Own()
    for call, (bw, cpu) in enumerate(FLIPS):
        codec.set_metrics(bw, 1.0, cpu)
        sub = on if (bw, cpu) == FLIPS[0] else off
        bad = run_slotted(codec, sub) if route == "slotted" else run_scattered(codec, sub, own)
        assert bad == [], "call %d (bandwidth %g, cpu %g)" % (call, bw, cpu)
    assert codec.error_flags() == 0
