"""The raw fallback on the host path (TDT_OPT_HOST_RAW_FALLBACK): tdt_encode_host and tdt_encode_host_v —
the chunked pipeline, pageable and pinned, and the one-message path — store a message whose TDT blob
would be longer than n + 4 bytes as its UNCP blob and leave every other message's blob, length and
status as they are; with the option off the host calls write what they always wrote, whatever
TDT_OPT_RAW_FALLBACK says.  Expected bytes are tests/raw_fallback_cases.py's — the CPU oracle's blob,
or "UNCP" + the message where that is longer than n + 4 — and every comparison is bit-exact.  Outputs
are exactly as long as the host bound says, between 0xA5 guard bytes that must stay intact."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

from tests import raw_fallback_cases as rc
from tests.support import CANARY, E_CAPACITY

torch = pytest.importorskip("torch")
from tests.gpu_support import _gpu, orc  # noqa: E402, F401

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
CPP_BIN = ROOT / "tests" / "cpp" / "test_host_raw_fallback"
OPT_LARGE_MIN, OPT_RAW_FALLBACK, OPT_HOST_RAW_FALLBACK = 1, 10, 11
GUARD = 64


def make_codec(ws=4, host_raw=True, tiled=False):
    from psyne_amd import TDTConfig, TdtCodec
    c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws), host_raw_fallback=host_raw)
    c.set_metrics(10.0, 1.0, 0.5)
    if tiled:
        c.set_option(OPT_LARGE_MIN, rc.LARGE_MIN_TILED)
    assert c.host_raw_fallback == host_raw
    return c


@pytest.fixture(scope="module")
def cases(orc):
    """The fixture batches by (ws, n), made once and never changed."""
    made = {}

    def get(ws, n):
        if (ws, n) not in made:
            made[(ws, n)] = rc.batch(orc, ws, n, rc.seed_of(ws, n))
        return made[(ws, n)]
    return get


def falls(batch):
    return sum(1 for c in batch if c["falls"])


def offsets(batch):
    off = np.zeros(len(batch) + 1, np.uint64)
    off[1:] = np.cumsum([c["x"].size for c in batch])
    return off


class Pinned:
    """tdt_host_alloc memory, canary-filled."""

    def __init__(self, lib, nbytes):
        from psyne_amd._lib import check
        self.lib, self.p = lib, C.c_void_p()
        check(lib.tdt_host_alloc(max(nbytes, 1), C.byref(self.p)))
        self.a = np.ctypeslib.as_array(C.cast(self.p, C.POINTER(C.c_uint8)), shape=(max(nbytes, 1),))
        self.a[:] = CANARY

    def close(self):
        self.a = None
        self.lib.tdt_host_free(self.p)


def host_encode(codec, batch, pin_in=False, pin_out=False, v=False, cap=None):
    """One tdt_encode_host (or _v) call into exactly `cap` bytes (default: the host bound of the batch)
    between guards: (the call's status, the blobs, out_off, statuses).  The guards are checked here."""
    lib, n = codec._lib, len(batch)
    off = offsets(batch)
    data = np.concatenate([c["x"] for c in batch]) if n else np.zeros(0, np.uint8)
    if cap is None:
        cap = sum(codec.host_encode_bound(c["x"].size) for c in batch)
    pins = []
    try:
        if pin_in:
            pins.append(Pinned(lib, data.size))
            pins[-1].a[: data.size] = data
            src = pins[-1].a
        else:
            src = np.ascontiguousarray(data) if data.size else np.zeros(1, np.uint8)
        if pin_out:
            pins.append(Pinned(lib, GUARD + cap + GUARD))
            buf = pins[-1].a
        else:
            buf = np.full(GUARD + cap + GUARD, CANARY, np.uint8)
        ooff, st = np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.int32)
        if v:
            keep = [src[int(off[i]):int(off[i + 1])] if pin_in else np.array(c["x"]) for i, c in enumerate(batch)]
            ptrs = (C.c_void_p * n)(*[m.ctypes.data if m.size else src.ctypes.data for m in keep])
            sz = np.array([c["x"].size for c in batch], np.uint64)
            r = lib.tdt_encode_host_v(codec._h, C.addressof(ptrs), sz.ctypes.data, n, buf.ctypes.data + GUARD, cap,
                                      ooff.ctypes.data, st.ctypes.data)
        else:
            r = lib.tdt_encode_host(codec._h, src.ctypes.data, off.ctypes.data, n, buf.ctypes.data + GUARD, cap,
                                    ooff.ctypes.data, st.ctypes.data)
        assert (buf[:GUARD] == CANARY).all() and (buf[GUARD + cap:] == CANARY).all(), "guards"
        out = buf[GUARD:GUARD + cap].copy()
        blobs = [out[int(ooff[i]):int(ooff[i + 1])].tobytes() for i in range(n)]
        return r, blobs, ooff, st[:n]
    finally:
        for p in pins:
            p.close()


def check_result(codec, batch, res, want_key="want", what="", stat=None):
    """Blobs, statuses, offsets and the stat of one call; then the blobs decode back to the messages."""
    r, blobs, ooff, st = res
    assert r == 0, what
    want = [c[want_key] for c in batch]
    for k, c in enumerate(batch):
        assert int(st[k]) == 0, "%s %s" % (what, c["name"])
        assert blobs[k] == want[k], "%s %s" % (what, c["name"])
    pre = np.zeros(len(batch) + 1, np.uint64)
    pre[1:] = np.cumsum([len(w) for w in want])
    assert ooff.tolist() == pre.tolist(), what
    assert codec.stat("HOST_RAW_FALLBACKS") == (falls(batch) if stat is None else stat), what
    enc = np.frombuffer(b"".join(blobs), np.uint8)
    total = sum(c["x"].size for c in batch)
    dec, doff, dst = codec.decode_host(enc, pre, total)
    assert int(np.abs(dst).sum()) == 0 and doff.tolist() == offsets(batch).tolist(), what
    assert dec.tobytes() == b"".join(c["x"].tobytes() for c in batch), what
    assert codec.error_flags() == 0, what


# ------------------------------------------------------------------------------- 1: option, bound, stat
def test_option_bound_and_stat(cases):
    from psyne_amd import TDTConfig, TdtCodec
    batch = cases(4, 1024)
    for ws in (4, 12):
        c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws))
        for n in (0, 60, 1024):
            assert c.host_encode_bound(n) == max(n + 4, 28 + 4 * ws + 2 * n)
        c.set_option(OPT_HOST_RAW_FALLBACK, 1)
        assert c.host_raw_fallback and not c.raw_fallback
        for n in (0, 60, 1024):
            assert c.host_encode_bound(n) == n + 4
            assert c.encode_bound(n) == max(n + 4, 28 + 4 * ws + 2 * n)  # (option 10's bound is its own)
        assert c.stat("HOST_RAW_FALLBACKS") == 0
        c.set_option(OPT_HOST_RAW_FALLBACK, 0)
        assert not c.host_raw_fallback and c.host_encode_bound(1024) == 28 + 4 * ws + 2048
    # option 10 alone leaves the host calls as they are
    codec = make_codec(4, host_raw=False)
    codec.set_option(OPT_RAW_FALLBACK, 1)
    assert codec.raw_fallback and not codec.host_raw_fallback
    check_result(codec, batch, host_encode(codec, batch), want_key="plain", what="option 10 alone", stat=0)
    # on, off and on again on one context
    codec = make_codec(4)
    check_result(codec, batch, host_encode(codec, batch), what="on")
    codec.set_option(OPT_HOST_RAW_FALLBACK, 0)
    check_result(codec, batch, host_encode(codec, batch), want_key="plain", what="off", stat=0)
    codec.set_option(OPT_HOST_RAW_FALLBACK, 1)
    check_result(codec, batch, host_encode(codec, batch), what="on again")


def test_environment_sets_the_option(monkeypatch):
    from psyne_amd import TDTConfig, TdtCodec
    monkeypatch.setenv("PSYNE_TDT_HOST_RAW_FALLBACK", "1")
    c = TdtCodec(TDTConfig(sample_fraction=1.0))
    assert c.host_raw_fallback and not c.raw_fallback and c.host_encode_bound(1000) == 1004


# ------------------------------------------------------------------------------- 2: the pipeline, every class
PIPELINE = [(4, 1024), (4, 4100), (4, 32768), (4, 65540), (1, 1024), (2, 1024), (8, 65536), (16, 1024), (3, 1032),
            (12, 12288), (40, 1040)]


@pytest.mark.parametrize("ws,n", PIPELINE, ids=["ws%d-n%d" % c for c in PIPELINE])
def test_pipeline_every_class(cases, ws, n):
    batch = cases(ws, n)
    assert falls(batch) > 0
    if (ws, n) == (4, 32768):  # (the batch that takes the look-back route with the option off)
        sizes = [c["x"].size for c in batch]
        assert max(sizes) <= 65536 and sum(sizes) >= 16384 * len(sizes)
    codec = make_codec(ws)
    res = host_encode(codec, batch)
    assert sum(c["x"].size + 4 for c in batch) == sum(codec.host_encode_bound(c["x"].size) for c in batch)
    check_result(codec, batch, res)
    off_codec = make_codec(ws, host_raw=False)
    out, out_off, st = off_codec.encode_host(np.concatenate([c["x"] for c in batch]), offsets(batch))
    assert int(np.abs(st).sum()) == 0 and off_codec.stat("HOST_RAW_FALLBACKS") == 0
    for k, c in enumerate(batch):
        assert out[int(out_off[k]):int(out_off[k + 1])].tobytes() == c["plain"], c["name"]
    # and the Python wrapper sizes its own buffer by the host bound
    out, out_off, st = codec.encode_host(np.concatenate([c["x"] for c in batch]), offsets(batch))
    assert int(np.abs(st).sum()) == 0 and out.tobytes() == b"".join(c["want"] for c in batch)


# ------------------------------------------------------------------------------- 3: routes
ROUTES = {"pageable": {}, "pinned-in": dict(pin_in=True), "pinned-out": dict(pin_out=True), "v-pageable": dict(v=True),
          "v-pinned": dict(v=True, pin_in=True), "slot-streams": {}}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("n", [1024, 65540])
def test_routes(cases, monkeypatch, route, n):
    batch = cases(4, n)
    if route == "slot-streams":
        monkeypatch.setenv("PSYNE_TDT_SLOT_STREAMS", "1")
    codec = make_codec(4)
    check_result(codec, batch, host_encode(codec, batch, **ROUTES[route]), what=route)
    if route in ("pinned-out", "v-pinned"):  # both ends pinned: DMA in, the direct gather out
        check_result(codec, batch, host_encode(codec, batch, pin_in=True, pin_out=True, v=route[0] == "v"), what=route + " both")


# ------------------------------------------------------------------------------- 4: more chunks than slots
def test_more_chunks_than_slots(cases):
    batch = cases(4, 65536) * 24
    total = sum(c["x"].size for c in batch)
    # an eighth of the call is under 2 MiB, so chunks hold at most 2 MiB of whole messages: at least 6 over the 4 slots
    assert total // 8 < (2 << 20) and -(-total // (2 << 20)) >= 6
    codec = make_codec(4)
    check_result(codec, batch, host_encode(codec, batch), what="pageable")
    check_result(codec, batch, host_encode(codec, batch, pin_in=True, pin_out=True), what="pinned")


# ------------------------------------------------------------------------------- 5: tiles
@pytest.mark.parametrize("ws,n", [(4, 196640), (12, 196608)])
def test_tiles(cases, ws, n):
    batch = cases(ws, n)
    codec = make_codec(ws, tiled=True)
    check_result(codec, batch, host_encode(codec, batch), what="tiled")


# ------------------------------------------------------------------------------- 6: one message per call
ONE = [(4, n) for n in rc.TUNED_SIZES[4]] + [(2, 1024), (8, 65536)]


@pytest.mark.parametrize("ws,n", ONE, ids=["ws%d-n%d" % c for c in ONE])
def test_one_message_per_call(cases, monkeypatch, ws, n):
    batch = cases(ws, n)
    codec = make_codec(ws)
    monkeypatch.setenv("PSYNE_TDT_NO_ONE", "1")
    pipe = make_codec(ws)  # the same call through the pipeline
    for c in batch:
        one = host_encode(codec, [c])
        check_result(codec, [c], one, what="one")
        assert codec.stat("HOST_RAW_FALLBACKS") == int(c["falls"])
        res = host_encode(pipe, [c])
        check_result(pipe, [c], res, what="pipeline")
        assert res[1] == one[1]


def test_one_message_without_spin_and_over_the_limit(cases, orc, monkeypatch):
    monkeypatch.setenv("PSYNE_TDT_ONE_SPIN", "0")
    codec = make_codec(4)
    for c in cases(4, 1024):
        check_result(codec, [c], host_encode(codec, [c]), what="no spin")
    # over the one-message limit (256 KiB): the pipeline serves the call
    x = rc.dense(262160, 77)
    want, plain = rc.expected_blob(orc, x, 4)
    assert want == rc.UNCP + x.tobytes() and len(plain) > x.size + 4
    big = dict(name="dense/262160", x=x, want=want, plain=plain, falls=True)
    check_result(codec, [big], host_encode(codec, [big]), what="over the limit")


# ------------------------------------------------------------------------------- 7: capacity
@pytest.mark.parametrize("pin_out", [False, True], ids=["pageable", "pinned"])
def test_capacity(cases, pin_out):
    batch = cases(4, 1024) + cases(4, 65540)
    exact = sum(len(c["want"]) for c in batch)
    assert exact < sum(c["x"].size + 4 for c in batch)
    codec = make_codec(4)
    check_result(codec, batch, host_encode(codec, batch, pin_out=pin_out, cap=exact), what="exact")
    r, _, ooff, _ = host_encode(codec, batch, pin_out=pin_out, cap=exact - 1)  # (the guards behind out_cap: checked there)
    assert r == E_CAPACITY
    # one message per call: n + 3 bytes do not hold a falling message, n + 4 do
    c = next(c for c in batch if c["kind"] == "dense")
    r, _, ooff, _ = host_encode(codec, [c], pin_out=pin_out, cap=c["x"].size + 3)
    assert r == E_CAPACITY and int(ooff[1]) == 0
    check_result(codec, [c], host_encode(codec, [c], pin_out=pin_out, cap=c["x"].size + 4), what="one exact")


# ------------------------------------------------------------------------------- 8: the public layers
def test_python_protocol(cases):
    from psyne_amd import TDTConfig
    from psyne_amd.tdt import TDTCompressionProtocol
    batch = cases(4, 65536)
    g = next(c for c in batch if c["kind"] == "grad70")
    d = next(c for c in batch if c["kind"] == "dense")
    on = TDTCompressionProtocol(TDTConfig(sample_fraction=1.0), host_raw_fallback=True)
    off = TDTCompressionProtocol(TDTConfig(sample_fraction=1.0))
    for p in (on, off):
        p.update_network_metrics(10.0, 1.0)
    assert on.encode(g["x"].tobytes()) == off.encode(g["x"].tobytes()) == g["plain"]
    ratio, t = on.transformation_ratio(), on.last_encode_time_ms_
    blob = on.encode(d["x"].tobytes())
    assert blob == rc.UNCP + d["x"].tobytes() and off.encode(d["x"].tobytes()) == d["plain"]
    assert on.transformation_ratio() == ratio and on.last_encode_time_ms_ == t
    assert on.decode(blob) == d["x"].tobytes()


def test_cpp_layers():
    if not CPP_BIN.exists():
        pytest.skip("tests/cpp/test_host_raw_fallback not built (python -m psyne_amd.build)")
    p = subprocess.run([str(CPP_BIN)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "cpp host raw fallback OK" in p.stdout, p.stdout + p.stderr
