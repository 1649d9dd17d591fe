"""The tiled form of encode-narrow (psyne_amd/csrc/tdt_enc_narrow_tiled.h): tensors of tdt_encode_narrow_v
above TDT_OPT_LARGE_MIN encoded as tiles of TDT_NARROW_TILE_ELEMS elements, one workgroup per tile.  The
reference is tests/test_gpu_enc_narrow.py's: the numpy `narrow`, then the oracle's width-2 encode.  Blob,
length and status are compared byte for byte; `run` checks the canaries, that a refused blob is untouched,
and the round trip through decode_v."""
import numpy as np
import pytest

from tests.support import E_CAPACITY
from tests.test_gpu_enc_narrow import CODES, E_ARG, E_ELEMENT, UNCP, bound, family, narrow, run, want, widen

torch = pytest.importorskip("torch")
from psyne_amd._lib import (TDT_NARROW_TILE_ELEMS as R, TDT_OPT_LARGE_MIN, TDT_OPT_NARROW_TILED,  # noqa: E402
                            TDT_OPT_RAW_FALLBACK, TDT_OPT_TILE_CAP)
from tests.gpu_support import _gpu, make_codec, orc  # noqa: E402, F401

pytestmark = pytest.mark.gpu

OPTS = ((TDT_OPT_LARGE_MIN, 4 * R),)  # 65,536 source bytes: a tensor of more than R elements tiles
HOW = {"tiled": (), "option_0": ((TDT_OPT_NARROW_TILED, 0),), "tile_cap_1": ((TDT_OPT_TILE_CAP, 1),)}
FAMILIES = ("gradient", "lowconst", "zeros", "repeated", "dense")
_lists = {}


def sized_list(orc, t, raw):
    """(cases, sources, expected blobs) of test 1, built once per type and raw setting."""
    if (t, raw) not in _lists:
        rng = np.random.default_rng(3101)
        cases = [(f, n) for n in (R + 2, 2 * R, 2 * R + 18, 3 * R - 2) for f in FAMILIES]
        srcs = [family(rng, f, n, t) for f, n in cases]
        _lists[t, raw] = cases, srcs, [want(orc, narrow(u, t).tobytes(), raw) for u in srcs]
    return _lists[t, raw]


@pytest.mark.parametrize("how", list(HOW))
@pytest.mark.parametrize("raw", [False, True], ids=["tdt", "rawfb"])
@pytest.mark.parametrize("t", list(CODES))
def test_sizes_families_alignments(orc, t, raw, how):
    """Every size and family (all three mappings, a final run that spans every tile, dense data that falls back),
    the source 0 / 4 / 8 / 12 bytes and the blob 0 .. 3 bytes off a boundary, twice on one codec: the second call
    finds the workspace warm and the bins zeroed again.  Every tensor has two tiles or more, so a budget of one
    tile holds none of them."""
    cases, srcs, blobs = sized_list(orc, t, raw)
    leads = [4 * (i % 4) for i in range(len(cases))]
    bleads = [(i // 4) % 4 for i in range(len(cases))]
    codec = make_codec(ws=4, options=OPTS + HOW[how] + (((TDT_OPT_RAW_FALLBACK, 1),) if raw else ()))
    for _ in range(2):
        res = run(codec, srcs, [CODES[t]] * len(cases), leads, bleads)
        for (f, n), exp, (blob, ln, st) in zip(cases, blobs, res):
            assert (st, ln) == (0, len(blob)) and blob == exp, (f, n)
            if f in ("zeros", "dense"):
                assert (blob[:4] == UNCP) == (raw and f == "dense"), (f, n)
    tiled = how == "tiled"
    assert codec.stat("NARROW_LARGE") == (len(cases) if tiled else 0)
    assert codec.stat("NARROW_TILES") == (sum(-(-n // R) for _, n in cases) if tiled else 0)


LENGTHS = (254, 255, 256, 510, 765, 5000, R + 300)


def placed(L, T, N):
    """Where a run of L stream bytes goes in a stream of N bytes whose tiles hold T: ending at the first tile
    edge, starting at it, straddling it, straddling the second from a lane's middle, ending with the stream."""
    at = (T - L, T, T - L // 2, (2 * T - L // 2) // 16 * 16 + 5, N - L)
    return [p for p in at if p >= 0]


@pytest.mark.parametrize("stream", ["plane0", "plane1", "interleaved"])
def test_runs_at_tile_edges(orc, stream):
    """One run per tensor in otherwise run-free data of 4 R elements.  A run of R + 300 that ends with the stream
    leaves the last tile without a run start."""
    rng = np.random.default_rng(3102)
    n, srcs = 4 * R, []
    for L in LENGTHS:
        if stream == "interleaved":  # mapping [0,0]: the stream is the message, lo at 2 i and hi at 2 i + 1
            for p in placed(L, 2 * R, 2 * n):
                st = np.tile(np.array([0x7B, 0x3C], np.int64), n)
                st[p:p + L] = 0
                # an odd run (the one of 255 that ends at the tile edge starts at an odd position) leaves one
                # plane a zero short: one lone zero there keeps the planes' counts, and with them the entropies, equal
                if L % 2:
                    st[2 * (R + 6000) + (p + L) % 2] = 0
                assert (st[0::2] == 0).sum() == (st[1::2] == 0).sum()
                srcs.append(widen((st[0::2] | (st[1::2] << 8)).astype(np.uint16), "bf16"))
        else:  # (no two equal neighbours in either plane: tests/test_gpu_enc_narrow.py's construction)
            plane = int(stream[-1])
            for p in placed(L, R, n):
                pl = [rng.integers(0, 254, n), 0x3C + (np.arange(n) & 1)]
                pl[0] = np.where(pl[0] == np.roll(pl[0], 1), pl[0] ^ 1, pl[0])
                pl[plane][p:p + L] = 0x7E
                srcs.append(widen((pl[0] | (pl[1] << 8)).astype(np.uint16), "bf16"))
    k = len(srcs)
    res = run(make_codec(options=OPTS), srcs, [0x13] * k, leads=[4 * (i % 4) for i in range(k)], bleads=[i % 4 for i in range(k)])
    for i, (u, (blob, ln, st)) in enumerate(zip(srcs, res)):
        assert (st, blob) == (0, want(orc, narrow(u, "bf16").tobytes())), i
        assert int.from_bytes(blob[8:12], "little") == (1 if stream == "interleaved" else 2), i  # the stream count
    assert k == 5 * len(LENGTHS) - (stream != "interleaved")  # (a plane's run of R + 300 cannot end at the first tile edge)


def test_statuses_and_routing_in_one_mixed_list(orc):
    rng = np.random.default_rng(3103)
    n = 2 * R + 18
    g = family(rng, "gradient", n, "bf16").view(np.uint8)
    short = family(rng, "gradient", 2048, "bf16").view(np.uint8)
    small = family(rng, "gradient", 100, "f16").view(np.uint8)  # (UNCP by the 1,024-byte floor)
    gb, gf = (want(orc, narrow(g.view(np.uint32), t).tobytes()) for t in ("bf16", "f16"))
    sb = want(orc, narrow(short.view(np.uint32), "bf16").tobytes())
    #        short      long exact  UNCP short  long - 1    long lead 2  short      long bad code  long fp16  UNCP exact
    srcs = [short,      g,          small,      g,          g,           short,     g,             g,         small]
    codes = [0x13,      0x13,       0x12,       0x13,       0x13,        0x13,      0x31,          0x12,      0x12]
    leads = [0,         4,          0,          8,          2,           12,        0,             12,        4]
    caps = [len(sb),    len(gb),    203,        len(gb) - 1, bound(2 * n), len(sb) - 1, bound(2 * n), len(gf), 204]
    stats = [0,         0,          E_CAPACITY, E_CAPACITY, E_ELEMENT,   E_CAPACITY, E_ARG,        0,         0]
    codec = make_codec(options=OPTS)
    res = run(codec, srcs, codes, leads, [i % 4 for i in range(9)], caps)
    assert [r[2] for r in res] == stats
    for i, (blob, ln, st) in enumerate(res):  # (run() found the refused blobs' bytes untouched: nothing behind length 0)
        assert ln == (0 if st else caps[i]), i
    assert (res[0][0], res[1][0], res[7][0]) == (sb, gb, gf)
    assert res[8][0] == UNCP + narrow(small.view(np.uint32), "f16").tobytes()
    assert codec.stat("NARROW_LARGE") == 3 and codec.stat("NARROW_TILES") == 9  # the aligned long ones with a code
    # the policy off: the long tensors' tiles copy the narrowed bytes
    codec = make_codec(bandwidth=1000.0, options=OPTS)
    res = run(codec, [g, short, g], [0x13] * 3, [0, 4, 8], [1, 2, 3], [2 * n + 4, 4100, 2 * n + 3])
    assert [(ln, st) for _, ln, st in res] == [(2 * n + 4, 0), (4100, 0), (0, E_CAPACITY)]
    assert res[0][0] == UNCP + narrow(g.view(np.uint32), "bf16").tobytes()
    assert codec.stat("NARROW_LARGE") == 2
