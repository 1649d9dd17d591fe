"""The 512-lane resident encode instance at its edge sizes, on the speculated mapping [1,1,1,0]
(float tensors) and on other mappings in the same launch: slotted batches (tdt_encode_batch_into,
size hint 65536) byte for byte against the CPU oracle, with lengths and statuses, and every blob
decoded on the device back to its input.  Also the 255-cap and the capacity status on messages of
the speculated mapping, and a caller-supplied [1,1,1,0]."""
import struct

import numpy as np
import pytest

from tests.support import E_CAPACITY, gradient

torch = pytest.importorskip("torch")
from tests.gpu_support import orc  # noqa: E402, F401

pytestmark = pytest.mark.gpu

KIB = 1024
SPEC = (1, 1, 1, 0)
SIZES = (32 * KIB + 16, 64 * KIB - 16, 64 * KIB)


@pytest.fixture(scope="module")
def codec():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from psyne_amd import TDTConfig, TdtCodec, _lib
    _lib.load()
    c = TdtCodec(TDTConfig(sample_fraction=1.0))
    c.set_metrics(10.0, 1.0, 0.5)
    c.set_size_hint(65536)
    return c


def planes(rng, nbytes, random_positions):
    """Words whose byte positions in `random_positions` are uniform random, the others constant."""
    w = np.full((nbytes // 4, 4), 0x3C, np.uint8)
    for b in random_positions:
        w[:, b] = rng.integers(0, 256, nbytes // 4, dtype=np.uint8)
    return w.reshape(-1)


def mapping_of(blob):
    assert blob[:4] == struct.pack("<I", 0x54445444), "a TDT blob"
    return struct.unpack_from("<4I", blob, 20)


def pack(msgs):
    off = np.zeros(len(msgs) + 1, np.int64)
    off[1:] = np.cumsum([m.size for m in msgs])
    assert not np.any(off % 16), "every message 16-byte aligned"
    return np.concatenate(msgs), off


def check_slotted(codec, msgs, want):
    """Encode msgs into their slots; blobs, lengths and statuses against `want`; decode back."""
    buf, off = pack(msgs)
    d, o = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    out, slots, lens, st = codec.encode_into(d, o)
    torch.cuda.synchronize()
    e, sl, ln, s = out.cpu().numpy(), slots.cpu().numpy(), lens.cpu().numpy(), st.cpu().numpy()
    for i, w in enumerate(want):
        assert int(s[i]) == 0, i
        assert int(ln[i]) == len(w), i
        assert e[sl[i]:sl[i] + ln[i]].tobytes() == w, i
    back, dsl, dln, dst = codec.decode_into(out, slots, in_lengths=lens)
    torch.cuda.synchronize()
    assert int(dst[: len(msgs)].abs().sum()) == 0
    assert np.array_equal(dsl.cpu().numpy(), off)
    assert np.array_equal(dln.cpu().numpy()[: len(msgs)], np.diff(off))
    assert np.array_equal(back.cpu().numpy()[: buf.size], buf)


@pytest.fixture(scope="module")
def mixed(orc):
    """Messages of the speculated mapping interleaved with messages of other mappings, at every
    edge size; the oracle's blobs."""
    rng = np.random.default_rng(0x5EC0)
    others = [(0, 1), (0,), (3,), (1, 2, 3), ()]
    msgs = []
    for k, n in enumerate(SIZES * 2):
        msgs.append(gradient(rng, n).copy())
        msgs.append(planes(rng, n, others[k % len(others)]))
    return msgs, [orc.encode(m) for m in msgs]


def test_sizes_and_both_arms_in_one_launch(codec, mixed):
    msgs, want = mixed
    maps = [mapping_of(w) for w in want]
    # conditions on the inputs: the speculated mapping at every size, and at least three others
    assert all(maps[i] == SPEC for i in range(0, len(msgs), 2))
    assert {msgs[i].size for i in range(0, len(msgs), 2)} == set(SIZES)
    assert len(set(maps) - {SPEC}) >= 3, sorted(set(maps))
    check_slotted(codec, msgs, want)


@pytest.fixture(scope="module")
def capped(orc):
    """64 KiB gradient messages with zero stretches of 255, 256, 257 and 600 words: one inside
    wave 0's 8 KiB range, one across the boundary between waves 3 and 4."""
    rng = np.random.default_rng(0xCA9)
    msgs = []
    for stretch in (255, 256, 257, 600):
        m = gradient(rng, 64 * KIB).copy().view(np.uint32)
        m[300:300 + stretch] = 0
        b = 4 * (8 * KIB // 4)
        m[b - stretch // 2:b - stretch // 2 + stretch] = 0
        msgs.append(m.view(np.uint8))
    return msgs, [orc.encode(m) for m in msgs]


def test_cap_on_speculated_mapping(codec, capped):
    msgs, want = capped
    assert all(mapping_of(w) == SPEC for w in want)
    # the stretches do make capped runs: a (count 255, value 0) pair
    assert all(bytes([255, 0]) in w for w in want)
    check_slotted(codec, msgs, want)


def test_capacity_on_speculated_mapping(codec, orc):
    rng = np.random.default_rng(0xCAFE)
    msgs = [gradient(rng, 64 * KIB).copy() for _ in range(3)]
    want = [orc.encode(m) for m in msgs]
    assert all(mapping_of(w) == SPEC for w in want)
    buf, off = pack(msgs)
    bound = codec.encode_bound(64 * KIB)
    sizes = [bound, len(want[1]) - 2, bound]
    sl = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    d, o = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    out = torch.full((int(sl[-1]),), 0xA5, dtype=torch.uint8, device="cuda")
    out, _, lens, st = codec.encode_into(d, o, slots=torch.from_numpy(sl).cuda(), out=out)
    torch.cuda.synchronize()
    e, ln, s = out.cpu().numpy(), lens.cpu().numpy(), st.cpu().numpy()
    assert list(s[:3]) == [0, E_CAPACITY, 0]
    assert list(ln[:3]) == [len(want[0]), 0, len(want[2])]
    expect = np.full(int(sl[-1]), 0xA5, np.uint8)  # the short slot and the slack stay untouched
    for i in (0, 2):
        expect[sl[i]:sl[i] + len(want[i])] = np.frombuffer(want[i], np.uint8)
    assert np.array_equal(e, expect)


def test_caller_mapping_speculated(codec, orc):
    rng = np.random.default_rng(0x3A9)
    msgs = [gradient(rng, 64 * KIB).copy(), rng.integers(0, 256, 64 * KIB, dtype=np.uint8), gradient(rng, 64 * KIB).copy()]
    want = [orc.encode(m, mapping=SPEC) for m in msgs]
    assert all(mapping_of(w) == SPEC for w in want)
    buf, off = pack(msgs)
    d, o = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    mp = torch.tensor(SPEC * len(msgs), dtype=torch.int32, device="cuda")
    enc, eoff, st = codec.encode_batch(d, o, mapping=mp)
    torch.cuda.synchronize()
    e, eo = enc.cpu().numpy(), eoff.cpu().numpy()
    assert int(st[: len(msgs)].abs().sum()) == 0
    for i, w in enumerate(want):
        assert e[eo[i]:eo[i + 1]].tobytes() == w, i
    dec, doff, dst = codec.decode_batch(enc, eoff)
    torch.cuda.synchronize()
    assert int(dst[: len(msgs)].abs().sum()) == 0
    assert np.array_equal(dec.cpu().numpy()[: buf.size], buf)
