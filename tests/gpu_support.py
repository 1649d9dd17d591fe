"""What the GPU test modules share: the module fixtures that require a GPU and load the library, the
oracle, device tensors of the C ABI's table types, guarded allocations and the plain codec.  A test
module imports the fixtures by name (pytest finds fixtures in the importing module's namespace), after
its own `torch = pytest.importorskip("torch")` line.

The module is no test module, so pytest does not rewrite its asserts: each carries its message."""
import numpy as np
import pytest
import torch

from oracle.oracle import Oracle
from tests.support import CANARY, offsets_of


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from psyne_amd import _lib
    _lib.load()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def make_codec(ws=4, hint=None, options=(), bandwidth=10.0):
    from psyne_amd import TDTConfig, TdtCodec
    c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws))
    c.set_metrics(bandwidth, 1.0, 0.5)  # bandwidth < 100 Mbps: compression on
    if hint is not None:
        c.set_size_hint(hint)
    for opt, value in options:
        c.set_option(opt, value)
    return c


def i64(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64, device="cuda")


def i32(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device="cuda")


def u64(values):
    """Mapping words as the int64 tensor the calls take (bit 63 is the sign there)."""
    return torch.from_numpy(np.array([int(v) for v in values], dtype=np.uint64).view(np.int64)).cuda()


def ptrs(tensors):
    return i64(t.data_ptr() if t.numel() else 0 for t in tensors)


def own(data, lead=0):
    """`data` in a device allocation of its own, `lead` bytes into it."""
    data = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    t = torch.empty(lead + data.size + 16, dtype=torch.uint8, device="cuda")
    v = t[lead:lead + data.size]
    if data.size:
        v.copy_(torch.from_numpy(np.ascontiguousarray(data)))
    return v


def guarded(cap, lead=0):
    """A `cap`-byte output `lead` bytes off a 64-byte boundary, 64 canary bytes before the boundary
    and 64 behind the output."""
    t = torch.full((64 + lead + cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    return t, t[64 + lead:64 + lead + cap]


def canaries_intact(t, cap):
    h = t.cpu().numpy()
    return bool((h[:64] == CANARY).all() and (h[64 + cap:] == CANARY).all())


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a writable copy: some inputs are views of bytes)


def on_gpu(msgs):
    return torch.from_numpy(np.concatenate(msgs)).cuda(), torch.from_numpy(offsets_of(msgs)).cuda()


def packed_blobs(out, off):
    oh, off = out.cpu().numpy(), off.cpu().numpy()
    return [oh[off[k]:off[k + 1]].tobytes() for k in range(off.size - 1)], off


def at_phase(buf: np.ndarray, phase: int, pad: int = 64):
    """buf on the GPU at `phase` bytes past a 256-byte aligned address, with a guard after it."""
    t = torch.full((phase + buf.size + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    v = t[phase:phase + max(buf.size, 1)]
    if buf.size:
        v[:buf.size] = torch.from_numpy(np.array(buf, dtype=np.uint8)).cuda()  # (a writable copy)
    return t, v


def encode_slotted(codec, msgs, pi=0, po=0, slots=None):
    """(blobs, statuses, lengths) of a slotted encode with input / output at byte phases pi / po."""
    data = np.concatenate([np.asarray(m, np.uint8) for m in msgs]) if msgs else np.zeros(0, np.uint8)
    off = torch.from_numpy(offsets_of(msgs)).cuda()
    _, d = at_phase(data, pi)
    sl = codec.encode_slots(off) if slots is None else torch.from_numpy(np.asarray(slots, np.int64)).cuda()
    total = int(sl[-1].item())
    raw = torch.full((po + total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out, _, lens, st = codec.encode_into(d, off, slots=sl, out=raw[po:po + max(total, 1)])
    torch.cuda.synchronize()
    assert int((raw[:po] != 0xA5).sum()) == 0 and int((raw[po + total:] != 0xA5).sum()) == 0, \
        "wrote outside its %d bytes" % total
    o, s, l, t = out.cpu().numpy(), sl.cpu().numpy(), lens.cpu().numpy(), st.cpu().numpy()
    return [o[s[i]:s[i] + l[i]].tobytes() for i in range(len(msgs))], list(t[:len(msgs)]), list(l[:len(msgs)])


def decode_slotted(codec, blobs, pi=0, po=0, slots=None):
    data = np.frombuffer(b"".join(blobs), np.uint8)
    off = torch.from_numpy(offsets_of(blobs)).cuda()
    _, d = at_phase(data, pi)
    sl = codec.decode_slots(d, off) if slots is None else torch.from_numpy(np.asarray(slots, np.int64)).cuda()
    total = int(sl[-1].item())
    raw = torch.full((po + total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out, _, lens, st = codec.decode_into(d, off, slots=sl, out=raw[po:po + max(total, 1)])
    torch.cuda.synchronize()
    assert int((raw[:po] != 0xA5).sum()) == 0 and int((raw[po + total:] != 0xA5).sum()) == 0, \
        "wrote outside its %d bytes" % total
    o, s, l, t = out.cpu().numpy(), sl.cpu().numpy(), lens.cpu().numpy(), st.cpu().numpy()
    return [o[s[i]:s[i] + l[i]].tobytes() for i in range(len(blobs))], list(t[:len(blobs)]), list(l[:len(blobs)])
