"""The SIZES x WIDTHS batch of the mixed-width, packed, sizes-first and known-mapping GPU tests: every
size class at every width, the oracle's blobs, and what encode_v on a context of each width gives.
A test module imports the `batch` fixture by name, with `orc` and `_gpu` of tests/gpu_support.py.  The
tables and `records` need no torch: what runs on the GPU imports it when called.

The module is no test module, so pytest does not rewrite its asserts: each carries its message."""
import numpy as np
import pytest

from oracle.oracle import encode_bound
from tests.anyws_cases import from_streams, low_pattern
from tests.support import address_order, mask_of

WIDTHS = [1, 2, 4, 8, 16, 3, 12]
# the smallest sizes that reach the UNCP copy (0, 3, 64, 1000: below min_tensor), the one-wave
# (<= 4 KiB), 256-lane (<= 32 KiB), resident 512-lane (<= 64 KiB, aligned) and streaming classes and,
# in so small a batch, the tiles (> 256 KiB).  4104, 32784, 65544 and 100008 are multiples of 12;
# 4104 is no multiple of 16 (the per-message n % ws fallback)
SIZES = [0, 3, 64, 1000, 1024, 4096, 4104, 4112, 32768, 32784, 65536, 65544, 65552, 100000, 100008, 262208]
LEADS = {4112: 1, 32784: 4, 65552: 8, 100000: 15}  # views this many bytes into their allocation


def records(rng, ws, n):
    """n bytes of ws-byte records whose byte positions differ in entropy (both streams populated
    from width 2 up); sizes that hold no whole number of records, and width 1, get few-valued bytes."""
    if ws > 1 and n >= ws and n % ws == 0:
        wc = n // ws
        return from_streams(ws, wc, low_pattern(wc * ws, rng), rng)
    return rng.integers(0, 4, n, dtype=np.uint8)


def oracle_blob(orc, m, w):
    return orc.encode(m, cfg=orc.config(sample_fraction=1.0, word_size=w))


def encode_v_sub(ws, tensors, caps):
    """encode_v on a context of width ws: (blobs as bytes, lengths, statuses)."""
    import torch
    from tests.gpu_support import i64, make_codec, ptrs
    outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    codec = make_codec(ws)
    ln, st = codec.encode_v(ptrs(tensors), i64(t.numel() for t in tensors), ptrs(outs), i64(caps))
    torch.cuda.synchronize()
    ln, st = ln.cpu().numpy()[: len(tensors)], st.cpu().numpy()[: len(tensors)]
    assert codec.error_flags() == 0, "encode_v at width %d: error flags %#x" % (ws, codec.error_flags())
    return [o[: ln[k]].cpu().numpy().tobytes() for k, o in enumerate(outs)], ln, st


@pytest.fixture(scope="module")
def batch(orc):
    """Every size at every width, the widths interleaved message by message; the oracle's blobs; and
    per width what encode_v on a context of that width gives for the width's sub-batch."""
    from tests.gpu_support import own
    rng = np.random.default_rng(20261)
    ws, msgs, leads = [], [], []
    for k, n in enumerate(SIZES):
        for j, w in enumerate(WIDTHS):
            ws.append(w)
            msgs.append(records(rng, w, n))
            leads.append(LEADS.get(n, 0) if (j + k) % 2 == 0 else 0)
    ws += [2, 8]
    msgs += [np.full(32768, 0x3C, np.uint8), rng.integers(0, 256, 65536, dtype=np.uint8)]  # constant, uniform random
    leads += [0, 0]
    blobs = [oracle_blob(orc, m, w) for m, w in zip(msgs, ws)]
    tensors = [own(m, lead) for m, lead in zip(msgs, leads)]
    caps = [encode_bound(len(m), w) for m, w in zip(msgs, ws)]
    sub = {}
    for w in WIDTHS:
        idx = [i for i, x in enumerate(ws) if x == w]
        b, ln, st = encode_v_sub(w, [tensors[i] for i in idx], [caps[i] for i in idx])
        for k, i in enumerate(idx):
            sub[i] = (b[k], int(ln[k]), int(st[k]))
    return dict(ws=ws, msgs=msgs, blobs=blobs, tensors=tensors, caps=caps, sub=sub, runs={})


def run_vw(batch, order):
    """One encode_vw call over the whole batch in the given address order (kept for the round trip)."""
    import torch
    from tests.gpu_support import i32, i64, make_codec, ptrs
    if order not in batch["runs"]:
        idx = address_order(batch["tensors"], order)
        tensors = [batch["tensors"][i] for i in idx]
        caps = [batch["caps"][i] for i in idx]
        outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
        codec = make_codec(4)
        ln, st = codec.encode_vw(ptrs(tensors), i64(t.numel() for t in tensors), i32(batch["ws"][i] for i in idx),
                                 mask_of(WIDTHS), ptrs(outs), i64(caps))
        torch.cuda.synchronize()
        flags = codec.error_flags()
        batch["runs"][order] = (idx, outs, ln.cpu().numpy(), st.cpu().numpy(), flags)
    return batch["runs"][order]
