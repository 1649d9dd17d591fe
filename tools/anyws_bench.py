"""Rates of the generic-word-size kernels (psyne_amd/csrc/tdt_anyws.hip): slotted encode and decode
of N x BYTES-byte messages at word size WS, timed with device events, beside the reference codec
on the same batch on up to 16 host threads (oracle/_ref, when built) and the PCIe ceiling the
README records.  Messages are of the constructed kind of tests/golden/make_anyws.py: positions
b % 3 == 0 uniform random, the others runs (up to 765 long, then a two-value pattern of period 300).

Usage: python tools/anyws_bench.py [--msgs 4096] [--bytes 49152] [--ws 12] [--steps 10] [--out FILE]
Prints one JSON line (and appends it to --out)."""
import argparse
import json
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PCIE_GBPS = 48.5  # README: pinned copies, each way


def messages(n_msgs, nbytes, ws, seed=12):
    rng = np.random.default_rng(seed)
    wc = nbytes // ws
    mp = [1 if b % 3 == 0 else 0 for b in range(ws)]
    lo = [b for b in range(ws) if not mp[b]]
    hi = [b for b in range(ws) if mp[b]]
    runs = (254, 255, 256, 509, 510, 511, 1, 765, 1)
    out = np.empty((n_msgs, wc, ws), np.uint8)
    out[:, :, hi] = rng.integers(0, 256, (n_msgs, wc, len(hi)), dtype=np.uint8)
    L = wc * len(lo)
    for i in range(n_msgs):
        vals = rng.permutation(200)[: len(runs) + 2] + 1
        s = np.concatenate([np.full(r, vals[k], np.uint8) for k, r in enumerate(runs)])
        period = np.concatenate([np.full(200, vals[-2], np.uint8), np.full(100, vals[-1], np.uint8)])
        s = np.concatenate([s] + [period] * ((max(L - s.size, 0) + 299) // 300))[:L]
        out[i][:, lo] = s.reshape(wc, len(lo))
    return out.reshape(n_msgs, wc * ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=4096)
    ap.add_argument("--bytes", type=int, default=49152)
    ap.add_argument("--ws", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec
    m = messages(a.msgs, a.bytes, a.ws)
    nbytes = m.shape[1]
    data_h = m.reshape(-1)
    off_h = np.arange(a.msgs + 1, dtype=np.int64) * nbytes
    codec = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=a.ws))
    codec.set_metrics(10.0, 1.0, 0.5)
    data, off = torch.from_numpy(data_h).cuda(), torch.from_numpy(off_h).cuda()
    slots = codec.encode_slots(off)
    out = torch.empty(int(slots[-1].item()), dtype=torch.uint8, device="cuda")
    lens = torch.empty(a.msgs, dtype=torch.int64, device="cuda")
    st = torch.empty(a.msgs, dtype=torch.int32, device="cuda")
    back = torch.empty_like(data)
    blens = torch.empty_like(lens)
    dst = torch.empty_like(st)

    def enc():
        codec.encode_into(data, off, slots=slots, out=out, lengths=lens, status=st)

    def dec():
        codec.decode_into(out, slots, in_lengths=lens, slots=off, out=back, lengths=blens, status=dst)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    enc_ms = timed(enc)
    dec_ms = timed(dec)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0 and int(dst.abs().sum()) == 0 and torch.equal(back, data)
    assert codec.error_flags() == 0
    total = data_h.size
    res = dict(tool="anyws_bench", ws=a.ws, msgs=a.msgs, msg_bytes=nbytes, input_bytes=total,
               encoded_bytes=int(lens.sum().item()),
               encode_ms=dict(min=min(enc_ms), median=float(np.median(enc_ms))),
               decode_ms=dict(min=min(dec_ms), median=float(np.median(dec_ms))),
               encode_GBps=total / (float(np.median(enc_ms)) * 1e6), decode_GBps=total / (float(np.median(dec_ms)) * 1e6),
               pcie_ceiling_GBps=PCIE_GBPS)
    from oracle.oracle import Reference
    if Reference.available():
        thr = min(16, len(os.sched_getaffinity(0)))
        s, _ = Reference().bench(data_h, off_h.astype(np.uint64), sample_fraction=1.0, word_size=a.ws, threads=thr, reps=1)
        res["reference"] = dict(threads=thr, round_trip_s=s, round_trip_GBps=total / s / 1e9)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
