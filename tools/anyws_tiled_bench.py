"""A/B of the tiled generic-width encode (psyne_amd/csrc/tdt_anyws.h): slotted encode of batches with
long messages, TDT_OPT_ANY_TILED at 0 (every message on one workgroup) and at 1 (long messages as
64 KiB tiles) in the same build, alternating, medians of --rounds rounds timed with device events.

Rows:
  one_long      one 256 MiB message at width 12 (a float3 point cloud)
  frames        eight 3840 x 2160 RGB8 frames (24.9 MB each) at width 3
  long_beside   one 256 MiB message beside 4,096 x 48 KiB, width 12
  yardstick     the bytes of one_long as 5,462 x 48 KiB messages, width 12: nothing is tiled, every
                CU has work — what those bytes cost when the batch is spread by itself
The acceptance line compares one_long (option 1) with the yardstick: at most 1.5 x.

Messages are of the constructed kind of tools/anyws_bench.py: positions b % 3 == 0 uniform random, the
others runs (up to 765 long, then a two-value pattern of period 300).

Usage: python tools/anyws_tiled_bench.py [--rows one_long,frames,...] [--rounds 10] [--scale 1.0] [--out FILE]
Prints one JSON line per row and option, then the acceptance line (and appends them to --out)."""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
TDT_OPT_ANY_TILED = 8
RUNS = (254, 255, 256, 509, 510, 511, 1, 765, 1)


def message(nbytes, ws, rng):
    wc = nbytes // ws
    lo = [b for b in range(ws) if b % 3]
    hi = [b for b in range(ws) if b % 3 == 0]
    out = np.empty((wc, ws), np.uint8)
    out[:, hi] = rng.integers(0, 256, (wc, len(hi)), dtype=np.uint8)
    L = wc * len(lo)
    vals = rng.permutation(200)[: len(RUNS) + 2] + 1
    head = np.concatenate([np.full(r, vals[k], np.uint8) for k, r in enumerate(RUNS)])
    period = np.concatenate([np.full(200, vals[-2], np.uint8), np.full(100, vals[-1], np.uint8)])
    s = np.concatenate([head, np.tile(period, (max(L - head.size, 0) + 299) // 300)])[:L]
    out[:, lo] = s.reshape(wc, len(lo))
    return out.reshape(-1)


def rows(scale):
    long12 = int(256 * 2**20 * scale) // 12 * 12
    frame = int(3840 * 2160 * scale) * 3 // 12 * 12
    small = 49152
    return {
        "one_long": (12, [long12]),
        "frames": (3, [frame] * 8),
        "long_beside": (12, [long12] + [small] * 4096),
        "yardstick": (12, [small] * max(1, round(long12 / small))),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="one_long,frames,long_beside,yardstick")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every long message (a quick look)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec
    table = rows(a.scale)
    medians = {}
    lines = []
    for name in a.rows.split(","):
        ws, sizes = table[name]
        rng = np.random.default_rng(12)
        uniq = {n: message(n, ws, rng) for n in set(sizes)}  # (one message per size: the rate does not depend on more)
        data_h = np.concatenate([uniq[n] for n in sizes])
        off_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        data, off = torch.from_numpy(data_h).cuda(), torch.from_numpy(off_h).cuda()
        n = len(sizes)
        codecs, outs = {}, {}
        for opt in (0, 1):
            c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws))
            c.set_metrics(10.0, 1.0, 0.5)
            c.set_option(TDT_OPT_ANY_TILED, opt)
            codecs[opt] = c
        slots = codecs[0].encode_slots(off)
        for opt in (0, 1):
            outs[opt] = (torch.zeros(int(slots[-1].item()), dtype=torch.uint8, device="cuda"),
                         torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))

        def enc(opt):
            o, ln, st = outs[opt]
            codecs[opt].encode_into(data, off, slots=slots, out=o, lengths=ln, status=st)

        for _ in range(a.warmup):
            for opt in (0, 1):
                enc(opt)
                torch.cuda.synchronize()
        # the same bytes, lengths and statuses either way
        assert torch.equal(outs[0][1], outs[1][1]) and int(outs[0][2].abs().sum()) == 0 and int(outs[1][2].abs().sum()) == 0
        assert torch.equal(outs[0][0], outs[1][0]), "TDT_OPT_ANY_TILED changes the blobs"
        ms = {0: [], 1: []}
        for _ in range(a.rounds):
            for opt in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                enc(opt)
                e1.record()
                e1.synchronize()
                ms[opt].append(e0.elapsed_time(e1))
        total = int(data_h.size)
        for opt in (0, 1):
            assert codecs[opt].error_flags() == 0
            med = float(np.median(ms[opt]))
            medians[name, opt] = med
            lines.append(dict(tool="anyws_tiled_bench", row=name, any_tiled=opt, ws=ws, msgs=n, input_bytes=total,
                              longest=int(max(sizes)), encoded_bytes=int(outs[opt][1].sum().item()), rounds=a.rounds,
                              encode_ms=dict(min=min(ms[opt]), median=med, max=max(ms[opt])), encode_GBps=total / (med * 1e6)))
            print(json.dumps(lines[-1]), flush=True)
            codecs[opt].close()
        del data, off, outs, codecs
        torch.cuda.empty_cache()
    if ("one_long", 1) in medians and ("yardstick", 1) in medians:
        ratio = medians["one_long", 1] / medians["yardstick", 1]
        lines.append(dict(tool="anyws_tiled_bench", row="acceptance", one_long_ms=medians["one_long", 1],
                          yardstick_ms=medians["yardstick", 1], ratio=ratio, bound=1.5, met=bool(ratio <= 1.5)))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
