"""A/B of the tiled generic-width decode (psyne_amd/csrc/tdt_anyws.h): slotted decode of batches with
long blobs, TDT_OPT_ANY_DEC_TILED at 0 (every blob on one workgroup: the kernel before the tile
pipeline, the baseline) and at 1 (long blobs as 32 KiB output tiles) in the same build and process,
alternating, medians of --rounds rounds timed with device events.  The blobs are the encode's of the
same build; the rows and the message data are those of tools/anyws_tiled_bench.py:

  one_long      one 256 MiB message at width 12 (a float3 point cloud)
  frames        eight 3840 x 2160 RGB8 frames (24.9 MB each) at width 3
  long_beside   one 256 MiB message beside 4,096 x 48 KiB, width 12
  yardstick     the bytes of one_long as 5,462 x 48 KiB messages, width 12: nothing is tiled, every
                CU has work — what those bytes cost when the batch is spread by itself; option 1
                adds the plan launch there and nothing else
The acceptance line compares one_long (option 1) with the yardstick (option 1); the aim is 1.5 x
(measured: 0.63 x, 0.786 ms against 1.255 ms — profiles/anyws_dec_tiled/anyws_dec_tiled_bench.jsonl).

Usage: python tools/anyws_dec_tiled_bench.py [--rows one_long,frames,...] [--rounds 10] [--scale 1.0] [--out FILE]
Prints one JSON line per row and option, then the acceptance line (and appends them to --out)."""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tools.anyws_tiled_bench import message, rows  # noqa: E402

TDT_OPT_ANY_DEC_TILED = 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="one_long,frames,long_beside,yardstick")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2, help="calls per option before timing (the budgets grow on the second)")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every long message (a quick look)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec
    table = rows(a.scale)
    stats, lines = {}, []
    for name in a.rows.split(","):
        ws, sizes = table[name]
        rng = np.random.default_rng(12)
        uniq = {n: message(n, ws, rng) for n in set(sizes)}
        data_h = np.concatenate([uniq[n] for n in sizes])
        off_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        data, off = torch.from_numpy(data_h).cuda(), torch.from_numpy(off_h).cuda()
        n = len(sizes)
        codecs = {}
        for opt in (0, 1):
            c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws))
            c.set_metrics(10.0, 1.0, 0.5)
            c.set_option(TDT_OPT_ANY_DEC_TILED, opt)
            codecs[opt] = c
        # the blobs: the slotted encode of this build
        blobs, eslots, elens, est = codecs[1].encode_into(data, off)
        torch.cuda.synchronize()
        assert int(est.abs().sum()) == 0
        outs = {opt: (torch.zeros(int(off_h[-1]), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda"),
                      torch.full((n,), -1, dtype=torch.int32, device="cuda")) for opt in (0, 1)}

        def dec(opt):
            o, ln, st = outs[opt]
            codecs[opt].decode_into(blobs, eslots, in_lengths=elens, slots=off, out=o, lengths=ln, status=st)

        for _ in range(a.warmup):
            for opt in (0, 1):
                dec(opt)
                torch.cuda.synchronize()
        # the same bytes, lengths and statuses either way — and the messages back
        assert torch.equal(outs[0][1], outs[1][1]) and int(outs[0][2].abs().sum()) == 0 and int(outs[1][2].abs().sum()) == 0
        assert torch.equal(outs[0][0], outs[1][0]), "TDT_OPT_ANY_DEC_TILED changes the output"
        assert torch.equal(outs[1][0], data), "the decode does not give the messages back"
        claimed = {k: codecs[1].stat(k) for k in ("ANY_DEC_LARGE", "ANY_DEC_BLOCKS", "ANY_DEC_TILES")}
        ms = {0: [], 1: []}
        for _ in range(a.rounds):
            for opt in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dec(opt)
                e1.record()
                e1.synchronize()
                ms[opt].append(e0.elapsed_time(e1))
        total = int(data_h.size)
        for opt in (0, 1):
            assert codecs[opt].error_flags() == 0
            med = float(np.median(ms[opt]))
            stats[name, opt] = dict(min=min(ms[opt]), median=med, max=max(ms[opt]))
            lines.append(dict(tool="anyws_dec_tiled_bench", row=name, any_dec_tiled=opt, ws=ws, blobs=n, decoded_bytes=total,
                              longest=int(max(sizes)), blob_bytes=int(elens.sum().item()), rounds=a.rounds,
                              claimed=claimed if opt else None, decode_ms=stats[name, opt], decode_GBps=total / (med * 1e6)))
            print(json.dumps(lines[-1]), flush=True)
        for c in codecs.values():
            c.close()
        del data, off, outs, codecs, blobs
        torch.cuda.empty_cache()
    for name in a.rows.split(","):  # option 1 against option 0, by the min-max spread of either option's rounds
        s0, s1 = stats[name, 0], stats[name, 1]
        spread = max(s0["max"] - s0["min"], s1["max"] - s1["min"])
        lines.append(dict(tool="anyws_dec_tiled_bench", row=name + ":ab", option0_ms=s0["median"], option1_ms=s1["median"],
                          spread_ms=spread, speedup=s0["median"] / s1["median"],
                          verdict="faster" if s0["median"] - s1["median"] > spread else
                          "within spread" if abs(s0["median"] - s1["median"]) <= spread else "slower"))
        print(json.dumps(lines[-1]), flush=True)
    if ("one_long", 1) in stats and ("yardstick", 1) in stats:
        ratio = stats["one_long", 1]["median"] / stats["yardstick", 1]["median"]
        lines.append(dict(tool="anyws_dec_tiled_bench", row="acceptance", one_long_ms=stats["one_long", 1]["median"],
                          yardstick_ms=stats["yardstick", 1]["median"], ratio=ratio, aim=1.5, met=bool(ratio <= 1.5)))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
