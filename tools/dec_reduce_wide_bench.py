"""Times of the widening decode-reduce (tdt_decode_reduce_v with TDT_ELEM_F32_FROM_BF16 / _F16: half-precision
blobs summed into float32 tensors) beside what it replaces and beside its floor.  Device events around each
form; within a row the forms ALTERNATE, one timed run of each per round after --warmup rounds; median of
--steps rounds with the lowest and highest.  One process per run.

  columns  a_fused_wide      one decode_reduce_v with the widening code
           b_decode_then_add one decode_v of the K peers' blobs into one flat half-precision scratch, then K
                             dst.add_(scratch_k) on flat float32 views: today's three steps in their most
                             favourable form (no per-tensor launches)
           c_narrow_reduce   decode_reduce_v of the same blobs into a half-precision tensor: the same wire
                             bytes read, half the destination bytes written: the floor
  rows     1-3  MSGS x BYTES bytes of wire per peer (gradient-like: 70 % exact zeros, else N(0, 0.01), each
                peer its own data), bfloat16, at K = 2, 4, 8
           4    the same as float16 at K = 4
           5    row 2 with every blob UNCP
           6    one 128 MiB-of-wire tensor beside 4,096 x 64 KiB at K = 4 (the tiled route)

Before timing, each row checks once that (a) and (b) leave identical bytes on equal destinations.

Usage: python tools/dec_reduce_wide_bench.py [--rows 123456] [--steps 10] [--warmup 3] [--out FILE]
Prints one JSON line per row (and appends them to --out)."""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=16384)
    ap.add_argument("--bytes", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="123456")
    ap.add_argument("--out", default="profiles/dec_reduce_wide/dec_reduce_wide_bench.jsonl")
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec
    from psyne_amd._lib import TDT_ELEM_BF16, TDT_ELEM_F16, TDT_ELEM_F32_FROM_BF16, TDT_ELEM_F32_FROM_F16
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)

    def grads(nbytes, dtype):
        x = torch.empty(nbytes // 2, dtype=torch.float32, device="cuda").normal_(0, 0.01, generator=g)
        x.masked_fill_(torch.rand(x.numel(), device="cuda", generator=g) < 0.7, 0.0)
        return x.to(dtype)

    def codec_of():
        c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=2))
        c.set_metrics(10.0, 1.0, 0.5)
        return c

    def timed(calls):
        for _ in range(a.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(a.steps):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return {k: dict(min=min(v), median=float(np.median(v)), max=max(v)) for k, v in ms.items()}

    def run(row, sizes, K, dtype=torch.bfloat16, uncp=False):
        wide, narrow = {torch.bfloat16: (TDT_ELEM_F32_FROM_BF16, TDT_ELEM_BF16),
                        torch.float16: (TDT_ELEM_F32_FROM_F16, TDT_ELEM_F16)}[dtype]
        n, total = len(sizes), sum(sizes)  # (wire bytes per peer, decoded)
        starts = torch.tensor(np.cumsum([0] + sizes[:-1]), dtype=torch.int64, device="cuda")
        ptrs, lens, keep, wire = [], [], [], 0
        for _ in range(K):  # each peer's blobs: one buffer, message i at its slot
            data = grads(total, dtype)
            if uncp:
                nbytes = sizes[0]
                rows = torch.empty((n, nbytes + 4), dtype=torch.uint8, device="cuda")
                rows[:, :4] = torch.tensor(list(b"PCNU"), dtype=torch.uint8, device="cuda")
                rows[:, 4:] = data.view(torch.uint8).view(n, nbytes)
                blobs, off = rows.view(-1), torch.arange(n, device="cuda", dtype=torch.int64) * (nbytes + 4)
                ln = torch.full((n,), nbytes + 4, dtype=torch.int64, device="cuda")
            else:
                enc = codec_of()
                blobs, slots, ln, st = enc.encode_tensors(list(torch.split(data, [b // 2 for b in sizes])))
                torch.cuda.synchronize()
                assert int(st.abs().sum()) == 0
                off, ln = slots[:n].clone(), ln[:n].clone()
                enc.close()
            del data
            keep.append(blobs)
            ptrs.append(off + blobs.data_ptr())
            lens.append(ln)
            wire += int(ln.sum().item())
        all_ptrs, all_lens = torch.cat(ptrs), torch.cat(lens)
        cap = torch.tensor(sizes, dtype=torch.int64, device="cuda")
        da = torch.full((total // 2,), 0.25, dtype=torch.float32, device="cuda")
        db, dc = da.clone(), torch.full((total // 2,), 0.25, dtype=dtype, device="cuda")
        scratch = torch.empty((K, total // 2), dtype=dtype, device="cuda")
        ta, tc = 2 * starts + da.data_ptr(), starts + dc.data_ptr()
        ts = torch.cat([starts + scratch[k].data_ptr() for k in range(K)])
        ctx = dict(a=codec_of(), b=codec_of(), c=codec_of())
        res = {k: (torch.zeros(m, dtype=torch.int64, device="cuda"), torch.zeros(m, dtype=torch.int32, device="cuda"))
               for k, m in (("a", n), ("b", K * n), ("c", n))}

        def decode_then_add():
            ctx["b"].decode_v(all_ptrs, all_lens, ts, cap.repeat(K), lengths=res["b"][0], status=res["b"][1])
            for k in range(K):
                db.add_(scratch[k])

        calls = dict(a_fused_wide=lambda: ctx["a"].decode_reduce_v(all_ptrs, all_lens, K, ta, 2 * cap, elem=wide,
                                                                   lengths=res["a"][0], status=res["a"][1]),
                     b_decode_then_add=decode_then_add,
                     c_narrow_reduce=lambda: ctx["c"].decode_reduce_v(all_ptrs, all_lens, K, tc, cap, elem=narrow,
                                                                      lengths=res["c"][0], status=res["c"][1]))
        calls["a_fused_wide"]()
        calls["b_decode_then_add"]()
        torch.cuda.synchronize()
        assert all(int(st.abs().sum()) == 0 for _, st in res.values())
        assert torch.equal(da.view(torch.int32), db.view(torch.int32)), "the fused call and decode-then-add differ"
        tiled = ctx["a"].stat("REDUCE_LARGE")
        t = timed(calls)
        torch.cuda.synchronize()
        assert all(int(st.abs().sum()) == 0 for _, st in res.values())
        for c in ctx.values():
            assert c.error_flags() == 0
            c.close()
        line = json.dumps(dict(tool="dec_reduce_wide_bench", row=row, steps=a.steps, warmup=a.warmup, msgs=n, peers=K,
                               decoded_bytes_per_peer=total, wire_bytes=wire, ms=t, tiled_destinations=tiled,
                               fused_over_decode_then_add=t["a_fused_wide"]["median"] / t["b_decode_then_add"]["median"],
                               fused_over_narrow_reduce=t["a_fused_wide"]["median"] / t["c_narrow_reduce"]["median"],
                               fused_median_below_decode_then_add_min=t["a_fused_wide"]["median"] < t["b_decode_then_add"]["min"]))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del keep
        torch.cuda.empty_cache()

    for r, K in (("1", 2), ("2", 4), ("3", 8)):
        if r in a.rows:
            run("%s_bf16_%dx%d_k%d" % (r, a.msgs, a.bytes, K), [a.bytes] * a.msgs, K)
    if "4" in a.rows:
        run("4_f16_%dx%d_k4" % (a.msgs, a.bytes), [a.bytes] * a.msgs, 4, dtype=torch.float16)
    if "5" in a.rows:
        run("5_bf16_%dx%d_k4_uncp" % (a.msgs, a.bytes), [a.bytes] * a.msgs, 4, uncp=True)
    if "6" in a.rows:
        run("6_bf16_1x128MiB_4096x65536_k4", [128 << 20] + [65536] * 4096, 4)


if __name__ == "__main__":
    main()
