"""Times of decode-reduce (tdt_decode_reduce_v) beside the K decode-accumulate calls it replaces.
Device events around each form; within a row the forms ALTERNATE, one timed run of each per round
after --warmup rounds; median of --steps rounds with the lowest and highest.  One process per run.

  columns  a_k_accumulates   K calls of decode_accumulate_v on one context and stream: the yardstick
           b_reduce          one decode_reduce_v
           c_decode_one_peer decode_v of one peer alone: the floor
  rows     1-3  MSGS x BYTES-byte gradient-like float32 tensors (70 % exact 0.0f, else N(0, 0.01):
                tools/dec_acc_bench.py's generator, each peer its own data) at K = 2, 4, 8
           4    the same shape as bfloat16 at K = 4
           5    SMALL x 1 KiB float32 at K = 4
           6    row 2 with every blob UNCP
           7-9  one long float32 destination, the tiled form's rows: 64 MiB at K = 4, 256 MiB at K = 2 and K = 8
           a    one 256 MiB destination beside 4,096 x 64 KiB at K = 4
           b    row 2 again with the extra column
                these five add column d_reduce_one_wg: decode_reduce_v with TDT_OPT_REDUCE_TILED 0, the
                one-workgroup kernels alone (what the call launched before the tiled form); b_reduce runs
                with the default, 1.  --parent: the loaded library (PSYNE_TDT_LIB) predates the option;
                column d is left out and b_reduce is that library's call.

Before timing, each row checks once that (a) and (b) leave identical bytes on equal destinations.

Usage: python tools/dec_reduce_bench.py [--rows 123456] [--steps 10] [--warmup 3] [--out FILE]
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
    ap.add_argument("--small", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="123456")
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--out", default="profiles/dec_reduce/dec_reduce_bench.jsonl")
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)

    def grads(nbytes, dtype):
        x = torch.empty(nbytes // dtype.itemsize, dtype=torch.float32, device="cuda").normal_(0, 0.01, generator=g)
        x.masked_fill_(torch.rand(x.numel(), device="cuda", generator=g) < 0.7, 0.0)
        return x.to(dtype)

    def codec_of(ws):
        c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws))
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

    def run(row, n, nbytes, K, dtype=torch.float32, uncp=False, sizes=None, one_wg=False):
        ws, code = dtype.itemsize, {torch.float32: 1, torch.bfloat16: 3}[dtype]
        if sizes is None:
            sizes = [nbytes] * n
        n, total = len(sizes), sum(sizes)
        starts = torch.tensor(np.cumsum([0] + sizes[:-1]), dtype=torch.int64, device="cuda")
        ptrs, lens, keep, wire = [], [], [], 0
        for _ in range(K):  # each peer's blobs: one buffer, message i at its slot
            data = grads(total, dtype)
            if uncp:
                rows = torch.empty((n, nbytes + 4), dtype=torch.uint8, device="cuda")
                rows[:, :4] = torch.tensor(list(b"PCNU"), dtype=torch.uint8, device="cuda")
                rows[:, 4:] = data.view(torch.uint8).view(n, nbytes)
                blobs, off = rows.view(-1), torch.arange(n, device="cuda", dtype=torch.int64) * (nbytes + 4)
                ln = torch.full((n,), nbytes + 4, dtype=torch.int64, device="cuda")
            else:
                enc = codec_of(ws)
                blobs, slots, ln, st = enc.encode_tensors(list(torch.split(data, [b // ws for b in sizes])))
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

        def dests(fill):
            buf = torch.empty(total // ws, dtype=dtype, device="cuda")
            if fill is not None:
                buf.fill_(fill)
            return buf, starts + buf.data_ptr()

        one_wg = one_wg and not a.parent
        (da, ta), (db, tb), (dc, tc) = dests(0.25), dests(0.25), dests(None)
        ctx = dict(a=codec_of(ws), b=codec_of(ws), c=codec_of(ws))
        if one_wg:
            from psyne_amd._lib import TDT_OPT_REDUCE_TILED
            (dd, td), ctx["d"] = dests(0.25), codec_of(ws)
            ctx["d"].set_option(TDT_OPT_REDUCE_TILED, 0)
        res = {k: (torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
               for k in ctx}

        def k_calls():
            for k in range(K):
                ctx["a"].decode_accumulate_v(ptrs[k], lens[k], ta, cap, elem=code, lengths=res["a"][0], status=res["a"][1])

        calls = dict(a_k_accumulates=k_calls,
                     b_reduce=lambda: ctx["b"].decode_reduce_v(all_ptrs, all_lens, K, tb, cap, elem=code, lengths=res["b"][0],
                                                               status=res["b"][1]),
                     c_decode_one_peer=lambda: ctx["c"].decode_v(ptrs[0], lens[0], tc, cap, lengths=res["c"][0],
                                                                 status=res["c"][1]))
        if one_wg:
            calls["d_reduce_one_wg"] = lambda: ctx["d"].decode_reduce_v(all_ptrs, all_lens, K, td, cap, elem=code,
                                                                        lengths=res["d"][0], status=res["d"][1])
            calls["d_reduce_one_wg"]()
        calls["a_k_accumulates"]()
        calls["b_reduce"]()
        torch.cuda.synchronize()
        assert all(int(st.abs().sum()) == 0 for _, st in res.values())
        assert torch.equal(da.view(torch.uint8), db.view(torch.uint8)), "the reduce call and K accumulate calls differ"
        assert not one_wg or torch.equal(dd.view(torch.uint8), db.view(torch.uint8)), "the tiled and one-workgroup forms differ"
        tiled = None if a.parent else ctx["b"].stat("REDUCE_LARGE")
        t = timed(calls)
        torch.cuda.synchronize()
        assert all(int(st.abs().sum()) == 0 for _, st in res.values())
        for c in ctx.values():
            assert c.error_flags() == 0
            c.close()
        line = json.dumps(dict(tool="dec_reduce_bench", row=row, steps=a.steps, warmup=a.warmup, msgs=n, peers=K,
                               decoded_bytes_per_peer=total, wire_bytes=wire, ms=t, tiled_destinations=tiled,
                               parent_library=a.parent,
                               reduce_over_k_accumulates=t["b_reduce"]["median"] / t["a_k_accumulates"]["median"],
                               reduce_median_below_accumulates_min=t["b_reduce"]["median"] < t["a_k_accumulates"]["min"]))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del keep
        torch.cuda.empty_cache()

    for r, K in (("1", 2), ("2", 4), ("3", 8)):
        if r in a.rows:
            run("%s_f32_%dx%d_k%d" % (r, a.msgs, a.bytes, K), a.msgs, a.bytes, K)
    if "4" in a.rows:
        run("4_bf16_%dx%d_k4" % (a.msgs, a.bytes), a.msgs, a.bytes, 4, dtype=torch.bfloat16)
    if "5" in a.rows:
        run("5_f32_%dx1024_k4" % a.small, a.small, 1024, 4)
    if "6" in a.rows:
        run("6_f32_%dx%d_k4_uncp" % (a.msgs, a.bytes), a.msgs, a.bytes, 4, uncp=True)
    for r, mib, K in (("7", 64, 4), ("8", 256, 2), ("9", 256, 8)):
        if r in a.rows:
            run("%s_f32_1x%dMiB_k%d" % (r, mib, K), 0, 0, K, sizes=[mib << 20], one_wg=True)
    if "a" in a.rows:
        run("a_f32_1x256MiB_4096x65536_k4", 0, 0, 4, sizes=[256 << 20] + [65536] * 4096, one_wg=True)
    if "b" in a.rows:
        run("b_f32_%dx%d_k4" % (a.msgs, a.bytes), a.msgs, a.bytes, 4, one_wg=True)


if __name__ == "__main__":
    main()
