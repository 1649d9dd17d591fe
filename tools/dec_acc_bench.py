"""Times of decode-accumulate (tdt_decode_accumulate_v) beside the two-step form it replaces.
Device events around each form; within a row the forms ALTERNATE, one timed run of each per round
after --warmup rounds, so that whatever else the box is doing falls on all of them alike; median of
--steps rounds with the lowest and highest.  One process per run.

  columns  a_decode_then_add   decode_v into scratch tensors, then torch._foreach_add_ (one call per
                               dtype): today's way
           b_decode_only       decode_v alone: the floor (the fused call contains this decode)
           c_fused             decode_accumulate_v
  The pointer tables of all three are built once, outside the timed region (decode_tensors builds them
  per call on the host, the same work for every column).

  1  MSGS x BYTES-byte gradient-like float32 tensors (70 % exact 0.0f, else N(0, 0.01): bench.py's
     generator), TDT blobs
  2  the same bytes as dense UNCP blobs (what TDT_OPT_RAW_FALLBACK ships for incompressible tensors)
  3  the mixed-precision list of tools/mixed_ws_bench.py (float32 at width 4, bfloat16 at 2, float64
     at 8, shuffled)
  4  one BIG-byte float32 tensor beside N4 x BYTES-byte ones

Every row checks what it timed: after one run of (a) and one of (c) on equal accumulators the two
hold the same bits.

Usage: python tools/dec_acc_bench.py [--rows 1234] [--steps 10] [--warmup 3] [--out FILE]
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
    ap.add_argument("--n4", type=int, default=8192)
    ap.add_argument("--n2", type=int, default=8192)
    ap.add_argument("--n8", type=int, default=256)
    ap.add_argument("--big", type=int, default=256 << 20)
    ap.add_argument("--beside", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="1234")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)

    def grads(nbytes, dtype=torch.float32, width=4):
        x = torch.empty(nbytes // width, dtype=torch.float32, device="cuda").normal_(0, 0.01, generator=g)
        x.masked_fill_(torch.rand(x.numel(), device="cuda", generator=g) < 0.7, 0.0)
        return x.to(dtype)

    def codec_of(ws=4):
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

    def emit(row, **kw):
        line = json.dumps(dict(tool="dec_acc_bench", row=row, steps=a.steps, warmup=a.warmup, **kw))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def run(row, tensors, uncp=False):
        """tensors: the gradients a peer sends, one message each (views of a few large buffers)."""
        n = len(tensors)
        sz_h = np.array([t.numel() * t.element_size() for t in tensors], np.int64)
        w_h = np.array([t.element_size() for t in tensors], np.int32)
        total = int(sz_h.sum())
        if uncp:  # the marker and the tensor's bytes (tensors of one size)
            off_h = np.concatenate([[0], np.cumsum(sz_h + 4)])
            rows = torch.empty((n, int(sz_h[0]) + 4), dtype=torch.uint8, device="cuda")
            rows[:, :4] = torch.tensor(list(b"PCNU"), dtype=torch.uint8, device="cuda")
            rows[:, 4:] = torch.stack([t.view(torch.uint8) for t in tensors])
            blobs = rows.view(-1)
            lens = torch.from_numpy(sz_h + 4).cuda()
        else:
            enc = codec_of()
            blobs, slots, lens, st = enc.encode_tensors(tensors, word_sizes=[int(w) for w in w_h])
            torch.cuda.synchronize()
            assert int(st.abs().sum()) == 0
            off_h = slots.cpu().numpy()
            lens = lens[:n].clone()
            enc.close()
        offs = torch.from_numpy(np.ascontiguousarray(off_h[:n])).cuda()
        wire = int(lens.sum().item())

        def like(fill):
            out = []
            for dt in sorted({t.dtype for t in tensors}, key=str):
                group = [t for t in tensors if t.dtype == dt]
                buf = torch.empty(sum(t.numel() for t in group), dtype=dt, device="cuda")
                if fill is not None:
                    buf.fill_(fill)
                out.append((dt, list(torch.split(buf, [t.numel() for t in group]))))
            it = {dt: iter(v) for dt, v in out}
            return [next(it[t.dtype]) for t in tensors]

        acc_a, acc_c, scratch, plain = like(0.25), like(0.25), like(None), like(None)
        ctx = dict(a=codec_of(), b=codec_of(), c=codec_of())
        bptr = offs + blobs.data_ptr()
        cap = torch.from_numpy(sz_h).cuda()

        def table(ts):
            return torch.from_numpy(TdtCodec._tensor_table(ts)[0]).cuda()

        t_scratch, t_plain, t_acc = table(scratch), table(plain), table(acc_c)
        code = {torch.float32: 1, torch.float16: 2, torch.bfloat16: 3, torch.float64: 4}
        elems = torch.tensor([code[t.dtype] for t in tensors], dtype=torch.uint8, device="cuda")
        by_dtype = [([x for x in acc_a if x.dtype == dt], [x for x in scratch if x.dtype == dt])
                    for dt in {t.dtype for t in tensors}]
        res = {k: (torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
               for k in "abc"}

        def two_step():
            ctx["a"].decode_v(bptr, lens, t_scratch, cap, lengths=res["a"][0], status=res["a"][1])
            for acc, src in by_dtype:
                torch._foreach_add_(acc, src)

        calls = dict(a_decode_then_add=two_step,
                     b_decode_only=lambda: ctx["b"].decode_v(bptr, lens, t_plain, cap, lengths=res["b"][0], status=res["b"][1]),
                     c_fused=lambda: ctx["c"].decode_accumulate_v(bptr, lens, t_acc, cap, elems=elems, lengths=res["c"][0],
                                                                  status=res["c"][1]))
        t = timed(calls)
        torch.cuda.synchronize()
        assert all(int(st.abs().sum()) == 0 for _, st in res.values())
        for x, y, src in zip(acc_a, acc_c, tensors):  # the same number of runs went into both
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "fused and two-step sums differ"
        assert all(torch.equal(p.view(torch.uint8), s.view(torch.uint8)) for p, s in zip(plain[:64], tensors[:64]))
        for c in ctx.values():
            assert c.error_flags() == 0
            c.close()
        emit(row, msgs=n, decoded_bytes=total, wire_bytes=wire, ms=t,
             decoded_GBps={k: total / (v["median"] * 1e6) for k, v in t.items()},
             fused_over_two_step=t["c_fused"]["median"] / t["a_decode_then_add"]["median"],
             fused_over_decode=t["c_fused"]["median"] / t["b_decode_only"]["median"])

    def split(buf, nbytes):
        return list(torch.split(buf, nbytes // buf.element_size()))

    if "1" in a.rows or "2" in a.rows:
        data = grads(a.msgs * a.bytes)
        if "1" in a.rows:
            run("1_f32_%dx%d_tdt" % (a.msgs, a.bytes), split(data, a.bytes))
        if "2" in a.rows:
            run("2_f32_%dx%d_uncp" % (a.msgs, a.bytes), split(data, a.bytes), uncp=True)
        del data
        torch.cuda.empty_cache()
    if "3" in a.rows:
        counts = {4: a.n4, 2: a.n2, 8: a.n8}
        dt = {4: torch.float32, 2: torch.bfloat16, 8: torch.float64}
        tensors = [t for w, c in counts.items() for t in split(grads(c * a.bytes, dt[w], w), a.bytes)]
        perm = np.random.default_rng(5).permutation(len(tensors))  # the list's order: the widths interleaved
        run("3_mixed_f32_bf16_f64_%dx%d" % (len(tensors), a.bytes), [tensors[i] for i in perm])
        del tensors
        torch.cuda.empty_cache()
    if "4" in a.rows:
        data = grads(a.big + a.beside * a.bytes)
        tensors = [data[:a.big // 4]] + split(data[a.big // 4:], a.bytes)
        run("4_f32_1x%d_beside_%dx%d" % (a.big, a.beside, a.bytes), tensors)


if __name__ == "__main__":
    main()
