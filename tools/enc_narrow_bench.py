"""Times of encode-narrow (tdt_encode_narrow_v: float32 tensors encoded as the width-2 blobs of their bf16 / fp16
narrowing) beside what it replaces and beside its floor.  Device events around each form; within a row the
forms ALTERNATE, one timed run of each per round after --warmup rounds; median of --steps rounds with the
lowest and highest.  One process per row (run the rows one by one: --rows 1, --rows 2, ...).

  columns  a_fused           one encode_narrow_v over the float32 tensors
           b_cast_then_encode torch._foreach_copy_ of the float32 tensors into preallocated half-precision
                             scratch tensors, then the width-2 scattered encode of the scratch: today's two steps
           c_encode_narrow_in the width-2 scattered encode of the already-narrow tensors alone: the floor
  rows     1, 2  MSGS x BYTES of float32 (gradient-like: 70 % exact zeros, else N(0, 0.01)), bfloat16, raw
                 fallback off / on
           3, 4  the same as float16
           5     4,096 x 1 MiB, bfloat16 (tensors longer than the kernel keeps in LDS: three reads)
           6     262,144 x 1 KiB, bfloat16 (512 wire bytes: UNCP by the size floor)
           7     row 2 with dense random data: everything goes UNCP

Before timing, each row checks once that (a) and (b) report the same lengths and leave the same bytes in the
first blobs.  The tables of all forms are uploaded beforehand: the timed region holds launches only.

Usage: python tools/enc_narrow_bench.py [--rows 1234567] [--steps 10] [--warmup 3] [--out FILE]
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
    ap.add_argument("--rows", default="1234567")
    ap.add_argument("--out", default="profiles/enc_narrow/enc_narrow_bench.jsonl")
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec
    from psyne_amd._lib import TDT_ELEM_BF16_FROM_F32, TDT_ELEM_F16_FROM_F32
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)

    def codec_of(raw):
        c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=2), raw_fallback=raw)
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

    def run(row, n, nbytes, dtype=torch.bfloat16, raw=False, dense=False):
        ne = nbytes // 4
        if dense:
            src = torch.randint(-2**31, 2**31 - 1, (n * ne,), dtype=torch.int32, device="cuda", generator=g)
            src = (src & 0x7F7FFFFF).view(torch.float32)  # (finite: a cast and the rule agree on every element)
        else:
            src = torch.empty(n * ne, dtype=torch.float32, device="cuda").normal_(0, 0.01, generator=g)
            src.masked_fill_(torch.rand(src.numel(), device="cuda", generator=g) < 0.7, 0.0)
        scratch = torch.empty(n * ne, dtype=dtype, device="cuda")
        srcs, dsts = list(src.view(n, ne).unbind(0)), list(scratch.view(n, ne).unbind(0))
        w = 2 * ne
        cap = w + 4 if raw else max(w + 4, 36 + 2 * w)
        idx = torch.arange(n, dtype=torch.int64, device="cuda")
        outs = {k: torch.empty(n * cap, dtype=torch.uint8, device="cuda") for k in "abc"}
        optr = {k: idx * cap + outs[k].data_ptr() for k in "abc"}
        caps = torch.full((n,), cap, dtype=torch.int64, device="cuda")
        p32, s32 = idx * nbytes + src.data_ptr(), torch.full((n,), nbytes, dtype=torch.int64, device="cuda")
        p16, s16 = idx * w + scratch.data_ptr(), torch.full((n,), w, dtype=torch.int64, device="cuda")
        ctx = {k: codec_of(raw) for k in "abc"}
        res = {k: (torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
               for k in "abc"}
        code = TDT_ELEM_BF16_FROM_F32 if dtype == torch.bfloat16 else TDT_ELEM_F16_FROM_F32

        def encode16(k):
            ctx[k].encode_v(p16, s16, optr[k], caps, lengths=res[k][0], status=res[k][1])

        def cast_then_encode():
            torch._foreach_copy_(dsts, srcs)
            encode16("b")

        calls = dict(a_fused=lambda: ctx["a"].encode_narrow_v(p32, s32, optr["a"], caps, elem=code, lengths=res["a"][0],
                                                              status=res["a"][1]),
                     b_cast_then_encode=cast_then_encode, c_encode_narrow_in=lambda: encode16("c"))
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        assert all(int(st.abs().sum()) == 0 for _, st in res.values())
        assert torch.equal(res["a"][0], res["b"][0]), "the fused call and cast-then-encode report different lengths"
        for i in range(min(n, 64)):
            ln = int(res["a"][0][i])
            assert torch.equal(outs["a"][i * cap:i * cap + ln], outs["b"][i * cap:i * cap + ln]), "blob %d differs" % i
        wire = int(res["a"][0].sum().item())
        uncp = int((outs["a"].view(n, cap)[:, 0] == 0x50).sum().item())  # ("PCNU": the marker's first byte)
        t = timed(calls)
        torch.cuda.synchronize()
        assert all(int(st.abs().sum()) == 0 for _, st in res.values())
        for c in ctx.values():
            assert c.error_flags() == 0
            c.close()
        line = json.dumps(dict(tool="enc_narrow_bench", row=row, steps=a.steps, warmup=a.warmup, msgs=n, source_bytes=n * nbytes,
                               wire_bytes=wire, uncp_blobs=uncp, raw_fallback=raw, ms=t,
                               fused_over_cast_then_encode=t["a_fused"]["median"] / t["b_cast_then_encode"]["median"],
                               fused_over_encode_alone=t["a_fused"]["median"] / t["c_encode_narrow_in"]["median"],
                               fused_median_below_cast_then_encode_min=t["a_fused"]["median"] < t["b_cast_then_encode"]["min"]))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    bf, hf = torch.bfloat16, torch.float16
    rows = {"1": ("1_bf16_%dx%d" % (a.msgs, a.bytes), a.msgs, a.bytes, bf, False, False),
            "2": ("2_bf16_%dx%d_rawfb" % (a.msgs, a.bytes), a.msgs, a.bytes, bf, True, False),
            "3": ("3_f16_%dx%d" % (a.msgs, a.bytes), a.msgs, a.bytes, hf, False, False),
            "4": ("4_f16_%dx%d_rawfb" % (a.msgs, a.bytes), a.msgs, a.bytes, hf, True, False),
            "5": ("5_bf16_4096x1MiB", 4096, 1 << 20, bf, False, False),
            "6": ("6_bf16_262144x1KiB", 262144, 1024, bf, False, False),
            "7": ("7_bf16_%dx%d_dense_rawfb" % (a.msgs, a.bytes), a.msgs, a.bytes, bf, True, True)}
    for r in a.rows:
        run(*rows[r])


if __name__ == "__main__":
    main()
