"""Times of encode-narrow (tdt_encode_narrow_v: float32 tensors encoded as the width-2 blobs of their bf16 / fp16
narrowing) beside what it replaces and beside its floor.  Device events around each form; within a row the
forms ALTERNATE, one timed run of each per round after --warmup rounds; median of --steps rounds with the
lowest and highest.  One process per row (run the rows one by one: --rows 1, --rows 2, ...).

  columns  a_fused           one encode_narrow_v over the float32 tensors (TDT_OPT_NARROW_TILED at its default, 1)
           a0_one_workgroup  the same call on a context with TDT_OPT_NARROW_TILED 0: one workgroup per tensor
           b_cast_then_encode torch._foreach_copy_ of the float32 tensors into preallocated half-precision
                             scratch tensors, then the width-2 scattered encode of the scratch: today's two steps
           c_encode_narrow_in the width-2 scattered encode of the already-narrow tensors alone: the floor
  rows     1, 2  MSGS x BYTES of float32 (gradient-like: 70 % exact zeros, else N(0, 0.01)), bfloat16, raw
                 fallback off / on
           3, 4  the same as float16
           5     4,096 x 1 MiB, bfloat16 (tensors longer than the kernel keeps in LDS: three reads)
           6     262,144 x 1 KiB, bfloat16 (512 wire bytes: UNCP by the size floor)
           7     row 2 with dense random data: everything goes UNCP
           8     one 256 MiB tensor, bfloat16        9  one 256 MiB tensor beside 4,096 x 64 KiB
           a     row 8 all-zero                      b  row 8 dense with raw fallback
         (rows 1 and 6 hold no long tensor: a_fused against a0_one_workgroup there is what the plan and the
          snapshot cost)

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
    from psyne_amd._lib import TDT_ELEM_BF16_FROM_F32, TDT_ELEM_F16_FROM_F32, TDT_OPT_NARROW_TILED
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

    def run(row, n, nbytes, dtype=torch.bfloat16, raw=False, dense=False, zero=False, head=0):
        """n tensors of nbytes, behind one of `head` bytes (0: none)."""
        sizes = ([head] if head else []) + [nbytes] * n
        n, tot = len(sizes), sum(sizes) // 4
        if dense:
            src = torch.randint(-2**31, 2**31 - 1, (tot,), dtype=torch.int32, device="cuda", generator=g)
            src = (src & 0x7F7FFFFF).view(torch.float32)  # (finite: a cast and the rule agree on every element)
        elif zero:
            src = torch.zeros(tot, dtype=torch.float32, device="cuda")
        else:
            src = torch.empty(tot, dtype=torch.float32, device="cuda").normal_(0, 0.01, generator=g)
            src.masked_fill_(torch.rand(src.numel(), device="cuda", generator=g) < 0.7, 0.0)
        scratch = torch.empty(tot, dtype=dtype, device="cuda")
        srcs, dsts = list(src.split([b // 4 for b in sizes])), list(scratch.split([b // 4 for b in sizes]))
        s32 = torch.tensor(sizes, dtype=torch.int64, device="cuda")
        s16 = s32 // 2
        caps = s16 + 4 if raw else torch.maximum(s16 + 4, 36 + 2 * s16)
        ooff = torch.cumsum(caps, 0) - caps
        forms = ("a", "a0", "b", "c")
        outs = {k: torch.empty(int(caps.sum()), dtype=torch.uint8, device="cuda") for k in forms}
        optr = {k: ooff + outs[k].data_ptr() for k in forms}
        p32 = torch.cumsum(s32, 0) - s32 + src.data_ptr()
        p16 = torch.cumsum(s16, 0) - s16 + scratch.data_ptr()
        ctx = {k: codec_of(raw) for k in forms}
        ctx["a0"].set_option(TDT_OPT_NARROW_TILED, 0)
        res = {k: (torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
               for k in forms}
        code = TDT_ELEM_BF16_FROM_F32 if dtype == torch.bfloat16 else TDT_ELEM_F16_FROM_F32

        def encode16(k):
            ctx[k].encode_v(p16, s16, optr[k], caps, lengths=res[k][0], status=res[k][1])

        def cast_then_encode():
            torch._foreach_copy_(dsts, srcs)
            encode16("b")

        def fused(k):
            ctx[k].encode_narrow_v(p32, s32, optr[k], caps, elem=code, lengths=res[k][0], status=res[k][1])

        calls = dict(a_fused=lambda: fused("a"), a0_one_workgroup=lambda: fused("a0"),
                     b_cast_then_encode=cast_then_encode, c_encode_narrow_in=lambda: encode16("c"))
        for _ in range(2):  # (the second call finds the budgets grown to the first one's claims)
            for fn in calls.values():
                fn()
            torch.cuda.synchronize()
        assert all(int(st.abs().sum()) == 0 for _, st in res.values())
        assert torch.equal(res["a"][0], res["b"][0]), "the fused call and cast-then-encode report different lengths"
        assert torch.equal(res["a"][0], res["a0"][0]), "the tiled and the one-workgroup call report different lengths"
        oo = ooff.tolist()
        for i in range(min(n, 64)):
            ln = int(res["a"][0][i])
            for k in ("a0", "b"):
                assert torch.equal(outs["a"][oo[i]:oo[i] + ln], outs[k][oo[i]:oo[i] + ln]), "blob %d differs from %s" % (i, k)
        wire = int(res["a"][0].sum().item())
        uncp = int((outs["a"][ooff] == 0x50).sum().item())  # ("PCNU": the marker's first byte)
        tiled = (ctx["a"].stat("NARROW_LARGE"), ctx["a"].stat("NARROW_TILES"))
        t = timed(calls)
        torch.cuda.synchronize()
        assert all(int(st.abs().sum()) == 0 for _, st in res.values())
        for c in ctx.values():
            assert c.error_flags() == 0
            c.close()
        line = json.dumps(dict(tool="enc_narrow_bench", row=row, steps=a.steps, warmup=a.warmup, msgs=n, source_bytes=4 * tot,
                               wire_bytes=wire, uncp_blobs=uncp, raw_fallback=raw, tiled_tensors=tiled[0], tiles=tiled[1], ms=t,
                               tiled_over_one_workgroup=t["a_fused"]["median"] / t["a0_one_workgroup"]["median"],
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
            "7": ("7_bf16_%dx%d_dense_rawfb" % (a.msgs, a.bytes), a.msgs, a.bytes, bf, True, True),
            "8": ("8_bf16_1x256MiB", 1, 1 << 28, bf, False, False),
            "9": ("9_bf16_1x256MiB_4096x64KiB", 4096, 65536, bf, False, False, False, 1 << 28),
            "a": ("a_bf16_1x256MiB_zero", 1, 1 << 28, bf, False, False, True),
            "b": ("b_bf16_1x256MiB_dense_rawfb", 1, 1 << 28, bf, True, True)}
    for r in a.rows:
        run(*rows[r])


if __name__ == "__main__":
    main()
