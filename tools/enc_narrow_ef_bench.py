"""Times of encode-narrow with error feedback (tdt_encode_narrow_ef_v: v = g + r narrowed and encoded, the fp32
residual r updated in place in the same launches) beside the composition it replaces and beside the plain
call.  Device events around each form; within a row the forms ALTERNATE, one timed run of each per round after
--warmup rounds; median of --steps rounds with the lowest and highest.  One process per row (--rows 1, ...).

  columns  a_fused_ef     one encode_narrow_v(resid_ptrs=...) over the float32 tensors and their residuals
           b_composition  what a user writes today: v = g + r into float32 scratch, encode_narrow_v of v, h = v cast
                          to the wire type, r = v - h.  The three PyTorch passes run over the FLAT buffers the
                          tensors are views of (one kernel each): the floor of the _foreach forms over the list
           c_plain        encode_narrow_v of the same tensors without residuals: what feedback adds
           c0_plain_parent the same call through the library given with --parent-lib (a build of the parent
                          commit, loaded beside this one): that the old call did not move.  --parent-first
                          times it ahead of c_plain instead of behind it (the second of the two finds the source
                          it shares with the first where the first left it)
  rows     1, 2  MSGS x BYTES of float32 (gradient-like: 70 % exact zeros, else N(0, 0.01)), bfloat16, raw fallback
                 off / on; residuals N(0, 1e-5)        3, 4  the same as float16
           5     one 256 MiB tensor beside 4,096 x 64 KiB, bfloat16        6  4,096 x 1 MiB, bfloat16

Before timing, each row checks once that (a) and (b), started from equal residuals, report the same lengths and
leave the same blobs and the same residuals (finite data: a cast and the rule agree on every element).

Usage: python tools/enc_narrow_ef_bench.py [--rows 123456] [--steps 10] [--warmup 3] [--parent-lib SO] [--out FILE]
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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-first", action="store_true")
    ap.add_argument("--out", default="profiles/enc_narrow_ef/enc_narrow_ef_bench.jsonl")
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec, _lib
    from psyne_amd._lib import TDT_ELEM_BF16_FROM_F32, TDT_ELEM_F16_FROM_F32
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    parent = _lib.load(pathlib.Path(a.parent_lib)) if a.parent_lib else None

    def codec_of(raw, lib=None):
        c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=2), raw_fallback=raw, lib=lib)
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

    def run(row, n, nbytes, dtype=torch.bfloat16, raw=False, head=0):
        """n tensors of nbytes, behind one of `head` bytes (0: none)."""
        sizes = ([head] if head else []) + [nbytes] * n
        n, tot = len(sizes), sum(sizes) // 4
        src = torch.empty(tot, dtype=torch.float32, device="cuda").normal_(0, 0.01, generator=g)
        src.masked_fill_(torch.rand(src.numel(), device="cuda", generator=g) < 0.7, 0.0)
        r0 = torch.empty(tot, dtype=torch.float32, device="cuda").normal_(0, 1e-5, generator=g)
        forms = ("a", "b", "c") + (("c0",) if parent else ())
        resid = {k: r0.clone() for k in ("a", "b")}
        v, h = torch.empty_like(src), torch.empty(tot, dtype=dtype, device="cuda")
        s32 = torch.tensor(sizes, dtype=torch.int64, device="cuda")
        off = torch.cumsum(s32, 0) - s32
        caps = s32 // 2 + 4 if raw else torch.maximum(s32 // 2 + 4, 36 + s32)
        ooff = torch.cumsum(caps, 0) - caps
        outs = {k: torch.empty(int(caps.sum()), dtype=torch.uint8, device="cuda") for k in forms}
        optr = {k: ooff + outs[k].data_ptr() for k in forms}
        psrc, pv, pres = off + src.data_ptr(), off + v.data_ptr(), off + resid["a"].data_ptr()
        ctx = {k: codec_of(raw, parent if k == "c0" else None) for k in forms}
        res = {k: (torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
               for k in forms}
        code = TDT_ELEM_BF16_FROM_F32 if dtype == torch.bfloat16 else TDT_ELEM_F16_FROM_F32

        def narrow(k, p, rp=None):
            kw = dict(resid_ptrs=rp) if rp is not None else {}
            ctx[k].encode_narrow_v(p, s32, optr[k], caps, elem=code, lengths=res[k][0], status=res[k][1], **kw)

        def composition():
            torch.add(src, resid["b"], out=v)
            narrow("b", pv)
            h.copy_(v)
            torch.sub(v, h, out=resid["b"])

        calls = dict(a_fused_ef=lambda: narrow("a", psrc, pres), b_composition=composition)
        if parent and a.parent_first:  # (which of the two plain calls follows the composition, which follows its twin)
            calls["c0_plain_parent"] = lambda: narrow("c0", psrc)
        calls["c_plain"] = lambda: narrow("c", psrc)
        if parent and not a.parent_first:
            calls["c0_plain_parent"] = lambda: narrow("c0", psrc)
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        assert all(int(st.abs().sum()) == 0 for _, st in res.values())
        assert torch.equal(res["a"][0], res["b"][0]), "the fused call and the composition report different lengths"
        assert torch.equal(resid["a"].view(torch.int32), resid["b"].view(torch.int32)), "the residuals differ"
        oo = ooff.tolist()
        for i in range(min(n, 64)):
            ln = int(res["a"][0][i])
            assert torch.equal(outs["a"][oo[i]:oo[i] + ln], outs["b"][oo[i]:oo[i] + ln]), "blob %d differs" % i
        if parent:
            assert torch.equal(outs["c"], outs["c0"]) and torch.equal(res["c"][0], res["c0"][0]), "the plain call moved"
        wire = int(res["a"][0].sum().item())
        tiled = (ctx["a"].stat("NARROW_LARGE"), ctx["a"].stat("NARROW_TILES"))
        t = timed(calls)
        torch.cuda.synchronize()
        assert all(int(st.abs().sum()) == 0 for _, st in res.values())
        for c in ctx.values():
            assert c.error_flags() == 0
            c.close()
        line = dict(tool="enc_narrow_ef_bench", row=row, parent_first=a.parent_first, steps=a.steps, warmup=a.warmup, msgs=n, source_bytes=4 * tot,
                    wire_bytes=wire, raw_fallback=raw, tiled_tensors=tiled[0], tiles=tiled[1], ms=t,
                    fused_over_composition=t["a_fused_ef"]["median"] / t["b_composition"]["median"],
                    fused_over_plain=t["a_fused_ef"]["median"] / t["c_plain"]["median"])
        if parent:
            p = t["c0_plain_parent"]
            line["plain_median_within_parent_min_max"] = p["min"] <= t["c_plain"]["median"] <= p["max"]
        line = json.dumps(line)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    bf, hf = torch.bfloat16, torch.float16
    rows = {"1": ("1_bf16_%dx%d" % (a.msgs, a.bytes), a.msgs, a.bytes, bf, False),
            "2": ("2_bf16_%dx%d_rawfb" % (a.msgs, a.bytes), a.msgs, a.bytes, bf, True),
            "3": ("3_f16_%dx%d" % (a.msgs, a.bytes), a.msgs, a.bytes, hf, False),
            "4": ("4_f16_%dx%d_rawfb" % (a.msgs, a.bytes), a.msgs, a.bytes, hf, True),
            "5": ("5_bf16_1x256MiB_4096x64KiB", 4096, 65536, bf, False, 1 << 28),
            "6": ("6_bf16_4096x1MiB", 4096, 1 << 20, bf, False)}
    for r in a.rows:
        run(*rows[r])


if __name__ == "__main__":
    main()
