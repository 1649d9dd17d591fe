"""Time of the mixed-width scattered encode (tdt_encode_batch_vw) on a mixed-precision gradient list
of about 1 GiB: N4 x BYTES-byte float32 messages at width 4, N2 x BYTES bfloat16 ones at width 2 (the
same distribution: 70 % exact zeros, else N(0, 0.01) — bench.py's generator — rounded to bf16) and
N8 x BYTES float64 ones at width 8, every message a view of its own, the list in shuffled order.
Device events around each call, median of --steps with the lowest and highest.

  a  what a caller does without the call: three contexts (widths 2, 4, 8) and three encode_v calls on
     one stream, the per-width tables split beforehand (the split is not timed)
  b  one encode_vw call, mask {2, 4, 8}
  c  the same call, mask {1, 2, 4, 8, 16}: the price of two pipelines that find no message
  d  every message of the list at width 4: encode_v on a width-4 context | encode_vw with mask {4}

Rows b and c must produce row a's bytes, row d's second call its first call's.
Usage: python tools/mixed_ws_bench.py [--n4 8192] [--n2 8192] [--n8 256] [--bytes 65536] [--steps 10]
       [--rows abcd] [--out FILE]          Prints one JSON line (and appends it to --out)."""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n4", type=int, default=8192)
    ap.add_argument("--n2", type=int, default=8192)
    ap.add_argument("--n8", type=int, default=256)
    ap.add_argument("--bytes", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="abcd")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec
    mb = a.bytes
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)

    def grads(count, dtype, width):
        x = torch.empty(count * mb // width, dtype=torch.float32, device="cuda").normal_(0, 0.01, generator=g)
        x.masked_fill_(torch.rand(x.numel(), device="cuda", generator=g) < 0.7, 0.0)
        return x.to(dtype).view(torch.uint8)

    bufs = {4: grads(a.n4, torch.float32, 4), 2: grads(a.n2, torch.bfloat16, 2), 8: grads(a.n8, torch.float64, 8)}
    counts = {4: a.n4, 2: a.n2, 8: a.n8}
    n = sum(counts.values())
    width_h = np.concatenate([np.full(c, w, np.int32) for w, c in counts.items()])
    addr_h = np.concatenate([bufs[w].data_ptr() + np.arange(c, dtype=np.int64) * mb for w, c in counts.items()])
    perm = np.random.default_rng(5).permutation(n)  # the list's order: the widths interleaved
    width_h, addr_h = width_h[perm], addr_h[perm]

    def codec_of(ws):
        c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws))
        c.set_metrics(10.0, 1.0, 0.5)
        return c

    def layout(widths):
        """Slots (the prefix sum of the encode bounds at `widths`) in an output buffer of their own."""
        w = widths.astype(np.int64)
        cap = np.maximum(mb + 4, 28 + 4 * w + 2 * mb)
        slot = np.concatenate([[0], np.cumsum(cap)])
        out = torch.zeros(int(slot[-1]), dtype=torch.uint8, device="cuda")
        return out, torch.from_numpy(out.data_ptr() + slot[:-1]).cuda(), torch.from_numpy(cap).cuda()

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    ptr, sizes, widths = dev(addr_h), torch.full((n,), mb, dtype=torch.int64, device="cuda"), dev(width_h)

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
        return dict(min=min(ms), median=float(np.median(ms)), max=max(ms))

    res = dict(tool="mixed_ws_bench", msgs={str(w): c for w, c in counts.items()}, msg_bytes=mb, input_bytes=n * mb,
               steps=a.steps, rows={})

    def fresh():
        return torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")

    def ok(codec, st):
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0 and codec.error_flags() == 0

    out_a = None
    if "a" in a.rows:
        out_a, bp, cap = layout(width_h)
        len_a, st_a = fresh()
        split = {}
        for w in counts:
            idx = dev(np.flatnonzero(width_h == w))
            split[w] = (codec_of(w), ptr[idx].contiguous(), sizes[idx].contiguous(), bp[idx].contiguous(),
                        cap[idx].contiguous(), torch.zeros(idx.numel(), dtype=torch.int64, device="cuda"),
                        torch.zeros(idx.numel(), dtype=torch.int32, device="cuda"), idx)

        def enc_a():
            for c, p, s, b, cp, ln, st, _ in split.values():
                c.encode_v(p, s, b, cp, lengths=ln, status=st)

        res["rows"]["a_three_contexts"] = dict(encode_ms=timed(enc_a))
        for c, _, _, _, _, ln, st, idx in split.values():
            ok(c, st)
            len_a[idx] = ln
    mixed = codec_of(4)
    for name, key, ws in (("b_vw_mask_2_4_8", "b", (2, 4, 8)), ("c_vw_mask_1_2_4_8_16", "c", (1, 2, 4, 8, 16))):
        if key not in a.rows:
            continue
        out_b, bp, cap = layout(width_h)
        ln, st = fresh()
        mask = TdtCodec.width_mask(ws)

        def enc_b():
            mixed.encode_vw(ptr, sizes, widths, mask, bp, cap, lengths=ln, status=st)

        res["rows"][name] = dict(encode_ms=timed(enc_b))
        ok(mixed, st)
        if out_a is not None:
            assert torch.equal(ln, len_a) and torch.equal(out_b, out_a), name + " differs from row a"
        del out_b
    if "d" in a.rows:
        w4 = np.full(n, 4, np.int32)
        out_v, bp_v, cap = layout(w4)
        out_w, bp_w, _ = layout(w4)
        (ln_v, st_v), (ln_w, st_w) = fresh(), fresh()
        c4, d4 = codec_of(4), dev(w4)

        def enc_v():
            c4.encode_v(ptr, sizes, bp_v, cap, lengths=ln_v, status=st_v)

        def enc_w():
            mixed.encode_vw(ptr, sizes, d4, 8, bp_w, cap, lengths=ln_w, status=st_w)

        res["rows"]["d_all_width_4"] = dict(encode_v_ms=timed(enc_v), encode_vw_ms=timed(enc_w))
        ok(c4, st_v)
        ok(mixed, st_w)
        assert torch.equal(ln_v, ln_w) and torch.equal(out_v, out_w), "row d: encode_vw differs from encode_v"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
