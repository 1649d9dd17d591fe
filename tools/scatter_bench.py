"""Rates of the scattered-batch calls (tdt_encode_batch_v / tdt_decode_batch_v) beside the slotted
calls on the same bytes: N x BYTES-byte gradient-like messages (70 % exact 0.0f, else N(0, 0.01):
bench.py's generator) at word size 4, encode and decode timed with device events, median of --steps.

  a  encode_into / decode_into on the contiguous batch
  b  encode_v / decode_v with pointers into that same buffer, in order
  c  the same pointers shuffled
  d  what a caller holding one tensor per message did before: torch.cat of the N tensors into a
     staging buffer + (a)'s encode; (a)'s decode + one copy_ per message back out

Usage: python tools/scatter_bench.py [--msgs 16384] [--bytes 65536] [--steps 10] [--rows abcd] [--out FILE]
Prints one JSON line (and appends it to --out)."""
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
    ap.add_argument("--rows", default="abcd")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec
    n, mb = a.msgs, a.bytes
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    x = torch.empty(n * mb // 4, dtype=torch.float32, device="cuda").normal_(0, 0.01, generator=g)
    x.masked_fill_(torch.rand(x.numel(), device="cuda", generator=g) < 0.7, 0.0)
    data = x.view(torch.uint8)
    off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * mb
    codec = TdtCodec(TDTConfig(sample_fraction=1.0))
    codec.set_metrics(10.0, 1.0, 0.5)
    slots = codec.encode_slots(off)
    out = torch.empty(int(slots[-1].item()), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    back = torch.empty_like(data)
    blens = torch.zeros_like(lens)
    dst = torch.zeros_like(st)
    sizes = torch.full((n,), mb, dtype=torch.int64, device="cuda")
    caps = slots[1:] - slots[:-1]

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

    def verify(est, dlen, dstat):
        torch.cuda.synchronize()
        assert int(est.abs().sum()) == 0 and int(dstat.abs().sum()) == 0 and torch.equal(back, data)
        assert int((dlen != mb).sum()) == 0 and codec.error_flags() == 0
        back.zero_()

    def enc_a():
        codec.encode_into(data, off, slots=slots, out=out, lengths=lens, status=st)

    def dec_a():
        codec.decode_into(out, slots, in_lengths=lens, slots=off, out=back, lengths=blens, status=dst)

    res = dict(tool="scatter_bench", ws=4, msgs=n, msg_bytes=mb, input_bytes=n * mb, steps=a.steps, rows={})

    def row(name, enc, dec, est=st, dlen=blens, dstat=dst):
        e, d = timed(enc), timed(dec)
        verify(est, dlen, dstat)
        res["rows"][name] = dict(encode_ms=e, decode_ms=d, encode_GBps=n * mb / (e["median"] * 1e6),
                                 decode_GBps=n * mb / (d["median"] * 1e6))

    if "a" in a.rows:
        row("a_contiguous", enc_a, dec_a)
        ref_lens = lens.clone()
    for name, key, perm in (("b_v_in_order", "b", torch.arange(n, device="cuda")),
                            ("c_v_shuffled", "c", torch.randperm(n, device="cuda", generator=g))):
        if key not in a.rows:
            continue
        ip = (data.data_ptr() + off[:-1])[perm].contiguous()
        bp = (out.data_ptr() + slots[:-1])[perm].contiguous()
        op = (back.data_ptr() + off[:-1])[perm].contiguous()
        cp = caps[perm].contiguous()
        vl, vs, vbl, vds = (torch.zeros_like(t) for t in (lens, st, blens, dst))

        def enc_v():
            codec.encode_v(ip, sizes, bp, cp, lengths=vl, status=vs)

        def dec_v():
            codec.decode_v(bp, vl, op, sizes, lengths=vbl, status=vds)

        row(name, enc_v, dec_v, vs, vbl, vds)
        if "a" in a.rows:
            assert torch.equal(vl, ref_lens[perm])
    if "d" in a.rows:
        tensors = [data[i * mb:(i + 1) * mb].clone() for i in range(n)]
        outs = [torch.empty(mb, dtype=torch.uint8, device="cuda") for _ in range(n)]
        stage = torch.empty_like(data)

        def enc_d():
            torch.cat(tensors, out=stage)
            codec.encode_into(stage, off, slots=slots, out=out, lengths=lens, status=st)

        def dec_d():
            dec_a()
            for i, t in enumerate(outs):
                t.copy_(back[i * mb:(i + 1) * mb])

        row("d_pack_and_unpack", enc_d, dec_d)
        assert torch.equal(outs[n // 2], data[(n // 2) * mb:(n // 2 + 1) * mb])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
