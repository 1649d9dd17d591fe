"""Times of the size pass (tdt_encoded_sizes_v) and of the sizes-first packed encode
(TDT_OPT_PACK_SIZES_FIRST) beside the calls they are judged against.  Device events around each call;
within a row the calls ALTERNATE, one timed call of each per round after --warmup rounds, so that
whatever else the box is doing falls on all of them alike; median of --steps rounds with the lowest
and highest.  One process.

  1  MSGS x BYTES-byte gradient-like messages (70 % exact 0.0f, else N(0, 0.01): bench.py's
     generator, the batch of tools/pack_bench.py) at width 4: encoded_sizes_v | encode_v into slots of
     the encode bound | encode_vp, two phases | encode_vp, sizes first
  2  the mixed-precision list of tools/mixed_ws_bench.py (float32 at width 4, bfloat16 at 2, float64
     at 8, shuffled): the same four calls at mixed widths (encode_vw for encode_v)
  3  MSGS12 x BYTES12-byte records of width 12 (the generic kernels): encoded_sizes_v | encode_v

--parent-lib FILE: a build of the parent commit's library; rows 1 and 2 then also time its encode_v
(the yardstick of the size pass) and its two-phase encode_vp, in the same rounds.
Every row checks what it timed: the sizes against encode_v's lengths, both packed forms against
each other byte for byte.  `scratch_bytes` is what the context holds for the packed form.

--reverse runs the calls of a round in the opposite order (a call's place in the round is not free:
it inherits the caches and the clocks the call before it left).

Usage: python tools/enc_sizes_bench.py [--rows 123] [--steps 10] [--warmup 3] [--parent-lib FILE] [--reverse] [--out FILE]
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
    ap.add_argument("--msgs12", type=int, default=4096)
    ap.add_argument("--bytes12", type=int, default=49152)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="123")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reverse", action="store_true", help="the calls of a round in the opposite order")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec, _lib
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    parent = _lib.load(pathlib.Path(a.parent_lib)) if a.parent_lib else None

    def grads(nbytes, dtype=torch.float32, width=4):
        x = torch.empty(nbytes // width, dtype=torch.float32, device="cuda").normal_(0, 0.01, generator=g)
        x.masked_fill_(torch.rand(x.numel(), device="cuda", generator=g) < 0.7, 0.0)
        return x.to(dtype).view(torch.uint8)

    def codec_of(ws, lib=None, sizes_first=False):
        c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws), lib=lib)
        c.set_metrics(10.0, 1.0, 0.5)
        if sizes_first:
            c.set_option(_lib.TDT_OPT_PACK_SIZES_FIRST, 1)
        return c

    def timed(calls):
        """calls: name -> function.  One call of each per round, in turn."""
        if a.reverse:
            calls = dict(reversed(list(calls.items())))
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
        line = json.dumps(dict(tool="enc_sizes_bench", row=row, steps=a.steps, warmup=a.warmup, reverse=a.reverse, **kw))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def run(row, ws, ptr, sizes, widths_h, packed_rows=True):
        """widths_h: None (every message at `ws`) or the host array of per-message widths."""
        n = sizes.numel()
        mixed = widths_h is not None
        sz_h = sizes.cpu().numpy()
        w_h = widths_h.astype(np.int64) if mixed else np.full(n, ws, np.int64)
        cap_h = np.maximum(sz_h + 4, 28 + 4 * w_h + 2 * sz_h)
        slot_h = np.concatenate([[0], np.cumsum(cap_h)])
        total = int(sz_h.sum())
        mask = TdtCodec.width_mask(set(int(w) for w in w_h)) if mixed else 0
        dw = torch.from_numpy(widths_h.astype(np.int32)).cuda() if mixed else None
        slotted = torch.empty(int(slot_h[-1]), dtype=torch.uint8, device="cuda")
        bp = torch.from_numpy(slotted.data_ptr() + slot_h[:-1]).cuda()
        cap = torch.from_numpy(cap_h).cuda()
        lens = torch.zeros(n, dtype=torch.int64, device="cuda")
        st = torch.zeros(n, dtype=torch.int32, device="cuda")
        ctx = dict(size=codec_of(ws), slot=codec_of(ws))
        got = {}

        def sizes_call():
            got["sizes"] = ctx["size"].encoded_sizes_v(ptr, sizes, word_sizes=dw, width_mask=mask)

        def slotted_with(c):
            if mixed:
                return lambda: c.encode_vw(ptr, sizes, dw, mask, bp, cap, lengths=lens, status=st)
            return lambda: c.encode_v(ptr, sizes, bp, cap, lengths=lens, status=st)

        calls = dict(encoded_sizes_v=sizes_call, encode_v_slotted=slotted_with(ctx["slot"]))
        if packed_rows:
            ctx.update(two=codec_of(ws), first=codec_of(ws, sizes_first=True))
            out2 = torch.zeros(int(slot_h[-1]), dtype=torch.uint8, device="cuda")
            out1 = torch.zeros(int(slot_h[-1]), dtype=torch.uint8, device="cuda")
            off2 = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            off1 = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            st2 = torch.zeros(n, dtype=torch.int32, device="cuda")
            st1 = torch.zeros(n, dtype=torch.int32, device="cuda")
            calls["encode_vp_two_phase"] = lambda: ctx["two"].encode_vp(ptr, sizes, total, out2, word_sizes=dw, width_mask=mask,
                                                                       out_offsets=off2, status=st2)
            calls["encode_vp_sizes_first"] = lambda: ctx["first"].encode_vp(ptr, sizes, 0, out1, word_sizes=dw, width_mask=mask,
                                                                           out_offsets=off1, status=st1)
        if parent is not None:
            ctx.update(pslot=codec_of(ws, lib=parent))
            calls["parent_encode_v_slotted"] = slotted_with(ctx["pslot"])
            if packed_rows:
                ctx.update(ptwo=codec_of(ws, lib=parent))
                outp = torch.zeros(int(slot_h[-1]), dtype=torch.uint8, device="cuda")
                offp = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
                stp = torch.zeros(n, dtype=torch.int32, device="cuda")
                calls["parent_encode_vp_two_phase"] = lambda: ctx["ptwo"].encode_vp(ptr, sizes, total, outp, word_sizes=dw,
                                                                                   width_mask=mask, out_offsets=offp, status=stp)
        t = timed(calls)
        torch.cuda.synchronize()
        enc, est = got["sizes"]
        assert int(st.abs().sum()) == 0 and int(est.abs().sum()) == 0 and torch.equal(enc, lens), "sizes differ from encode_v's"
        wire = int(lens.sum().item())
        scratch = {}
        if packed_rows:
            assert int(st1.abs().sum()) == 0 and int(st2.abs().sum()) == 0
            assert torch.equal(off1, off2) and int(off1[-1].item()) == wire and torch.equal(out1[:wire], out2[:wire])
            wmax = int(w_h.max())
            scratch = dict(encode_vp_two_phase=2 * total + n * (28 + 4 * wmax), encode_vp_sizes_first=0)
            if parent is not None:
                assert torch.equal(offp, off2) and torch.equal(outp[:wire], out2[:wire])
        for c in ctx.values():
            assert c.error_flags() == 0
            c.close()
        emit(row, msgs=n, input_bytes=total, wire_bytes=wire, ms=t, scratch_bytes=scratch,
             input_GBps={k: total / (v["median"] * 1e6) for k, v in t.items()})

    if "1" in a.rows:
        n, mb = a.msgs, a.bytes
        data = grads(n * mb)
        ptr = (data.data_ptr() + torch.arange(n, dtype=torch.int64, device="cuda") * mb).contiguous()
        run("1_width4_%dx%d" % (n, mb), 4, ptr, torch.full((n,), mb, dtype=torch.int64, device="cuda"), None)
        del data, ptr
        torch.cuda.empty_cache()
    if "2" in a.rows:
        mb = a.bytes
        counts = {4: a.n4, 2: a.n2, 8: a.n8}
        dt = {4: torch.float32, 2: torch.bfloat16, 8: torch.float64}
        bufs = {w: grads(c * mb, dt[w], w) for w, c in counts.items()}
        n = sum(counts.values())
        width_h = np.concatenate([np.full(c, w, np.int32) for w, c in counts.items()])
        addr_h = np.concatenate([bufs[w].data_ptr() + np.arange(c, dtype=np.int64) * mb for w, c in counts.items()])
        perm = np.random.default_rng(5).permutation(n)  # the list's order: the widths interleaved
        width_h, addr_h = width_h[perm], addr_h[perm]
        run("2_mixed_2_4_8_%dx%d" % (n, mb), 4, torch.from_numpy(addr_h).cuda(), torch.full((n,), mb, dtype=torch.int64, device="cuda"),
            width_h)
        del bufs
        torch.cuda.empty_cache()
    if "3" in a.rows:
        n, mb = a.msgs12, a.bytes12
        assert mb % 12 == 0
        # float3 records: three gradient-like floats per 12-byte record
        data = grads(n * mb)
        ptr = (data.data_ptr() + torch.arange(n, dtype=torch.int64, device="cuda") * mb).contiguous()
        run("3_width12_%dx%d" % (n, mb), 12, ptr, torch.full((n,), mb, dtype=torch.int64, device="cuda"), None,
            packed_rows=False)


if __name__ == "__main__":
    main()
