"""Times of the raw fallback (TDT_OPT_RAW_FALLBACK) on the scattered and the packed encode.  Device events
around each call; within a row the calls ALTERNATE, one timed call of each per round after --warmup
rounds, so that whatever else the box is doing falls on all of them alike; median of --steps rounds
with the lowest and highest.  One process per run.

  1  MSGS x BYTES-byte gradients, 70 % exact 0.0f (bench.py's generator): nothing falls back
  2  the same count of dense gradients, fp32 N(0, 1e-3): everything falls back
  3  half and half of the two, interleaved
  4  one BIG-byte dense tensor beside N4 x BYTES-byte gradients of row 1
  5  SMALL x 1 KiB of uniform random bytes

Per row, for encode_v, encode_vp (two phases) and encode_into (the contiguous slotted call, which under
the option reads its batch through tables and runs the scattered instances):
  opt0 / opt1   the branch library with the option at 0 and at 1
  parent        with --parent-lib FILE (a build of the parent commit's library): its encode in the same
                rounds — the no-regression comparison for opt0
  floor         tdt_encoded_sizes_v plus tdt_copy_device of the batch's bytes: the analysis and one
                copy, what the design cannot go below when everything falls back
and the memory: the slot bytes and the packed-scratch bytes at option 0 and 1.  Every row checks what it
timed: the option-1 blobs decode to the messages, and their lengths are min(option-0 length, n + 4).

Usage: python tools/raw_fallback_bench.py [--rows 12345] [--steps 10] [--warmup 3] [--parent-lib FILE] [--out FILE]
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
    ap.add_argument("--big", type=int, default=256 << 20)
    ap.add_argument("--beside", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="12345")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec, _lib
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    parent = _lib.load(pathlib.Path(a.parent_lib)) if a.parent_lib else None
    WS = 4

    def grads(nbytes):
        x = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_(0, 0.01, generator=g)
        x.masked_fill_(torch.rand(x.numel(), device="cuda", generator=g) < 0.7, 0.0)
        return x.view(torch.uint8)

    def dense(nbytes):
        x = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_(0, 1e-3, generator=g)
        x.masked_fill_(x == 0, 1e-3)
        return x.view(torch.uint8)

    def uniform(nbytes):
        return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)

    def codec_of(raw, lib=None):
        c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=WS), lib=lib)
        c.set_metrics(10.0, 1.0, 0.5)
        if raw:
            c.set_option(_lib.TDT_OPT_RAW_FALLBACK, 1)
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
        line = json.dumps(dict(tool="raw_fallback_bench", row=row, steps=a.steps, warmup=a.warmup, **kw))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def run(row, data, size_h):
        """data: one device buffer holding the messages back to back; size_h: their sizes (host int64)."""
        n = size_h.size
        off_h = np.concatenate([[0], np.cumsum(size_h)]).astype(np.int64)
        total = int(off_h[-1])
        ptr = torch.from_numpy(data.data_ptr() + off_h[:-1]).cuda()
        sizes = torch.from_numpy(size_h).cuda()
        bound = {0: np.maximum(size_h + 4, 28 + 4 * WS + 2 * size_h), 1: size_h + 4}
        mem = dict(slot_bytes={k: int(v.sum()) for k, v in bound.items()},
                   packed_scratch_bytes={0: 2 * total + n * (28 + 4 * WS), 1: total + 4 * n})

        def slots(opt):
            s = np.concatenate([[0], np.cumsum(bound[opt])])
            buf = torch.zeros(int(s[-1]), dtype=torch.uint8, device="cuda")
            return dict(buf=buf, ptr=torch.from_numpy(buf.data_ptr() + s[:-1]).cuda(), cap=torch.from_numpy(bound[opt]).cuda(),
                        ln=torch.zeros(n, dtype=torch.int64, device="cuda"), st=torch.zeros(n, dtype=torch.int32, device="cuda"))

        def packed(opt):
            return dict(out=torch.zeros(int(bound[opt].sum()), dtype=torch.uint8, device="cuda"),
                        off=torch.zeros(n + 1, dtype=torch.int64, device="cuda"), st=torch.zeros(n, dtype=torch.int32, device="cuda"))

        ctx, calls, o, p, q = {}, {}, {}, {}, {}
        d_off = torch.from_numpy(off_h).cuda()

        def add(key, opt, lib=None):
            cv, cp = codec_of(opt, lib), codec_of(opt, lib)
            ctx[key + "_v"], ctx[key + "_vp"] = cv, cp
            o[key], p[key] = slots(opt), packed(opt)
            calls["encode_v_" + key] = lambda s=o[key]: cv.encode_v(ptr, sizes, s["ptr"], s["cap"], lengths=s["ln"], status=s["st"])
            calls["encode_vp_" + key] = lambda q=p[key]: cp.encode_vp(ptr, sizes, total, q["out"], out_offsets=q["off"], status=q["st"])
            ci = ctx[key + "_into"] = codec_of(opt, lib)
            sl = ci.encode_slots(d_off)
            q[key] = dict(slots=sl, out=torch.zeros(int(bound[opt].sum()), dtype=torch.uint8, device="cuda"),
                          ln=torch.zeros(n, dtype=torch.int64, device="cuda"), st=torch.zeros(n, dtype=torch.int32, device="cuda"))
            calls["encode_into_" + key] = lambda r=q[key]: ci.encode_into(data, d_off, slots=r["slots"], out=r["out"],
                                                                           lengths=r["ln"], status=r["st"])

        add("opt0", 0)
        add("opt1", 1)
        if parent is not None:
            add("parent", 0, parent)
        ctx["floor"] = codec_of(0)
        fl = dict(dst=torch.zeros(total, dtype=torch.uint8, device="cuda"), enc=torch.zeros(n, dtype=torch.int64, device="cuda"),
                  st=torch.zeros(n, dtype=torch.int32, device="cuda"))
        lib = _lib.load()

        def floor():
            ctx["floor"].encoded_sizes_v(ptr, sizes, enc_sizes=fl["enc"], status=fl["st"])
            s = torch.cuda.current_stream().cuda_stream
            _lib.check(lib.tdt_copy_device(fl["dst"].data_ptr(), data.data_ptr(), total, s))
        calls["floor_sizes_plus_copy"] = floor
        t = timed(calls)
        torch.cuda.synchronize()
        for key in o:
            assert int(o[key]["st"].abs().sum()) == 0 and int(p[key]["st"].abs().sum()) == 0, key
        want = torch.minimum(o["opt0"]["ln"], sizes + 4)
        for key in q:
            assert int(q[key]["st"].abs().sum()) == 0 and torch.equal(q[key]["ln"], o[key]["ln"]), key
        assert torch.equal(o["opt1"]["ln"], want), "option-1 lengths are not min(E, n + 4)"
        assert torch.equal(p["opt1"]["off"][1:] - p["opt1"]["off"][:-1], want)
        if parent is not None:
            assert torch.equal(o["parent"]["ln"], o["opt0"]["ln"]) and torch.equal(o["parent"]["buf"], o["opt0"]["buf"])
        fell = int((o["opt0"]["ln"] > sizes + 4).sum().item())
        # the option-1 blobs decode to the messages
        back = torch.zeros(total, dtype=torch.uint8, device="cuda")
        dl, ds = ctx["opt1_v"].decode_v(o["opt1"]["ptr"], o["opt1"]["ln"], torch.from_numpy(back.data_ptr() + off_h[:-1]).cuda(), sizes)
        torch.cuda.synchronize()
        assert int(ds.abs().sum()) == 0 and torch.equal(back, data[:total]), "option-1 blobs do not decode to the messages"
        stat = ctx["opt1_v"].stat("RAW_FALLBACKS")
        assert stat == fell, (stat, fell)
        wire = {k: int(o[k]["ln"].sum().item()) for k in ("opt0", "opt1")}
        for c in ctx.values():
            assert c.error_flags() == 0
            c.close()
        emit(row, msgs=int(n), input_bytes=total, fell_back=fell, wire_bytes=wire, memory=mem, ms=t,
             input_GBps={k: total / (v["median"] * 1e6) for k, v in t.items()})

    if "1" in a.rows:
        n, mb = a.msgs, a.bytes
        run("1_grad70_%dx%d" % (n, mb), grads(n * mb), np.full(n, mb, np.int64))
        torch.cuda.empty_cache()
    if "2" in a.rows:
        n, mb = a.msgs, a.bytes
        run("2_dense_%dx%d" % (n, mb), dense(n * mb), np.full(n, mb, np.int64))
        torch.cuda.empty_cache()
    if "3" in a.rows:
        n, mb = a.msgs, a.bytes
        data = torch.stack([grads(n // 2 * mb).view(n // 2, mb), dense(n // 2 * mb).view(n // 2, mb)], 1).reshape(-1)
        run("3_half_and_half_%dx%d" % (n, mb), data, np.full(n, mb, np.int64))
        del data
        torch.cuda.empty_cache()
    if "4" in a.rows:
        n, mb, big = a.beside, a.bytes, a.big
        data = torch.cat([dense(big), grads(n * mb)])
        run("4_dense_1x%d_beside_%dx%d" % (big, n, mb), data, np.concatenate([[big], np.full(n, mb, np.int64)]).astype(np.int64))
        del data
        torch.cuda.empty_cache()
    if "5" in a.rows:
        n, mb = a.small, 1024
        run("5_uniform_%dx%d" % (n, mb), uniform(n * mb), np.full(n, mb, np.int64))


if __name__ == "__main__":
    main()
