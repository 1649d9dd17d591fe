"""Rates of the packed wire buffer (tdt_pack_v, tdt_encode_batch_vp) beside the calls it is judged
against, on gradient-like messages (70 % exact 0.0f, else N(0, 0.01): bench.py's generator) at word
size 4.  Device events, median of --steps with the lowest and highest, one process.

  a  encode_v into slots of the encode bound: N x BYTES-byte messages
  b  encode_vp, the same messages, into a packed buffer
  c  tdt_encode_batch, the contiguous compacted call, on the same messages (they lie packed already)
  d  pack_v alone over row a's blobs
  e  tdt_copy_device of as many bytes as row d moved
  f  a skewed list, one BIG-byte message beside SMALL x BYTES-byte ones: pack_v alone over its slotted
     blobs, and tdt_encode_batch minus encode_into on the same list (the gather of one wave per blob
     with its scan; it cannot be timed alone)
  g  TINY x 1 KiB blobs through pack_v
  s  rows d, f and g again for every --cuts x --grids setting of the kernel's two knobs (the
     short-segment cut and the grid cap; PSYNE_TDT_PACK_CUT / PSYNE_TDT_PACK_GRID, read when a
     context is created)

Usage: python tools/pack_bench.py [--msgs 16384] [--bytes 65536] [--steps 10] [--rows abcdefgs] [--out FILE]
Prints one JSON line per row (and appends them to --out)."""
import argparse
import ctypes as C
import json
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=16384)
    ap.add_argument("--bytes", type=int, default=65536)
    ap.add_argument("--big", type=int, default=256 << 20)
    ap.add_argument("--small", type=int, default=4096)
    ap.add_argument("--tiny", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="abcdefgs")
    ap.add_argument("--cuts", default="0,1024,4096,16384,65536")
    ap.add_argument("--grids", default="1024,4096,16384,1048576")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from psyne_amd import TDTConfig, TdtCodec
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)

    def gradients(nbytes):
        x = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_(0, 0.01, generator=g)
        x.masked_fill_(torch.rand(x.numel(), device="cuda", generator=g) < 0.7, 0.0)
        return x.view(torch.uint8)

    def make_codec(cut=None, grid=None):
        for name, v in (("PSYNE_TDT_PACK_CUT", cut), ("PSYNE_TDT_PACK_GRID", grid)):
            os.environ.pop(name, None)
            if v is not None:
                os.environ[name] = str(v)
        c = TdtCodec(TDTConfig(sample_fraction=1.0))
        c.set_metrics(10.0, 1.0, 0.5)
        return c

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

    def emit(row, **kw):
        line = json.dumps(dict(tool="pack_bench", row=row, steps=a.steps, **kw))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def rate(nbytes, t):
        return nbytes / (t["median"] * 1e6)  # GB/s

    codec = make_codec()
    n, mb = a.msgs, a.bytes
    data = gradients(n * mb)
    off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * mb
    sizes = torch.full((n,), mb, dtype=torch.int64, device="cuda")
    slots = codec.encode_slots(off)
    bound = int(slots[-1].item())
    slotted = torch.empty(bound, dtype=torch.uint8, device="cuda")
    packed = torch.empty(bound, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    poff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    ip = (data.data_ptr() + off[:-1]).contiguous()
    bp = (slotted.data_ptr() + slots[:-1]).contiguous()
    caps = (slots[1:] - slots[:-1]).contiguous()
    shape = dict(msgs=n, msg_bytes=mb, input_bytes=n * mb)

    def enc_a():
        codec.encode_v(ip, sizes, bp, caps, lengths=lens, status=st)

    ta = timed(enc_a)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    wire = int(lens.sum().item())
    if "a" in a.rows:
        emit("a_encode_v_slotted", ms=ta, input_GBps=rate(n * mb, ta), wire_bytes=wire, **shape)

    # c first: its compacted output is what rows b and d must reproduce
    ref = torch.empty(bound, dtype=torch.uint8, device="cuda")
    roff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")

    def enc_c():
        codec.encode_batch(data, off, out=ref, out_offsets=roff, status=st)

    tc = timed(enc_c)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0 and int(roff[-1].item()) == wire
    if "c" in a.rows:
        emit("c_encode_batch_contiguous", ms=tc, input_GBps=rate(n * mb, tc), wire_bytes=wire, **shape)

    if "b" in a.rows:
        def enc_b():
            codec.encode_vp(ip, sizes, n * mb, packed, out_offsets=poff, status=st)

        tb = timed(enc_b)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0 and torch.equal(poff, roff) and torch.equal(packed[:wire], ref[:wire])
        emit("b_encode_vp_packed", ms=tb, input_GBps=rate(n * mb, tb), wire_bytes=wire, **shape)
        packed.zero_()

    def pack_row(c, ptr_t, len_t, out_t, off_t, st_t):
        def fn():
            c.pack_v(ptr_t, len_t, out_t, out_offsets=off_t, status=st_t)
        return timed(fn)

    if "d" in a.rows:
        td = pack_row(codec, bp, lens, packed, poff, st)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0 and torch.equal(poff, roff) and torch.equal(packed[:wire], ref[:wire])
        emit("d_pack_v", ms=td, copied_GBps=rate(wire, td), wire_bytes=wire, **shape)
    if "e" in a.rows:
        lib, stream = codec._lib, codec._stream(None)

        def copy_e():
            assert lib.tdt_copy_device(packed.data_ptr(), ref.data_ptr(), wire, stream) == 0

        te = timed(copy_e)
        emit("e_copy_device", ms=te, copied_GBps=rate(wire, te), wire_bytes=wire, **shape)
    assert codec.error_flags() == 0

    # the knob sweep reuses row d's blobs
    sweep = []
    if "s" in a.rows:
        sweep = [(int(c), int(gr)) for c in a.cuts.split(",") for gr in a.grids.split(",")]
    for cut, grid in sweep:
        c2 = make_codec(cut, grid)
        t = pack_row(c2, bp, lens, packed, poff, st)
        torch.cuda.synchronize()
        assert torch.equal(packed[:wire], ref[:wire])
        emit("s_d_pack_v", cut=cut, grid=grid, ms=t, copied_GBps=rate(wire, t), wire_bytes=wire)
        c2.close()
    del data, slotted, packed, ref
    torch.cuda.empty_cache()

    if "f" in a.rows:
        ns = a.small
        fsz = np.array([a.big] + [mb] * ns, dtype=np.int64)
        fn_ = fsz.size
        fdata = gradients(int(fsz.sum()))
        foff = torch.from_numpy(np.concatenate([[0], np.cumsum(fsz)])).cuda()
        fslots = codec.encode_slots(foff)
        fbound = int(fslots[-1].item())
        fslotted = torch.empty(fbound, dtype=torch.uint8, device="cuda")
        fpacked = torch.empty(fbound, dtype=torch.uint8, device="cuda")
        fref = torch.empty(fbound, dtype=torch.uint8, device="cuda")
        flens = torch.zeros(fn_, dtype=torch.int64, device="cuda")
        fst = torch.zeros(fn_, dtype=torch.int32, device="cuda")
        fpoff = torch.zeros(fn_ + 1, dtype=torch.int64, device="cuda")
        froff = torch.zeros(fn_ + 1, dtype=torch.int64, device="cuda")

        def enc_into():
            codec.encode_into(fdata, foff, slots=fslots, out=fslotted, lengths=flens, status=fst)

        def enc_batch():
            codec.encode_batch(fdata, foff, out=fref, out_offsets=froff, status=fst)

        ti, tb2 = timed(enc_into), timed(enc_batch)
        torch.cuda.synchronize()
        assert int(fst.abs().sum()) == 0
        fwire = int(flens.sum().item())
        fbp = (fslotted.data_ptr() + fslots[:-1]).contiguous()
        tf = pack_row(codec, fbp, flens, fpacked, fpoff, fst)
        torch.cuda.synchronize()
        assert torch.equal(fpoff, froff) and torch.equal(fpacked[:fwire], fref[:fwire])
        emit("f_skewed", big_bytes=a.big, small_msgs=ns, msg_bytes=mb, wire_bytes=fwire, big_blob_bytes=int(flens[0].item()),
             pack_v_ms=tf, pack_v_GBps=rate(fwire, tf), encode_into_ms=ti, encode_batch_ms=tb2,
             gather_by_difference_ms=tb2["median"] - ti["median"])
        for cut, grid in sweep:
            c2 = make_codec(cut, grid)
            t = pack_row(c2, fbp, flens, fpacked, fpoff, fst)
            torch.cuda.synchronize()
            assert torch.equal(fpacked[:fwire], fref[:fwire])
            emit("s_f_pack_v", cut=cut, grid=grid, ms=t, copied_GBps=rate(fwire, t), wire_bytes=fwire)
            c2.close()
        del fdata, fslotted, fpacked, fref
        torch.cuda.empty_cache()

    if "g" in a.rows:
        nt = a.tiny
        src = torch.randint(0, 256, (nt * 1024,), dtype=torch.uint8, device="cuda", generator=g)
        # the blobs: the KiBs of `src` in a shuffled order (scattered sources, no two alike)
        perm = torch.randperm(nt, device="cuda", generator=g)
        gp = (src.data_ptr() + perm * 1024).contiguous()
        gl = torch.full((nt,), 1024, dtype=torch.int64, device="cuda")
        gout = torch.empty(nt * 1024, dtype=torch.uint8, device="cuda")
        goff = torch.zeros(nt + 1, dtype=torch.int64, device="cuda")
        gst = torch.zeros(nt, dtype=torch.int32, device="cuda")
        want = src.view(nt, 1024)[perm].reshape(-1)
        tg = pack_row(codec, gp, gl, gout, goff, gst)
        torch.cuda.synchronize()
        assert torch.equal(gout, want) and int(gst.abs().sum()) == 0
        emit("g_tiny_blobs", blobs=nt, blob_bytes=1024, ms=tg, copied_GBps=rate(nt * 1024, tg))
        for cut, grid in sweep:
            c2 = make_codec(cut, grid)
            gout.zero_()
            t = pack_row(c2, gp, gl, gout, goff, gst)
            torch.cuda.synchronize()
            assert torch.equal(gout, want)
            emit("s_g_pack_v", cut=cut, grid=grid, ms=t, copied_GBps=rate(nt * 1024, t))
            c2.close()
        # odd lengths around 1 KiB: heads and tails at every blob boundary
        gl2 = torch.randint(900, 1025, (nt,), dtype=torch.int64, device="cuda", generator=g)
        tg2 = pack_row(codec, gp, gl2, gout, goff, gst)
        torch.cuda.synchronize()
        emit("g_tiny_blobs_ragged", blobs=nt, blob_bytes="900..1024", ms=tg2, copied_GBps=rate(int(gl2.sum().item()), tg2))
    assert codec.error_flags() == 0


if __name__ == "__main__":
    main()
