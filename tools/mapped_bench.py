"""Times of the known-mapping encode (tdt_encode_mapped_v) beside the ordinary scattered encode, of
tdt_mappings_v beside tdt_encoded_sizes_v, and of the packed encode at TDT_OPT_PACK_SIZES_FIRST 0 / 1 / 2.
Device events around each call; within a row the calls ALTERNATE, one timed call of each per round after
--warmup rounds, so that whatever else the box is doing falls on all of them alike; median of --steps
rounds with the lowest and highest.  One process per run.

  1  MSGS x BYTES-byte gradient-like float32 messages (70 % exact 0.0f, else N(0, 0.01): bench.py's
     generator) at width 4
  2  the mixed-precision list of tools/mixed_ws_bench.py (float32 at width 4, bfloat16 at 2, float64
     at 8, shuffled), one width per message
  3  SMALL x 1 KiB messages at width 4
  4  one BIG-byte tensor beside N4 x BYTES-byte ones at width 4; beside it the time of
     tdt_encode_with_mapping_batch on the same bytes laid contiguous (the one-team route the mapped
     scattered encode replaces)

The mapped calls use the mappings mappings_v decides for the batch, so every row checks what it timed:
the mapped blobs against the ordinary ones byte for byte, the three packed forms against each other.
--parent-lib FILE: a build of the parent commit's library; every row then also times its
encoded_sizes_v and encode_v in the same rounds (the size pass with and without the mapping export).

Usage: python tools/mapped_bench.py [--rows 1234] [--steps 10] [--warmup 3] [--parent-lib FILE] [--out FILE]
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
    ap.add_argument("--small", type=int, default=262144)
    ap.add_argument("--big", type=int, default=256 << 20)
    ap.add_argument("--beside", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="1234")
    ap.add_argument("--parent-lib", default=None)
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

    def codec_of(ws, lib=None, sizes_first=0):
        c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=ws), lib=lib)
        c.set_metrics(10.0, 1.0, 0.5)
        if sizes_first:
            c.set_option(_lib.TDT_OPT_PACK_SIZES_FIRST, sizes_first)
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
        line = json.dumps(dict(tool="mapped_bench", row=row, steps=a.steps, warmup=a.warmup, **kw))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def run(row, ws, ptr, sizes, widths_h, contiguous=None):
        """widths_h: None (every message at `ws`) or the host array of per-message widths.
        contiguous: (data, offsets) of the same bytes laid back to back, for encode_with_mapping_batch."""
        n = sizes.numel()
        mixed = widths_h is not None
        sz_h = sizes.cpu().numpy()
        w_h = widths_h.astype(np.int64) if mixed else np.full(n, ws, np.int64)
        cap_h = np.maximum(sz_h + 4, 28 + 4 * w_h + 2 * sz_h)
        slot_h = np.concatenate([[0], np.cumsum(cap_h)])
        total = int(sz_h.sum())
        mask = TdtCodec.width_mask(set(int(w) for w in w_h)) if mixed else 0
        dw = torch.from_numpy(widths_h.astype(np.int32)).cuda() if mixed else None
        cap = torch.from_numpy(cap_h).cuda()

        def slots():
            buf = torch.zeros(int(slot_h[-1]), dtype=torch.uint8, device="cuda")
            return (buf, torch.from_numpy(buf.data_ptr() + slot_h[:-1]).cuda(), torch.zeros(n, dtype=torch.int64, device="cuda"),
                    torch.zeros(n, dtype=torch.int32, device="cuda"))

        ctx = dict(plain=codec_of(ws), mapped=codec_of(ws), size=codec_of(ws), maps=codec_of(ws))
        _, bits, _ = ctx["maps"].mappings_v(ptr, sizes, word_sizes=dw, width_mask=mask)
        bits = bits.clone()
        o_plain, o_mapped = slots(), slots()
        got = {}

        def slotted_with(c, o, mapbits=None):
            if mixed:
                return lambda: c.encode_vw(ptr, sizes, dw, mask, o[1], cap, lengths=o[2], status=o[3], mapbits=mapbits)
            return lambda: c.encode_v(ptr, sizes, o[1], cap, lengths=o[2], status=o[3], mapbits=mapbits)

        def sizes_call(c, key):
            def fn():
                got[key] = c.encoded_sizes_v(ptr, sizes, word_sizes=dw, width_mask=mask)
            return fn

        def maps_call():
            got["maps"] = ctx["maps"].mappings_v(ptr, sizes, word_sizes=dw, width_mask=mask)

        calls = dict(encode_v=slotted_with(ctx["plain"], o_plain), encode_mapped_v=slotted_with(ctx["mapped"], o_mapped, bits),
                     encoded_sizes_v=sizes_call(ctx["size"], "sizes"), mappings_v=maps_call)
        packed = {}
        for value in (0, 1, 2):
            c = ctx["vp%d" % value] = codec_of(ws, sizes_first=value)
            out = torch.zeros(int(slot_h[-1]), dtype=torch.uint8, device="cuda")
            off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            st = torch.zeros(n, dtype=torch.int32, device="cuda")
            packed[value] = (out, off, st)
            calls["encode_vp_opt%d" % value] = (lambda c=c, out=out, off=off, st=st, tb=total if value == 0 else 0:
                                                c.encode_vp(ptr, sizes, tb, out, word_sizes=dw, width_mask=mask, out_offsets=off,
                                                            status=st))
        if parent is not None:
            ctx.update(pplain=codec_of(ws, lib=parent), psize=codec_of(ws, lib=parent))
            o_parent = slots()
            calls["parent_encode_v"] = slotted_with(ctx["pplain"], o_parent)
            calls["parent_encoded_sizes_v"] = sizes_call(ctx["psize"], "psizes")
        if contiguous is not None:
            data, offsets = contiguous
            ctx["lb"] = codec_of(ws)
            mp = torch.stack([(bits >> p) & 1 for p in range(ws)], 1).to(torch.int32).contiguous()
            lb_out = torch.zeros(int(slot_h[-1]), dtype=torch.uint8, device="cuda")
            lb_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            lb_st = torch.zeros(n, dtype=torch.int32, device="cuda")
            calls["encode_with_mapping_batch_contiguous"] = lambda: ctx["lb"].encode_batch(
                data, offsets, out=lb_out, out_offsets=lb_off, status=lb_st, mapping=mp)
        t = timed(calls)
        torch.cuda.synchronize()
        for o in (o_plain, o_mapped):
            assert int(o[3].abs().sum()) == 0
        assert torch.equal(o_plain[2], o_mapped[2]) and torch.equal(o_plain[0], o_mapped[0]), "mapped blobs differ"
        enc, est = got["sizes"]
        menc, mbits, mst = got["maps"]
        assert torch.equal(enc, o_plain[2]) and torch.equal(menc, enc) and torch.equal(mbits, bits)
        assert int(est.abs().sum()) == 0 and int(mst.abs().sum()) == 0
        wire = int(o_plain[2].sum().item())
        for value in (0, 1, 2):
            out, off, st = packed[value]
            assert int(st.abs().sum()) == 0 and int(off[-1].item()) == wire
            assert torch.equal(off, packed[0][1]) and torch.equal(out[:wire], packed[0][0][:wire]), "packed forms differ"
        if contiguous is not None:
            assert int(lb_st.abs().sum()) == 0 and int(lb_off[-1].item()) == wire
        for c in ctx.values():
            assert c.error_flags() == 0
            c.close()
        emit(row, msgs=n, input_bytes=total, wire_bytes=wire, ms=t,
             input_GBps={k: total / (v["median"] * 1e6) for k, v in t.items()})

    def same_size(n, mb):
        return torch.full((n,), mb, dtype=torch.int64, device="cuda")

    if "1" in a.rows:
        n, mb = a.msgs, a.bytes
        data = grads(n * mb)
        ptr = (data.data_ptr() + torch.arange(n, dtype=torch.int64, device="cuda") * mb).contiguous()
        run("1_width4_%dx%d" % (n, mb), 4, ptr, same_size(n, mb), None)
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
        run("2_mixed_2_4_8_%dx%d" % (n, mb), 4, torch.from_numpy(addr_h).cuda(), same_size(n, mb), width_h)
        del bufs
        torch.cuda.empty_cache()
    if "3" in a.rows:
        n, mb = a.small, 1024
        data = grads(n * mb)
        ptr = (data.data_ptr() + torch.arange(n, dtype=torch.int64, device="cuda") * mb).contiguous()
        run("3_width4_%dx%d" % (n, mb), 4, ptr, same_size(n, mb), None)
        del data, ptr
        torch.cuda.empty_cache()
    if "4" in a.rows:
        n, mb, big = a.beside, a.bytes, a.big
        data = grads(big + n * mb)
        size_h = np.concatenate([[big], np.full(n, mb, np.int64)]).astype(np.int64)
        off_h = np.concatenate([[0], np.cumsum(size_h)]).astype(np.int64)
        ptr = torch.from_numpy(data.data_ptr() + off_h[:-1]).cuda()
        run("4_width4_1x%d_beside_%dx%d" % (big, n, mb), 4, ptr, torch.from_numpy(size_h).cuda(), None,
            contiguous=(data, torch.from_numpy(off_h).cuda()))


if __name__ == "__main__":
    main()
