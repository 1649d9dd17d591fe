"""Times of the raw fallback on the host path (TDT_OPT_HOST_RAW_FALLBACK): tdt_encode_host through the
chunked pipeline and through the one-message path.  Host-inclusive wall clock around the blocking calls.
Within a row the configurations ALTERNATE, one timed call of each per round after --warmup rounds, each
round starting one configuration further on, so that whatever else the machine is doing, and whatever a
call inherits from the one before it, falls on all of them alike; median of --steps rounds with the
lowest and highest.  One process per run.

Pipeline rows, MSGS x BYTES-byte messages (16,384 x 64 KiB = 1 GiB by default):
  grad70 / dense     bench.py's gradient (70 % exact 0.0f: compresses) / fp32 N(0, 1e-3) (expands)
  pinned / pageable  tdt_host_alloc buffers in and out / numpy buffers in and out
One-message rows: one 64 KiB message per call, dense and grad70, median latency of --one-calls calls.

Configurations of every row:
  off / on           this build with the option at 0 and at 1
  parent / parent2   with --parent-lib FILE (a build of the parent commit's library; PSYNE_TDT_LIB names
                     it too): two contexts of it in the same rounds.  The gap between the two is the
                     spread the parent shows against itself, which `off` has to lie inside: the option-off
                     path is the parent's.
Per configuration: time, wire bytes (the call's last output offset) and, for `on`,
TDT_STAT_HOST_RAW_FALLBACKS.  Every row checks what it timed: `off` gives the parent's bytes, and the
`on` lengths are min(off length, n + 4).

--profile: only the dense pinned row with the option on, a few calls — the run to put under
`rocprofv3 --kernel-trace --stats` (the stats must show host_raw_gather_kernel and no tdt_raw_copy_kernel).

Usage: python tools/host_raw_fallback_bench.py [--msgs N] [--bytes B] [--steps 10] [--warmup 2]
           [--one-calls 1000] [--parent-lib FILE] [--rows pipeline,one] [--profile] [--out FILE]
Prints one JSON line per row (and appends them to --out)."""
import argparse
import ctypes as C
import json
import os
import pathlib
import sys
import time
import zlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=16384)
    ap.add_argument("--bytes", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one-calls", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rows", default="pipeline,one")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent_path = a.parent_lib or os.environ.pop("PSYNE_TDT_LIB", None)  # (the default library stays this build's)
    import torch
    from psyne_amd import TDTConfig, TdtCodec, _lib
    lib = _lib.load()
    parent = _lib.load(pathlib.Path(parent_path)) if parent_path and not a.profile else None
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    WS = 4

    def grads(nbytes):
        x = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_(0, 0.01, generator=g)
        x.masked_fill_(torch.rand(x.numel(), device="cuda", generator=g) < 0.7, 0.0)
        return x.view(torch.uint8).cpu().numpy()

    def dense(nbytes):
        x = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_(0, 1e-3, generator=g)
        x.masked_fill_(x == 0, 1e-3)
        return x.view(torch.uint8).cpu().numpy()

    def codec_of(on, use=None):
        c = TdtCodec(TDTConfig(sample_fraction=1.0, word_size=WS), lib=use)
        c.set_metrics(10.0, 1.0, 0.5)
        if on:
            c.set_option(_lib.TDT_OPT_HOST_RAW_FALLBACK, 1)
        return c

    def configs():
        cs = {"on": codec_of(True)} if a.profile else {"off": codec_of(False), "on": codec_of(True)}
        if parent is not None:
            cs["parent"], cs["parent2"] = codec_of(False, parent), codec_of(False, parent)
        return cs

    class Buf:
        """nbytes of host memory: tdt_host_alloc's or numpy's."""

        def __init__(self, nbytes, pinned):
            self.p = None
            if pinned:
                self.p = C.c_void_p()
                _lib.check(lib.tdt_host_alloc(nbytes, C.byref(self.p)))
                self.a = np.ctypeslib.as_array(C.cast(self.p, C.POINTER(C.c_uint8)), shape=(nbytes,))
            else:
                self.a = np.empty(nbytes, np.uint8)
            self.a[:] = 0  # (touched: no page fault inside a timed call)

        def close(self):
            self.a = None
            if self.p is not None:
                lib.tdt_host_free(self.p)

    def emit(row, **kw):
        line = json.dumps(dict(tool="host_raw_fallback_bench", row=row, **kw))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def rotated(cs, r):
        """The configurations in round r's order: each round starts one further on, so that no
        configuration always runs behind the same neighbour."""
        items = list(cs.items())
        return items[r % len(items):] + items[: r % len(items)]

    def stats(v):
        return dict(min=min(v), median=float(np.median(v)), max=max(v))

    def compare(t):
        """off against the parent, and the parent against itself, in percent of the parent's median."""
        if "parent" not in t:
            return {}
        p, p2 = t["parent"]["median"], t["parent2"]["median"]
        return dict(off_vs_parent_pct=100.0 * (t["off"]["median"] - p) / p, parent_vs_itself_pct=100.0 * abs(p2 - p) / p,
                    on_vs_off_pct=100.0 * (t["on"]["median"] - t["off"]["median"]) / t["off"]["median"])

    def encode(c, src, off, n, out, cap, ooff, st):
        t0 = time.perf_counter()
        r = c._lib.tdt_encode_host(c._h, src.ctypes.data, off.ctypes.data, n, out.ctypes.data, cap, ooff.ctypes.data,
                                   st.ctypes.data)
        dt = (time.perf_counter() - t0) * 1e3
        _lib.check(r)
        return dt

    def pipeline_row(kind, data, pinned):
        n, mb = a.msgs, a.bytes
        total = n * mb
        off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(mb))
        cap = n * max(mb + 4, 28 + 4 * WS + 2 * mb)
        src, out = Buf(total, pinned), Buf(cap, pinned)
        src.a[:] = data
        cs = configs()
        res = {k: (np.zeros(n + 1, np.uint64), np.zeros(n, np.int32)) for k in cs}
        ms = {k: [] for k in cs}
        steps, warm = (3, 1) if a.profile else (a.steps, a.warmup)
        for r in range(warm + steps):
            for k, c in rotated(cs, r):
                dt = encode(c, src.a, off, n, out.a, n * (mb + 4) if k == "on" else cap, *res[k])
                if r >= warm:
                    ms[k].append(dt)
                if r == 0 and k in ("off", "parent"):  # (all lengths, and the first 64 MiB of blobs, are compared)
                    res[k + "_sum"] = zlib.crc32(out.a[: min(int(res[k][0][-1]), 64 << 20)])
        for k in cs:
            assert int(np.abs(res[k][1]).sum()) == 0, k
        fell = cs["on"].stat("HOST_RAW_FALLBACKS")
        if "off" in cs:
            ln_off, ln_on = np.diff(res["off"][0]), np.diff(res["on"][0])
            assert np.array_equal(ln_on, np.minimum(ln_off, np.uint64(mb + 4))), "option-on lengths are not min(E, n + 4)"
            assert fell == int((ln_off > mb + 4).sum()), fell
            assert cs["off"].stat("HOST_RAW_FALLBACKS") == 0
        if parent is not None:
            assert np.array_equal(res["off"][0], res["parent"][0]) and res["off_sum"] == res["parent_sum"], "off != parent"
        t = {k: stats(v) for k, v in ms.items()}
        for c in cs.values():
            assert c.error_flags() == 0
            c.close()
        emit("pipeline_%s_%s_%dx%d" % (kind, "pinned" if pinned else "pageable", n, mb), msgs=n, input_bytes=total,
             steps=steps, warmup=warm, ms=t, input_GiBps={k: total / 2 ** 30 / (v["median"] * 1e-3) for k, v in t.items()},
             wire_bytes={k: int(res[k][0][-1]) for k in cs}, host_raw_fallbacks=fell, **compare(t))
        src.close()
        out.close()

    def one_row(kind, x):
        n = x.size
        off = np.array([0, n], np.uint64)
        out = np.zeros(28 + 4 * WS + 2 * n, np.uint8)
        cs = configs()
        res = {k: (np.zeros(2, np.uint64), np.zeros(1, np.int32)) for k in cs}
        ms = {k: [] for k in cs}
        blob = {}
        warm = max(10, a.one_calls // 20)
        for r in range(warm + a.one_calls):
            for k, c in rotated(cs, r):
                dt = encode(c, x, off, 1, out, n + 4 if k == "on" else out.size, *res[k])
                if r >= warm:
                    ms[k].append(dt * 1e3)
                if r == 0:
                    blob[k] = out[: int(res[k][0][1])].tobytes()
        fell = cs["on"].stat("HOST_RAW_FALLBACKS")
        assert fell == int(len(blob["off"]) > n + 4) and len(blob["on"]) == min(len(blob["off"]), n + 4)
        if fell:
            assert blob["on"] == b"PCNU" + x.tobytes()
        if parent is not None:
            assert blob["off"] == blob["parent"]
        t = {k: stats(v) for k, v in ms.items()}
        for c in cs.values():
            c.close()
        emit("one_%s_%d" % (kind, n), calls=a.one_calls, warmup=warm, us=t, wire_bytes={k: len(blob[k]) for k in cs},
             host_raw_fallbacks=fell, **compare(t))

    total = a.msgs * a.bytes
    if a.profile:
        pipeline_row("dense", dense(total), True)
        return
    if "pipeline" in a.rows:
        for kind, make in (("grad70", grads), ("dense", dense)):
            data = make(total)
            for pinned in (True, False):
                pipeline_row(kind, data, pinned)
            del data
    if "one" in a.rows:
        one_row("dense", dense(65536))
        one_row("grad70", grads(65536))


if __name__ == "__main__":
    main()
