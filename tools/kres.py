"""Per-kernel resource usage of the library (one line per kernel: VGPRs, spills, scratch, occupancy,
LDS), from hipcc's kernel-resource-usage remarks over the translation units psyne_amd/build.py
compiles: tdt_api.hip, tdt_anyws.hip (the generic-word-size kernels), tdt_pack.hip, and tdt_enc_ws.hip,
tdt_enc_sizes_ws.hip and tdt_enc_mapped_ws.hip once per word size (the tuned encode kernels, their size-pass
instances and their known-mapping instances live there).
Usage: python tools/kres.py [--ws 4[,8...]] [--grep SUBSTRING] [-DFLAG ...]   (device code only)"""
import concurrent.futures
import pathlib
import re
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
KEYS = ("Function Name|VGPRs|AGPRs|ScratchSize \\[bytes/lane\\]|SGPRs Spill|VGPRs Spill|"
        "Occupancy \\[waves/SIMD\\]|LDS Size \\[bytes/block\\]")


def remarks(src, flags, out):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-c", *flags,
           "-I", str(ROOT / "include"), str(src), "-o", out, "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode:
        sys.exit(p.stderr[-2000:])
    cur, rows = None, []
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(" + KEYS + r"): (\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            cur = {"name": v}
            rows.append(cur)
        elif cur is not None:
            cur[k] = v
    return rows


def main(argv):
    ws_list, grep, flags = [1, 2, 4, 8, 16], None, []
    it = iter(argv)
    for a in it:
        if a == "--ws":
            ws_list = [int(x) for x in next(it).split(",")]
        elif a == "--grep":
            grep = next(it)
        else:
            flags.append(a)
    csrc = ROOT / "psyne_amd" / "csrc"
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(csrc / "tdt_api.hip", flags, tmp + "/api.o"), (csrc / "tdt_anyws.hip", flags, tmp + "/anyws.o"),
                (csrc / "tdt_pack.hip", flags, tmp + "/pack.o")]
        if (csrc / "tdt_rawfb.hip").exists():  # (absent in a parent tree, as the mapped instances below)
            jobs.append((csrc / "tdt_rawfb.hip", flags, tmp + "/rawfb.o"))
        jobs += [(csrc / "tdt_enc_ws.hip", flags + ["-DPSY_INST_WS=%d" % ws], tmp + "/ws%d.o" % ws) for ws in ws_list]
        jobs += [(csrc / "tdt_enc_sizes_ws.hip", flags + ["-DPSY_INST_WS=%d" % ws], tmp + "/sws%d.o" % ws) for ws in ws_list]
        if (csrc / "tdt_enc_mapped_ws.hip").exists():  # (absent in a parent tree this file is copied into for an A/B)
            jobs += [(csrc / "tdt_enc_mapped_ws.hip", flags + ["-DPSY_INST_WS=%d" % ws], tmp + "/mws%d.o" % ws)
                     for ws in ws_list]
        with concurrent.futures.ThreadPoolExecutor(len(jobs)) as ex:
            rows = [r for rs in ex.map(lambda j: remarks(*j), jobs) for r in rs]
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True,
                           text=True).stdout.splitlines()
    for r, name in zip(rows, names):
        name = name.replace("void ", "").replace("psy::", "").replace("(EncodeArgs)", "").replace("(DecodeArgs)", "")
        if grep and grep not in name:
            continue
        print("%-64s vgpr %3s vspill %3s sspill %3s scratch %4s occ %s lds %s" % (
            name[:64], r.get("VGPRs"), r.get("VGPRs Spill"), r.get("SGPRs Spill"),
            r.get("ScratchSize [bytes/lane]"), r.get("Occupancy [waves/SIMD]"), r.get("LDS Size [bytes/block]")))


if __name__ == "__main__":
    main(sys.argv[1:])
