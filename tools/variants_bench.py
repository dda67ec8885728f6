#!/usr/bin/env python3
"""The variant table on M2 (62 x 5 Mbp, k = 25, f = 36, --seed 4242): `graphdump --variants file --variants-ref 0 --variants-vcf` two ways,

  (a) serial:  graphdump <stream> -k 25 -s ... --variants file --variants-ref 0 --variants-out file --variants-vcf file   (the walk,
               the colour, link and superbubble tables, then both walks of every event and an ordered map from (row, mask) to the allele)
  (b) device:  the same with --gpu --threads N   (csrc/tpc_segments.hip builds the table, the colour, link and superbubble stages
               read it, csrc/tpc_variants.hip walks every (event, direction), compacts, sorts and groups the traversals)

over one junction stream `twopaco -o` wrote first.  Runs alternate (a), (b), ...; every run starts --settle seconds after the
last process exit (bench.py's 3.5 s).  The sha256 of both outputs, TSV and VCF, must agree: exit code 1 if not.  Beside the walls, (b)'s
TWOPACO_GRAPHDUMP_STATS give the variant stage's kernel time (variants_kernel_ms, TPC_K_VARIANTS) next to the superbubble stage's
(superbubbles_kernel_ms) and the segment build's (kernel_ms), and the number of alleles.  The device path counts as a gain only if its
median is lower by more than the larger of the two spreads (the rule of graph_e2e_bench.py); no ratio is required of it.  A line of
progress per run goes to stderr.  One JSON line, also written to --out (profiles/variants.json).  Not part of bench.py.

    python tools/variants_bench.py [--scale 1.0] [--threads 16] [--runs 5] [--settle 3.5] [--dir <scratch>] [--out profiles/variants.json]
"""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 22), b""):
            h.update(blk)
    return h.hexdigest()


def timed(args, timeout, env):
    t0 = time.perf_counter()
    subprocess.run(args, check=True, stdout=subprocess.DEVNULL, env=env, timeout=timeout)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--settle", type=float, default=3.5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variants.json"))
    a = ap.parse_args()

    from twopaco_amd import synth
    d = a.dir or tempfile.mkdtemp(prefix="variants_bench_")
    os.makedirs(d, exist_ok=True)
    recs, p = synth.workload("m2", scale=a.scale)
    files = synth.fasta_files(recs, p, d, prefix="m2_")
    twopaco = os.path.join(ROOT, "twopaco_amd", "bin", "twopaco")
    graphdump = os.path.join(ROOT, "twopaco_amd", "bin", "graphdump")
    bin_file, serial_tsv, device_tsv, serial_vcf, device_vcf, stats = (os.path.join(d, n) for n in ("de_bruijn.bin", "serial.tsv", "device.tsv", "serial.vcf", "device.vcf", "stats.json"))
    quiet = dict(os.environ)
    quiet.pop("TWOPACO_TIMING", None)
    quiet.pop("TWOPACO_GRAPHDUMP_STATS", None)
    timed([twopaco, "-k", str(p["k"]), "-f", str(p["L"]), "-q", str(p["q"]), "-t", "16", "--seed", "4242", "--tmpdir", d, "-o", bin_file] + files, 1200, quiet)
    dump = [graphdump, bin_file, "-k", str(p["k"]), "--variants", "file", "--variants-ref", "0"]
    for f in files:
        dump += ["-s", f]

    wall_serial, wall_device, device_stats, sha = [], [], [], {}
    for _ in range(a.runs):   # alternating
        time.sleep(a.settle)
        wall_serial.append(timed(dump + ["--variants-out", serial_tsv, "--variants-vcf", serial_vcf], 3000, quiet))
        sha.setdefault("serial", (sha256_file(serial_tsv), sha256_file(serial_vcf)))
        time.sleep(a.settle)
        wall_device.append(timed(dump + ["--variants-out", device_tsv, "--variants-vcf", device_vcf, "--gpu", "--threads", str(a.threads)], 3000, dict(quiet, TWOPACO_GRAPHDUMP_STATS=stats)))
        sha.setdefault("device", (sha256_file(device_tsv), sha256_file(device_vcf)))
        with open(stats) as f:
            device_stats.append(json.load(f))
        print("run %d: serial %.3f s, device %.3f s" % (len(wall_serial), wall_serial[-1], wall_device[-1]), file=sys.stderr, flush=True)
    mid = sorted(range(a.runs), key=lambda i: wall_device[i])[a.runs // 2]
    s = device_stats[mid]
    result = {
        "workload": "m2", "scale": a.scale, "k": p["k"], "f": p["L"], "threads": a.threads, "runs": a.runs, "settle_s": a.settle, "colors": len(files),
        "events": s["events"], "segments": s["segments"], "tsv_bytes": os.path.getsize(device_tsv), "vcf_bytes": os.path.getsize(device_vcf), "stream_bytes": os.path.getsize(bin_file),
        "serial_wall_s": [round(x, 3) for x in wall_serial], "device_wall_s": [round(x, 3) for x in wall_device],
        "serial_median_s": round(statistics.median(wall_serial), 3), "device_median_s": round(statistics.median(wall_device), 3),
        "serial_spread_s": round(max(wall_serial) - min(wall_serial), 3), "device_spread_s": round(max(wall_device) - min(wall_device), 3),
        "segments_kernel_ms": [x["kernel_ms"] for x in device_stats], "superbubbles_kernel_ms": [x["superbubbles_kernel_ms"] for x in device_stats],
        "variants_kernel_ms": [x["variants_kernel_ms"] for x in device_stats], "variants_stage_ms": [x["variants_ms"] for x in device_stats],
        "superbubbles": s["superbubbles"], "alleles": s["variant_alleles"],
        "device_stats_of_median_run": s,
        "sha256_equal": sha["serial"] == sha["device"], "sha256": list(sha["device"]),
    }
    result["gain_s"] = round(result["serial_median_s"] - result["device_median_s"], 3)
    result["gain_beyond_spread"] = result["gain_s"] > max(result["serial_spread_s"], result["device_spread_s"])
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not a.dir:
        shutil.rmtree(d, ignore_errors=True)
    return 0 if result["sha256_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
