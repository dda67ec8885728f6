#!/usr/bin/env python3
"""graphdump -f gfa1 on M2 (62 x 5 Mbp, k = 25): the serial host walk against --gpu.

Makes M2's de_bruijn.bin with bin/twopaco, then times `graphdump -f gfa1` with and without --gpu -- stdout to a file on the
same disk, three runs each, the two alternating, median -- compares the sha256 of the two outputs and prints one JSON line
(kept in profiles/graphdump_gpu.json).  Not part of bench.py.

    python tools/graphdump_bench.py [--scale 1.0] [--threads 16] [--runs 3] [--dir <scratch directory>] [--out <json file>]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from twopaco_amd import synth
    d = a.dir or tempfile.mkdtemp(prefix="graphdump_bench_")
    os.makedirs(d, exist_ok=True)
    recs, p = synth.workload("m2", scale=a.scale)
    files = synth.fasta_files(recs, p, d, prefix="m2_")
    bin_file = os.path.join(d, "de_bruijn.bin")
    twopaco = os.path.join(ROOT, "twopaco_amd", "bin", "twopaco")
    graphdump = os.path.join(ROOT, "twopaco_amd", "bin", "graphdump")
    t0 = time.perf_counter()
    subprocess.run([twopaco, "-k", str(p["k"]), "-f", str(p["L"]), "-q", str(p["q"]), "-t", "16", "--seed", "4242", "--tmpdir", d, "-o", bin_file] + files,
                   check=True, stdout=subprocess.DEVNULL, timeout=1200)
    twopaco_s = time.perf_counter() - t0
    args = [graphdump, bin_file, "-f", "gfa1", "-k", str(p["k"])]
    for f in files:
        args += ["-s", f]
    out = {"host": os.path.join(d, "host.gfa"), "device": os.path.join(d, "device.gfa")}
    stats_file = os.path.join(d, "stats.json")
    wall = {"host": [], "device": []}
    stats, sha = [], {}
    for _ in range(a.runs):
        for side in ("host", "device"):   # alternating
            env = dict(os.environ)
            env.pop("TWOPACO_GRAPHDUMP_STATS", None)
            extra = []
            if side == "device":
                env["TWOPACO_GRAPHDUMP_STATS"] = stats_file
                extra = ["--gpu", "--threads", str(a.threads)]
            with open(out[side], "wb") as f:
                t0 = time.perf_counter()
                subprocess.run(args + extra, check=True, stdout=f, env=env, timeout=3000)
                wall[side].append(time.perf_counter() - t0)
            if side == "device":
                stats.append(json.load(open(stats_file)))
            if side not in sha:
                sha[side] = sha256_file(out[side])
    mid = sorted(range(a.runs), key=lambda i: wall["device"][i])[a.runs // 2]   # the stats of the median device run
    result = {
        "workload": "m2", "scale": a.scale, "k": p["k"], "stream_bytes": os.path.getsize(bin_file), "gfa_bytes": os.path.getsize(out["host"]),
        "twopaco_s": round(twopaco_s, 3),
        "host_wall_s": [round(x, 3) for x in wall["host"]], "device_wall_s": [round(x, 3) for x in wall["device"]],
        "host_median_s": round(statistics.median(wall["host"]), 3), "device_median_s": round(statistics.median(wall["device"]), 3),
        "host_spread_s": round(max(wall["host"]) - min(wall["host"]), 3), "device_spread_s": round(max(wall["device"]) - min(wall["device"]), 3),
        "sha256_equal": sha["host"] == sha["device"], "sha256": sha["host"], "threads": a.threads, "device_stats": stats[mid],
    }
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
