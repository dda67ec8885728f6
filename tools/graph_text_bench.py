#!/usr/bin/env python3
"""The graph text of M2 (62 x 5 Mbp, k = 25, f = 36, --seed 4242, gfa1) formatted two ways by one command:

  (h) twopaco --graph gfa1 --graph-text host --graph-threads N     the event table fetched, N host threads format and write
  (d) twopaco --graph gfa1 --graph-text device                     the text rendered on the device, the host only writes it

Runs alternate (h), (d), ...; every run starts --settle seconds after the last process exit (bench.py's 3.5 s).  Both write
into one directory on one disk; the sha256 of the two files must agree: exit code 1 if not.  One JSON line, also written to
--out (profiles/graph_text.json): walls, medians, spreads, the TWOPACO_TIMING phases of each path's median run (among them
"graph text on device" and text_kernel_ms, the kernels' share of it), and the verdict: the device path is the better one only
if its median is lower by more than the larger of the two spreads.  Not part of bench.py.

    python tools/graph_text_bench.py [--scale 1.0] [--threads 16] [--runs 5] [--settle 3.5] [--dir <scratch>] [--out <json file>]
"""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from graph_e2e_bench import phases, sha256_file, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--settle", type=float, default=3.5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from twopaco_amd import synth
    d = a.dir or tempfile.mkdtemp(prefix="graph_text_bench_")
    os.makedirs(d, exist_ok=True)
    recs, p = synth.workload("m2", scale=a.scale)
    files = synth.fasta_files(recs, p, d, prefix="m2_")
    twopaco = os.path.join(ROOT, "twopaco_amd", "bin", "twopaco")
    out = {"host": os.path.join(d, "host.gfa"), "device": os.path.join(d, "device.gfa")}
    base = [twopaco, "-k", str(p["k"]), "-f", str(p["L"]), "-q", str(p["q"]), "-t", "16", "--seed", "4242", "--tmpdir", d, "--graph", "gfa1",
            "--graph-threads", str(a.threads)]
    env = dict(os.environ, TWOPACO_TIMING="1")   # both paths alike: the lines cost nothing measurable
    env.pop("TWOPACO_GRAPHDUMP_STATS", None)

    def run(path):
        if os.path.exists(out[path]):
            os.unlink(out[path])
        t, r = timed(base + ["--graph-out", out[path], "--graph-text", path] + files, 3000, env=env, stderr=subprocess.PIPE)
        return t, phases(r.stderr.decode(errors="replace"))

    wall, phase, sha = {"host": [], "device": []}, {"host": [], "device": []}, {}
    for _ in range(a.runs):   # alternating
        for path in ("host", "device"):
            time.sleep(a.settle)
            t, ph = run(path)
            wall[path].append(t)
            phase[path].append(ph)
            sha.setdefault(path, sha256_file(out[path]))
    result = {"workload": "m2", "scale": a.scale, "k": p["k"], "f": p["L"], "format": "gfa1", "threads": a.threads, "runs": a.runs, "settle_s": a.settle,
              "gfa_bytes": os.path.getsize(out["device"]), "sha256_equal": sha["host"] == sha["device"], "sha256": sha["device"]}
    for path in ("host", "device"):
        mid = sorted(range(a.runs), key=lambda i: wall[path][i])[a.runs // 2]
        result[path + "_wall_s"] = [round(x, 3) for x in wall[path]]
        result[path + "_median_s"] = round(statistics.median(wall[path]), 3)
        result[path + "_spread_s"] = round(max(wall[path]) - min(wall[path]), 3)
        result[path + "_phases_ms"] = phase[path][mid]
    result["text_kernel_ms"] = result["device_phases_ms"].get("text_kernel_ms")
    result["gain_s"] = round(result["host_median_s"] - result["device_median_s"], 3)
    result["device_better_beyond_spread"] = result["gain_s"] > max(result["host_spread_s"], result["device_spread_s"])
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
