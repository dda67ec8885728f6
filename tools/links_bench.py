#!/usr/bin/env python3
"""The compact gfa1 against the plain gfa1 on M2 (62 x 5 Mbp, k = 25, f = 36, --seed 4242), genomes to graph file in one process:

  (a) plain:    twopaco --graph gfa1 --graph-out file
  (b) compact:  twopaco --graph gfa1 --graph-compact --graph-out file

Runs alternate (a), (b), ...; every run starts --settle seconds after the last process exit (bench.py's 3.5 s: a process
started sooner after the exit of one that held the filter can wait seconds in its first hipMalloc while the driver clears
that memory).  Per run: the wall time, the bytes of the output, the TWOPACO_TIMING phases, and for (b) the link stage's kernel
time (links_kernel_ms, TPC_K_LINKS) next to the segment build's (segments_kernel_ms).  The compact path counts as faster only
if its median is lower than the plain one's by more than the larger of the two spreads.  One JSON line, also written to --out
(profiles/links.json).  Not part of bench.py.

    python tools/links_bench.py [--scale 1.0] [--threads 16] [--runs 5] [--settle 3.5] [--dir <scratch>] [--out <json file>]
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def phases(stderr_text):
    """{phase: ms} of the "[timing] <phase>: <ms> ms" lines."""
    out = {}
    for m in re.finditer(r"^\[timing\] (.*): ([0-9.eE+-]+) ms$", stderr_text, re.M):
        out[m.group(1).strip()] = round(float(m.group(2)), 3)
    return out


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
    d = a.dir or tempfile.mkdtemp(prefix="links_bench_")
    os.makedirs(d, exist_ok=True)
    recs, p = synth.workload("m2", scale=a.scale)
    files = synth.fasta_files(recs, p, d, prefix="m2_")
    twopaco = os.path.join(ROOT, "twopaco_amd", "bin", "twopaco")
    out_file = {"plain": os.path.join(d, "plain.gfa"), "compact": os.path.join(d, "compact.gfa")}
    base = [twopaco, "-k", str(p["k"]), "-f", str(p["L"]), "-q", str(p["q"]), "-t", "16", "--seed", "4242", "--tmpdir", d, "--graph", "gfa1",
            "--graph-threads", str(a.threads)]
    env = dict(os.environ, TWOPACO_TIMING="1")
    env.pop("TWOPACO_GRAPHDUMP_STATS", None)

    def run(which):
        if os.path.exists(out_file[which]):
            os.unlink(out_file[which])
        extra = ["--graph-compact"] if which == "compact" else []
        t0 = time.perf_counter()
        r = subprocess.run(base + extra + ["--graph-out", out_file[which]] + files, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env, timeout=3000)
        return time.perf_counter() - t0, phases(r.stderr.decode(errors="replace")), os.path.getsize(out_file[which])

    wall, phase, size = {"plain": [], "compact": []}, {"plain": [], "compact": []}, {"plain": [], "compact": []}
    for _ in range(a.runs):   # alternating
        for which in ("plain", "compact"):
            time.sleep(a.settle)
            t, ph, n = run(which)
            wall[which].append(t)
            phase[which].append(ph)
            size[which].append(n)
    result = {"workload": "m2", "scale": a.scale, "k": p["k"], "f": p["L"], "threads": a.threads, "runs": a.runs, "settle_s": a.settle}
    for which in ("plain", "compact"):
        mid = sorted(range(a.runs), key=lambda i: wall[which][i])[a.runs // 2]
        result[which + "_wall_s"] = [round(x, 3) for x in wall[which]]
        result[which + "_median_s"] = round(statistics.median(wall[which]), 3)
        result[which + "_spread_s"] = round(max(wall[which]) - min(wall[which]), 3)
        result[which + "_bytes"] = size[which]
        result[which + "_phases_ms"] = phase[which]
        result[which + "_median_run"] = mid
    result["links_kernel_ms"] = [ph.get("links_kernel_ms") for ph in phase["compact"]]
    result["segments_kernel_ms"] = [ph.get("segments_kernel_ms") for ph in phase["compact"]]
    result["gain_s"] = round(result["plain_median_s"] - result["compact_median_s"], 3)
    result["compact_faster_beyond_spread"] = result["gain_s"] > max(result["plain_spread_s"], result["compact_spread_s"])
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not a.dir:
        shutil.rmtree(d, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
