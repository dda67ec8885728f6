#!/usr/bin/env python3
"""What the bubble table costs on M2 (62 x 5 Mbp, k = 25, f = 36, --seed 4242), genomes to files in one process:

  (a) links:    twopaco --graph gfa1 --graph-compact --graph-out file --links --links-out file
  (b) bubbles:  the same command with --bubbles file --bubbles-out file

(b) adds the colour stage (the arms' presence columns), the bubble stage and the table's file to (a).  Runs alternate (a), (b),
...; every run starts --settle seconds after the last process exit (bench.py's 3.5 s: a process started sooner after the exit
of one that held the filter can wait seconds in its first hipMalloc while the driver clears that memory).  Per run: the wall
time, the TWOPACO_TIMING phases, and for (b) the bubble stage's kernel time (bubbles_kernel_ms, TPC_K_BUBBLES) next to the link
stage's (links_kernel_ms) and the segment build's (segments_kernel_ms), and the header line of the table.  The bubble run counts
as slower only if its median is higher than the other's by more than the larger of the two spreads.  One JSON line, also written
to --out (profiles/bubbles.json).  Not part of bench.py.

    python tools/bubbles_bench.py [--scale 1.0] [--threads 16] [--runs 5] [--settle 3.5] [--dir <scratch>] [--out <json file>]
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
    d = a.dir or tempfile.mkdtemp(prefix="bubbles_bench_")
    os.makedirs(d, exist_ok=True)
    recs, p = synth.workload("m2", scale=a.scale)
    files = synth.fasta_files(recs, p, d, prefix="m2_")
    twopaco = os.path.join(ROOT, "twopaco_amd", "bin", "twopaco")
    graph, links, bubbles = os.path.join(d, "graph.gfa"), os.path.join(d, "links.tsv"), os.path.join(d, "bubbles.tsv")
    base = [twopaco, "-k", str(p["k"]), "-f", str(p["L"]), "-q", str(p["q"]), "-t", "16", "--seed", "4242", "--tmpdir", d, "--graph", "gfa1", "--graph-compact",
            "--graph-threads", str(a.threads), "--graph-out", graph, "--links", "--links-out", links]
    env = dict(os.environ, TWOPACO_TIMING="1")
    env.pop("TWOPACO_GRAPHDUMP_STATS", None)

    def run(which):
        for f in (graph, links, bubbles):
            if os.path.exists(f):
                os.unlink(f)
        extra = ["--bubbles", "file", "--bubbles-out", bubbles] if which == "bubbles" else []
        t0 = time.perf_counter()
        r = subprocess.run(base + extra + files, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env, timeout=3000)
        t = time.perf_counter() - t0
        head = open(bubbles).readline().rstrip("\n") if which == "bubbles" else None
        return t, phases(r.stderr.decode(errors="replace")), head

    kinds = ("links", "bubbles")
    wall, phase, head = {k: [] for k in kinds}, {k: [] for k in kinds}, None
    for _ in range(a.runs):   # alternating
        for which in kinds:
            time.sleep(a.settle)
            t, ph, h = run(which)
            wall[which].append(t)
            phase[which].append(ph)
            head = h or head
    result = {"workload": "m2", "scale": a.scale, "k": p["k"], "f": p["L"], "threads": a.threads, "runs": a.runs, "settle_s": a.settle, "table": head}
    for which in kinds:
        mid = sorted(range(a.runs), key=lambda i: wall[which][i])[a.runs // 2]
        result[which + "_wall_s"] = [round(x, 3) for x in wall[which]]
        result[which + "_median_s"] = round(statistics.median(wall[which]), 3)
        result[which + "_spread_s"] = round(max(wall[which]) - min(wall[which]), 3)
        result[which + "_phases_ms"] = phase[which]
        result[which + "_median_run"] = mid
    for key in ("bubbles_kernel_ms", "links_kernel_ms", "colors_kernel_ms", "segments_kernel_ms"):
        result[key] = [ph.get(key) for ph in phase["bubbles"]]
    result["cost_s"] = round(result["bubbles_median_s"] - result["links_median_s"], 3)
    result["bubbles_slower_beyond_spread"] = result["cost_s"] > max(result["links_spread_s"], result["bubbles_spread_s"])
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
