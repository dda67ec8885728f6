#!/usr/bin/env python3
"""Genomes to graph.gfa on M2 (62 x 5 Mbp, k = 25, f = 36, --seed 4242), end to end, two ways:

  (a) two processes, as a user chains them:  twopaco -o de_bruijn.bin ; graphdump --gpu --threads N > file
  (b) one process:                           twopaco --graph gfa1 --graph-out file

Runs alternate (a), (b), ...; every run starts --settle seconds after the last process exit (bench.py's 3.5 s: a process
started sooner after the exit of one that held the filter can wait seconds in its first hipMalloc while the driver clears
that memory).  Inside (a) the two commands are --settle apart as well; (a) is then run once more with nothing between its
two commands, which is what a shell pipeline of the two does.  Output files lie in one directory on one disk.  The sha256 of
both outputs must agree: exit code 1 if not.  One JSON line, also written to --out (profiles/graph_e2e.json): walls, medians,
spreads, and the TWOPACO_TIMING phases of (b)'s median run.  Not part of bench.py.

    python tools/graph_e2e_bench.py [--scale 1.0] [--threads 16] [--runs 5] [--settle 3.5] [--dir <scratch>] [--out <json file>]
"""
import argparse
import hashlib
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


def sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 22), b""):
            h.update(blk)
    return h.hexdigest()


def timed(args, timeout, stdout=subprocess.DEVNULL, env=None, stderr=None):
    t0 = time.perf_counter()
    r = subprocess.run(args, check=True, stdout=stdout, stderr=stderr, env=env, timeout=timeout)
    return time.perf_counter() - t0, r


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
    d = a.dir or tempfile.mkdtemp(prefix="graph_e2e_bench_")
    os.makedirs(d, exist_ok=True)
    recs, p = synth.workload("m2", scale=a.scale)
    files = synth.fasta_files(recs, p, d, prefix="m2_")
    twopaco = os.path.join(ROOT, "twopaco_amd", "bin", "twopaco")
    graphdump = os.path.join(ROOT, "twopaco_amd", "bin", "graphdump")
    bin_file, two_gfa, one_gfa = os.path.join(d, "de_bruijn.bin"), os.path.join(d, "two.gfa"), os.path.join(d, "one.gfa")
    base = [twopaco, "-k", str(p["k"]), "-f", str(p["L"]), "-q", str(p["q"]), "-t", "16", "--seed", "4242", "--tmpdir", d]
    dump = [graphdump, bin_file, "-f", "gfa1", "-k", str(p["k"])]
    for f in files:
        dump += ["-s", f]
    dump += ["--gpu", "--threads", str(a.threads)]
    quiet = dict(os.environ)
    quiet.pop("TWOPACO_TIMING", None)
    quiet.pop("TWOPACO_GRAPHDUMP_STATS", None)
    loud = dict(quiet, TWOPACO_TIMING="1")   # (b) only: the lines cost nothing measurable, (a) stays as a user runs it

    def two(settle_between):
        for f in (bin_file, two_gfa):
            if os.path.exists(f):
                os.unlink(f)
        t1, _ = timed(base + ["-o", bin_file] + files, 1200, env=quiet)
        time.sleep(settle_between)
        with open(two_gfa, "wb") as f:
            t2, _ = timed(dump, 3000, stdout=f, env=quiet)
        return t1, t2

    def one():
        if os.path.exists(one_gfa):
            os.unlink(one_gfa)
        t, r = timed(base + ["--graph", "gfa1", "--graph-out", one_gfa, "--graph-threads", str(a.threads)] + files, 3000, env=loud, stderr=subprocess.PIPE)
        return t, phases(r.stderr.decode(errors="replace"))

    wall_two, parts_two, wall_one, phase_one, sha = [], [], [], [], {}
    for _ in range(a.runs):   # alternating
        time.sleep(a.settle)
        t1, t2 = two(a.settle)
        wall_two.append(t1 + t2)
        parts_two.append([round(t1, 3), round(t2, 3)])
        sha.setdefault("two", sha256_file(two_gfa))
        time.sleep(a.settle)
        t, ph = one()
        wall_one.append(t)
        phase_one.append(ph)
        sha.setdefault("one", sha256_file(one_gfa))
        assert not os.path.exists(os.path.join(d, "de_bruijn.gfa1"))
    time.sleep(a.settle)
    back_to_back = two(0.0)
    mid = sorted(range(a.runs), key=lambda i: wall_one[i])[a.runs // 2]
    result = {
        "workload": "m2", "scale": a.scale, "k": p["k"], "f": p["L"], "threads": a.threads, "runs": a.runs, "settle_s": a.settle,
        "gfa_bytes": os.path.getsize(one_gfa), "stream_bytes": os.path.getsize(bin_file),
        "two_process_wall_s": [round(x, 3) for x in wall_two], "two_process_parts_s": parts_two,
        "one_process_wall_s": [round(x, 3) for x in wall_one],
        "two_process_median_s": round(statistics.median(wall_two), 3), "one_process_median_s": round(statistics.median(wall_one), 3),
        "two_process_spread_s": round(max(wall_two) - min(wall_two), 3), "one_process_spread_s": round(max(wall_one) - min(wall_one), 3),
        "two_process_back_to_back_s": [round(back_to_back[0], 3), round(back_to_back[1], 3), round(sum(back_to_back), 3)],
        "sha256_equal": sha["one"] == sha["two"], "sha256": sha["one"], "one_process_phases_ms": phase_one[mid],
    }
    result["gain_s"] = round(result["two_process_median_s"] - result["one_process_median_s"], 3)
    result["gain_beyond_spread"] = result["gain_s"] > max(result["two_process_spread_s"], result["one_process_spread_s"])
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
