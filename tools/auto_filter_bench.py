#!/usr/bin/env python3
"""`twopaco -f auto` measured on a workload (default m2, the 62-genome bench workload): the sketch's estimate against the exact
edge count, a sweep of the whole two-pass step over the filter sizes 28..38 with the floor it implies for
host/filterplan.h:FILTER_PLAN_FLOOR, the step at the size the plan chooses against the sweep's best, and the sketch kernel's time.

   python tools/auto_filter_bench.py [--workload m2] [--scale 1.0] [--out profiles/auto_filter.json]
   rocprofv3 --kernel-trace --stats -d DIR -o k -- python tools/auto_filter_bench.py --trace-run     (the step and the sketch, three
       times each, for per-kernel times of one run), then
   python tools/prof_summary.py DIR/.../k_results.db > stats.csv; python tools/auto_filter_bench.py --merge-stats stats.csv
       (adds k_part_hash2 and k_distinct_sketch of that run to the JSON)

The floor is the project's "beyond spread" rule: the smallest L whose median step time is within the larger of the two
run-to-run spreads (max - min over the timed steps) of the best median of the sweep."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 20240229


def timed_steps(ctx, steps):
    import torch

    def step():
        ctx.run_begin()
        ctx.filter_reset()
        ctx.pass1_insert(count=False)
        marks = ctx.pass1_query()
        ctx.pass2_filter((1 << 64) - 1)
        J = ctx.junctions_finalize()
        ctx.emit()
        return marks, J

    step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        marks, J = step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, marks, J


def model_false_marks(n, q, L, positions, rounds=1):
    """host/filterplan.h:PredictedFalseMarks x positions."""
    import math
    return 6.0 * (-math.expm1(-q * (n / rounds) / 2.0 ** L)) ** q * positions


def context(capi, text, p, L):
    ctx = capi.Context(0)
    ctx.seq_upload(text)   # the order of -f auto: the text first, the parameters once L is known
    ctx.set_params(p["k"], L, p["q"], capi.seed_table(p["q"], L, seed=SEED))
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="m2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sizes", default="28,29,30,31,32,33,34,35,36,37,38")
    ap.add_argument("--exact-L", type=int, default=36, help="filter size of the exact count (distinct set bits / q); 0 = skip")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auto_filter.json"))
    ap.add_argument("--trace-run", action="store_true", help="only the sketch and the step at the planned size, three times each (to run under a kernel trace)")
    ap.add_argument("--merge-stats", metavar="CSV", help="add the per-kernel averages of tools/prof_summary.py's csv of a --trace-run to --out")
    ap.add_argument("--remodel", action="store_true", help="recompute the model's column of an existing --out (arithmetic only, no device)")
    args = ap.parse_args()

    if args.remodel:
        with open(args.out) as f:
            doc = json.load(f)
        for row in doc["sweep"]:
            row["predicted_false_marks"] = model_false_marks(doc["estimate"], doc["q"], row["L"], doc["positions"])
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
        return

    if args.merge_stats:
        import csv
        with open(args.out) as f:
            doc = json.load(f)
        rows = {r["kernel"]: r for r in csv.DictReader(open(args.merge_stats))}
        pick = {}
        for name, row in rows.items():
            if name.startswith("k_part_hash") or name.startswith("k_distinct_sketch") or name.startswith("k_q_hash"):
                pick[name] = {"calls": int(row["calls"]), "avg_ms": float(row["avg_ms"])}
        doc["kernel_trace"] = pick
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
        print(json.dumps(pick))
        return

    import numpy as np
    from twopaco_amd import capi, synth
    recs, p = synth.workload(args.workload, scale=args.scale)
    text = capi.PackedText.from_codes(recs)
    k, q = p["k"], p["q"]

    ctx = capi.Context(0)
    ctx.seq_upload(text)
    sketch_ms = []
    for _ in range(5):
        reg, windows = ctx.distinct_sketch(k)
        sketch_ms.append(ctx.kernel_ms("sketch"))
    estimate = capi.hll_estimate(reg)
    cap = ctx.stat("device_free_bytes") // 2
    plan = capi.filter_plan(int(estimate + 0.5), q, text.length, cap)
    ctx.close()
    doc = {"workload": args.workload, "scale": args.scale, "k": k, "q": q, "positions": int(text.length), "windows": int(windows),
           "estimate": estimate, "filter_bytes_cap": int(cap), "plan": plan,
           "sketch_kernel_ms": {"median": statistics.median(sketch_ms), "all": [round(x, 4) for x in sketch_ms]}}
    print(json.dumps(doc), flush=True)

    if args.trace_run:
        ctx = context(capi, text, p, plan["L"])
        for _ in range(3):
            ctx.distinct_sketch(k)
        ms, marks, J = timed_steps(ctx, 3)
        print(json.dumps({"trace_run_step_ms": ms, "insert_hash_kernel": ctx.stat("insert_hash_kernel")}))
        ctx.close()
        return

    if args.exact_L:
        ctx = context(capi, text, p, args.exact_L)
        ctx.run_begin()
        ctx.filter_reset()
        ctx.pass1_insert(0, None, count=False)
        words = ctx.filter_download()
        even = (words.size // 2) * 2
        bits = int(np.bitwise_count(words[:even].view(np.uint64)).sum()) + int(np.bitwise_count(words[even:]).sum())
        del words
        ctx.close()
        exact = bits / q   # (distinct bits / q undercounts by the addresses that collide: 0.03 % at a fill of 0.2 %)
        doc["exact"] = {"L": args.exact_L, "distinct_bits": bits, "edges": exact, "estimate_error_percent": 100 * (estimate - exact) / exact}
        print(json.dumps(doc["exact"]), flush=True)

    sweep = []
    for L in [int(x) for x in args.sizes.split(",")]:
        ctx = context(capi, text, p, L)
        ms, marks, J = timed_steps(ctx, args.steps)
        row = {"L": L, "median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "steps_ms": [round(x, 3) for x in ms], "marks": int(marks), "junctions": int(J),
               "insert_ms": ctx.kernel_ms("insert"), "query_ms": ctx.kernel_ms("query"), "insert_path": ctx.stat("insert_path"), "query_path": ctx.stat("query_path"),
               "predicted_false_marks": model_false_marks(estimate, q, L, text.length)}
        sweep.append(row)
        print(json.dumps(row), flush=True)
        ctx.close()
    best = min(sweep, key=lambda r: r["median_ms"])
    within = [r for r in sweep if r["median_ms"] - best["median_ms"] <= max(r["spread_ms"], best["spread_ms"])]
    floor = min(r["L"] for r in within)
    chosen = [r for r in sweep if r["L"] == plan["L"]]
    doc.update(sweep=sweep, best={"L": best["L"], "median_ms": best["median_ms"], "spread_ms": best["spread_ms"]}, measured_floor=floor)
    if chosen:
        doc["chosen_against_best"] = {"L": plan["L"], "median_ms": chosen[0]["median_ms"], "best_L": best["L"], "best_median_ms": best["median_ms"],
                                      "ratio": chosen[0]["median_ms"] / best["median_ms"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k2: doc[k2] for k2 in ("best", "measured_floor", "chosen_against_best") if k2 in doc}))


if __name__ == "__main__":
    main()
