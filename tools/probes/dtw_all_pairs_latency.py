"""Latency of the all-pairs DTW costs on the device against the only way the pairwise entry points can
produce the same matrix.

New: dtw.all_pairs_costs(clouds) -- concatenation and upload of the clouds, mg_dtw_pair_costs, download of the (N, N) matrix.
Baseline: a Python loop of N dtw.dtw_batch(clouds[r], clouds) calls, reading `total` (N uploads of the table, the grids in
device memory, the paths downloaded and dropped).  Both in the same process on the same device, host wall clock of a
synchronised run, median of --reps after --warmup, for N motions of 156 frames +- 20 % of 19 joints; the two matrices are
compared in bits.

    python tools/probes/dtw_all_pairs_latency.py [--sizes 100,300,1000] [--baseline-max 300] [--reps 5] [--warmup 1] [--out FILE.json]

Every size runs in a child process of its own under `timeout` (--limit seconds); a size that fails ends the run.
profiles/dtw_all_pairs_latency.{json,log}: the command above with its defaults and --out.  profiles/dtw_all_pairs_kernel_stats.csv:
a run of its own, N = 100, no warm-up, one repetition of each:

    rocprofv3 --kernel-trace --stats -d DIR -o pairs --output-format csv -- \\
        python tools/probes/dtw_all_pairs_latency.py --one 100 --reps 1 --warmup 0
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dtw_latency import clouds  # noqa: E402


def median_wall(ctx, call, reps, warmup):
    walls, result = [], None
    for rep in range(warmup + reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        result = call()
        ctx.synchronize()
        if rep >= warmup:
            walls.append(time.perf_counter() - t0)
    return float(np.median(walls)), float(np.min(walls)), result


def one_size(n, reps, warmup, baseline):
    from morphablegraphs_amd import _capi, dtw
    ctx = _capi.Context(0)
    table = list(clouds(n).values())
    cells = int(sum(len(c) for c in table)) ** 2
    med, low, costs = median_wall(ctx, lambda: dtw.all_pairs_costs(table, ctx=ctx), reps, warmup)
    r = {"motions": n, "cells": cells, "device": ctx.device_info()["name"], "all_pairs_median_s": med, "all_pairs_min_s": low}
    if baseline:
        loop = lambda: np.array([[m["total"] for m in dtw.dtw_batch(a, table, ctx=ctx)] for a in table])      # noqa: E731
        bmed, blow, want = median_wall(ctx, loop, reps, warmup)
        r.update({"dtw_batch_loop_median_s": bmed, "dtw_batch_loop_min_s": blow, "ratio": bmed / med,
                  "same_bits": bool(np.array_equal(costs.view(np.uint64), want.view(np.uint64)))})
    key, means = dtw.reference_from_costs(costs, range(n))
    r.update({"selected": int(key), "least_mean_cost": float(means[key]), "mean_cost_of_motion_0": float(means[0])})
    ctx.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="100,300,1000")
    ap.add_argument("--baseline-max", type=int, default=300, help="the dtw_batch loop is timed up to this N (it is N calls)")
    ap.add_argument("--limit", type=int, default=240, help="seconds a size may take")
    ap.add_argument("--one", type=int, default=None, help="run this size in this process and print its JSON line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.one is not None:
        print("RESULT " + json.dumps(one_size(args.one, args.reps, args.warmup, args.one <= args.baseline_max)), flush=True)
        return 0
    out = {"reps": args.reps, "warmup": args.warmup, "frames": 156, "joints": 19, "results": []}
    for n in [int(s) for s in args.sizes.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", str(n), "--reps", str(args.reps), "--warmup",
               str(args.warmup), "--baseline-max", str(args.baseline_max)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")]
        if done.returncode != 0 or not lines:
            print("n=%5d  failed with status %d; nothing further is run" % (n, done.returncode), flush=True)
            return 1
        r = json.loads(lines[-1][len("RESULT "):])
        text = "n=%5d  %d cells  all_pairs_costs median %.4f s (min %.4f), %.3g ns per cell" % (n, r["cells"], r["all_pairs_median_s"], r["all_pairs_min_s"],
                                                                                               1e9 * r["all_pairs_median_s"] / r["cells"])
        if "ratio" in r:
            text += "; loop of %d dtw_batch calls median %.3f s (min %.3f): %.1fx; same bits: %s" % (n, r["dtw_batch_loop_median_s"], r["dtw_batch_loop_min_s"],
                                                                                                  r["ratio"], r["same_bits"])
        print(text + "; selected motion %d, mean cost %.4g (motion 0: %.4g)" % (r["selected"], r["least_mean_cost"], r["mean_cost_of_motion_0"]), flush=True)
        out["device"] = r.pop("device")
        out["results"].append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
