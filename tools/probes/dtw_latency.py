"""Latency of the batched exact DTW on the device against two CPU yardsticks on the same host.

Device: dtw.find_optimal_dtw(point_clouds, mean_key) -- upload of the clouds, distance grids, accumulated cost and
back-tracking, download, the paths as Python lists -- host wall clock of a synchronised run, median of --reps after
--warmup, for N motions of about 156 frames (+- 20 %) of 19 joints against a reference motion of 156 frames.
CPU, the reference's run_dtw shape: one Python call of the cell distance per cell (the NumPy closed-form fit and the mean
point distance, as tools/gen_dtw_golden.py hands it to the reference), then the Python recurrence and back-tracking
(dtw_paths_host).  Measured on --cpu-pairs pairs, one core, and EXTRAPOLATED to N pairs (N = 1000 would run for an hour).
CPU, the honest alternative: distance_grid_host (NumPy, vectorised over the grid) + dtw_paths_host per pair, the same way.

    python tools/probes/dtw_latency.py [--sizes 100,1000] [--reps 5] [--warmup 1] [--cpu-pairs 3] [--no-cpu] [--out FILE.json]

profiles/dtw_latency.{json,log}: the command above with its defaults and --out.  profiles/dtw_kernel_stats.csv: a run of
its own, N = 1000, no warm-up:

    rocprofv3 --kernel-trace --stats -d DIR -o dtw --output-format csv -- \\
        python tools/probes/dtw_latency.py --no-cpu --sizes 1000 --reps 1 --warmup 0
"""
import argparse
import collections
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from morphablegraphs_amd import _capi, dtw  # noqa: E402

F, J = 156, 19
FLOP_PER_CELL_JOINT = 20      # per joint of a cell: the two cross sums (8), the transform and the distance (12, the square root as one)


def clouds(n, seed=0):
    rng = np.random.default_rng(seed)
    rest = rng.uniform(-0.5, 0.5, (J, 3)) * np.array([0.6, 1.8, 0.4]) + np.array([0.0, 0.9, 0.0])
    amp, phase = rng.uniform(0.05, 0.35, (J, 3)), rng.uniform(0, 2 * np.pi, (J, 3))

    def motion(length, warp):
        t = np.linspace(0.0, 1.0, length)
        if warp:
            steps = np.exp(0.2 * np.cumsum(rng.standard_normal(length - 1)) * 0.25)
            t = np.concatenate([[0.0], np.cumsum(steps)])
            t /= t[-1]
        pos = rest[None] + amp[None] * np.sin(2 * np.pi * 1.5 * t[:, None, None] + phase[None])
        pos[:, :, 2] += 2.4 * t[:, None]
        return pos + 0.004 * rng.standard_normal(pos.shape)
    out = collections.OrderedDict([("ref", motion(F, False))])
    for i in range(n - 1):
        out["m%04d" % i] = motion(int(rng.integers(int(0.8 * F), int(1.2 * F) + 1)), True)
    return out


def cell_distance(a, b):
    """The closed-form fit and the mean point distance, one cell (what the reference's loop calls Fr x F times)."""
    sax, saz, sbx, sbz, sw = a[:, 0].sum(), a[:, 2].sum(), b[:, 0].sum(), b[:, 2].sum(), float(len(a))
    num = (a[:, 0] * b[:, 2] - b[:, 0] * a[:, 2]).sum() - (sax * sbz - sbx * saz) / sw
    den = (a[:, 0] * b[:, 0] + a[:, 2] * b[:, 2]).sum() - (sax * sbx + saz * sbz) / sw
    theta = math.atan2(num, den)
    c, s = math.cos(theta), math.sin(theta)
    ox, oz = (sax - sbx * c - sbz * s) / sw, (saz + sbx * s - sbz * c) / sw
    fitted = b.copy()
    fitted[:, 0] = b[:, 0] * c + b[:, 2] * s + ox
    fitted[:, 2] = -b[:, 0] * s + b[:, 2] * c + oz
    return float(np.linalg.norm(a - fitted, axis=1).sum() / len(b))


def cpu_pairs(pc, n_pairs):
    keys = list(pc.keys())[1:1 + n_pairs]
    ref = pc["ref"]
    t0 = time.perf_counter()
    for k in keys:
        S = np.array([[cell_distance(x, y) for y in pc[k]] for x in ref])
        dtw.dtw_paths_host(S)
    t1 = time.perf_counter()
    for k in keys:
        dtw.dtw_paths_host(dtw.distance_grid_host(ref, pc[k]))
    t2 = time.perf_counter()
    return (t1 - t0) / len(keys), (t2 - t1) / len(keys)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="100,1000")
    ap.add_argument("--cpu-pairs", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _capi.Context(0)
    out = {"device": ctx.device_info()["name"], "reps": args.reps, "warmup": args.warmup, "frames": F, "joints": J, "results": []}
    for n in [int(s) for s in args.sizes.split(",")]:
        pc = clouds(n)
        cells = sum(F * len(c) for c in pc.values())
        walls = []
        for rep in range(args.warmup + args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            paths = dtw.find_optimal_dtw(pc, "ref", ctx=ctx)
            ctx.synchronize()
            if rep >= args.warmup:
                walls.append(time.perf_counter() - t0)
        r = {"motions": n, "cells": cells, "grid_flop": cells * J * FLOP_PER_CELL_JOINT, "grid_bytes_stored": cells * 8,
             "device_median_s": float(np.median(walls)), "device_min_s": float(np.min(walls)), "mean_path_length": float(np.mean([len(p) for p in paths.values()]))}
        print("n=%5d  %d cells  device median %.4f s (min %.4f)  mean path length %.1f" % (n, cells, r["device_median_s"], r["device_min_s"], r["mean_path_length"]),
              flush=True)
        if not args.no_cpu:
            per_ref, per_np = cpu_pairs(pc, args.cpu_pairs)
            r.update({"cpu_pairs_measured": args.cpu_pairs, "cpu_reference_shape_s_per_pair": per_ref, "cpu_reference_shape_s_extrapolated": per_ref * n,
                      "cpu_numpy_grid_s_per_pair": per_np, "cpu_numpy_grid_s_extrapolated": per_np * n})
            print("n=%5d  CPU one core, %d pairs measured, extrapolated to %d: reference's loop shape %.3f s/pair -> %.1f s (%.0fx the device); "
                  "NumPy grid + Python recurrence %.4f s/pair -> %.2f s (%.1fx)" % (n, args.cpu_pairs, n, per_ref, per_ref * n, per_ref * n / r["device_median_s"],
                                                                                   per_np, per_np * n, per_np * n / r["device_median_s"]), flush=True)
        out["results"].append(r)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
