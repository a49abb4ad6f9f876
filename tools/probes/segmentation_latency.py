"""Latency of the batched keyframe search on the device against the NumPy restatement on the same host.

Device: Segmentation.extract_segments(captures, start_keyframe, end_keyframe, threshold) on point clouds -- concatenation and
upload of the clouds, the distances of every frame to both keyframes, the search, download of the pairs, the slices as views
-- host wall clock of a synchronised run, median of --reps after --warmup, for N captures of about 3000 frames (+- 10 %) of 19
joints; every capture repeats a cyclic pose sequence of about 400 frames.
CPU: keyframe_distances_host (NumPy, vectorised over a capture's frames) + segment_search_host (plain Python) per capture, one
core.  Measured on --cpu-captures captures and EXTRAPOLATED linearly to N (the captures are independent).

    python tools/probes/segmentation_latency.py [--sizes 100,1000] [--reps 5] [--warmup 1] [--cpu-captures 5] [--no-cpu] [--out FILE.json]

profiles/segmentation_latency.{json,log}: the command above with its defaults and --out.  profiles/segmentation_kernel_stats.csv:
a run of its own, N = 1000, no warm-up:

    rocprofv3 --kernel-trace --stats -d DIR -o segmentation --output-format csv -- \\
        python tools/probes/segmentation_latency.py --no-cpu --sizes 1000 --reps 1 --warmup 0
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from morphablegraphs_amd import _capi  # noqa: E402
from morphablegraphs_amd import segmentation as seg  # noqa: E402

F, J, PERIOD = 3000, 19, 400.0
THRESHOLD, MIN_SEGMENT_SIZE = 0.01, 10
FLOP_PER_CELL_JOINT = 20      # as tools/probes/dtw_latency.py counts a cell


def captures(n, seed=0):
    rng = np.random.default_rng(seed)
    rest = rng.uniform(-0.5, 0.5, (J, 3)) * np.array([0.6, 1.8, 0.4]) + np.array([0.0, 0.9, 0.0])
    amp, phase = rng.uniform(0.05, 0.35, (J, 3)), rng.uniform(0, 2 * np.pi, (J, 3))

    def pose(t):
        return rest[None] + amp[None] * np.sin(2 * np.pi * t[:, None, None] + phase[None])
    out = []
    for _ in range(n):
        length = int(rng.integers(int(0.9 * F), int(1.1 * F) + 1))
        t = np.arange(length) / (PERIOD * rng.uniform(0.9, 1.1)) + rng.uniform(0.0, 1.0)
        pos = pose(t)
        pos[:, :, 2] += 1.2 * t[:, None]
        out.append(pos + 0.004 * rng.standard_normal(pos.shape))
    keys = pose(np.array([0.15, 0.70]))
    return out, keys[0], keys[1]


def cpu_captures(clouds, start, end, n):
    t0 = time.perf_counter()
    found = 0
    for c in clouds[:n]:
        d = seg.keyframe_distances_host([c], np.stack([start, end]))[0]
        found += len(seg.segment_search_host(d[0], d[1], seg.MULTI, THRESHOLD, MIN_SEGMENT_SIZE))
    return (time.perf_counter() - t0) / n, found / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="100,1000")
    ap.add_argument("--cpu-captures", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _capi.Context(0)
    out = {"device": ctx.device_info()["name"], "reps": args.reps, "warmup": args.warmup, "frames": F, "joints": J, "threshold": THRESHOLD,
           "min_segment_size": MIN_SEGMENT_SIZE, "results": []}
    sg = seg.Segmentation(None, min_segment_size=MIN_SEGMENT_SIZE, ctx=ctx)
    for n in [int(s) for s in args.sizes.split(",")]:
        clouds, start, end = captures(n)
        frames = sum(len(c) for c in clouds)
        walls = []
        for rep in range(args.warmup + args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            slices = sg.extract_segments(clouds, start, end, THRESHOLD)
            ctx.synchronize()
            if rep >= args.warmup:
                walls.append(time.perf_counter() - t0)
        r = {"captures": n, "frames": frames, "cloud_bytes_uploaded": frames * J * 24, "distance_flop": 2 * frames * J * FLOP_PER_CELL_JOINT,
             "device_median_s": float(np.median(walls)), "device_min_s": float(np.min(walls)), "segments_per_capture": len(slices) / n}
        print("n=%5d  %d frames  device median %.4f s (min %.4f)  %.2f segments per capture" % (n, frames, r["device_median_s"], r["device_min_s"],
                                                                                                r["segments_per_capture"]), flush=True)
        if not args.no_cpu:
            per, found = cpu_captures(clouds, start, end, min(args.cpu_captures, n))
            r.update({"cpu_captures_measured": min(args.cpu_captures, n), "cpu_numpy_s_per_capture": per, "cpu_numpy_s_extrapolated": per * n,
                      "cpu_segments_per_capture": found})
            print("n=%5d  CPU one core, NumPy restatement, %d captures measured, extrapolated to %d: %.4f s/capture -> %.2f s (%.1fx the device)" % (
                n, r["cpu_captures_measured"], n, per, per * n, per * n / r["device_median_s"]), flush=True)
        out["results"].append(r)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
