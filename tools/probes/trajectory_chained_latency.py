"""Probe: (1) mg_score_trajectory_chained against mg_score_trajectory for the same shape -- 4096 candidates of the path-following
'walk' primitive (L = 40, F = 156, D = 79), one Catmull-Rom path, both searches: the event-bracketed kernel time (profile slot
"trajectory"), the two entry points taking turns inside one process, one warm-up each, the median and interquartile range of REPS
launches; (2) the three-step one-launch objective (HipGraphWalkObjective.residual_vector) with a root trajectory on steps 2 and 3
and without: wall clock of a synchronised evaluation, taking turns likewise.  Where two medians differ by less than the larger
spread the verdict is "no difference", not a ratio.
usage: python tools/probes/trajectory_chained_latency.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from morphablegraphs_amd import _capi, synthetic  # noqa: E402
from morphablegraphs_amd import objective_functions as of  # noqa: E402

REPS = 15
N = 4096
L, F, D = 40, 156, 79

ctx = _capi.Context(0)
prim = _capi.Primitive(ctx, synthetic.make_path_following_primitive(seed=0))
t = np.linspace(0.0, 1.0, 7)
cps = np.stack([166.0 * t, 90.0 + 2.0 * np.sin(6.0 * t), 40.0 * np.sin(2.0 * t) - 4.0 * t], axis=-1)
traj = _capi.Trajectory(prim, cps, 1000)
S = np.random.default_rng(0).standard_normal((N, L))
record = {"joint": 0, "position": (0.0, 0.0, 0.0), "heading": (0.0, 1.0), "ref_dir": (0.0, 0.0, 1.0)}
align = np.tile([0.0, 1.0, 0.0, 0.0], (N, 1))
d_S, d_A, d_e, d_e2 = ctx.upload(S), ctx.upload(align), ctx.malloc(8 * N), ctx.malloc(8 * N)


def quartiles(v):
    return [float(x) for x in np.percentile(v, [25, 50, 75])]


def verdict(a, b, name_b):
    (a25, a50, a75), (b25, b50, b75) = a, b
    spread = max(a75 - a25, b75 - b25)
    if abs(a50 - b50) < spread:
        return "no difference"
    return "%s x%.3f %s" % (name_b, max(a50, b50) / min(a50, b50), "slower" if b50 > a50 else "faster")


results = {"device": ctx.device_info()["name"], "n": N, "reps": REPS, "kernel": [], "objective": []}
for search in (0, 1):
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
    plan = ctx.trajectory_plan(L, 3 * 31 + 4, len(cps) - 1, N)
    single = lambda: prim.score_trajectory_dev(traj, d_S, S.dtype, N, L, d_e, 0.0, 1.0, record)
    chained = lambda: prim.score_trajectory_chained_dev(traj, d_S, S.dtype, N, L, d_A, record, d_e2)
    single(), chained()
    ctx.synchronize()
    same = bool(np.array_equal(ctx.download(d_e, (N,), np.uint64), ctx.download(d_e2, (N,), np.uint64)))
    ctx.profile_enable(1)
    ctx.profile_reset()
    for _ in range(REPS):            # interleaved: samples 0, 2, 4 ... are the single-record launch's
        single()
        chained()
    ctx.synchronize()
    samples = 1e3 * ctx.profile_samples("trajectory")
    ctx.profile_enable(0)
    assert len(samples) == 2 * REPS, len(samples)
    a, b = quartiles(samples[0::2]), quartiles(samples[1::2])
    row = {"search": search, "kernel": plan["kernel"], "single_us": a[1], "single_iqr_us": a[2] - a[0], "chained_us": b[1], "chained_iqr_us": b[2] - b[0],
           "same_bits": same, "verdict": verdict(a, b, "chained")}
    results["kernel"].append(row)
    print("search %d (%s): single record %8.1f us (iqr %.1f) | chained %8.1f us (iqr %.1f) | %s | same bits: %s" % (
        search, plan["kernel"], a[1], a[2] - a[0], b[1], b[2] - b[0], row["verdict"], same), flush=True)
ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)


class _Skeleton(object):
    aligning_root_node, aligning_root_dir, root = "Hips", (0.0, 0.0, 1.0), "Hips"


class _Constraints(object):
    def __init__(self, cons):
        self.constraints, self.is_local, self.hip_skeleton, self.skeleton, self.start_pose, self.evaluations = cons, False, None, _Skeleton(), None, 0


class _Step(object):
    def __init__(self, cons):
        self.node_key, self.parameters, self.n_spatial_components, self.n_time_components, self.motion_primitive_constraints = "walk", np.zeros(L), L, 0, cons


class _Graph(object):
    nodes, skeleton, hip_skeleton = {"walk": prim}, _Skeleton(), None


def steps(with_trajectories):
    out = []
    for i in range(3):
        cons = [{"type": "position", "t": F - 1.0, "weight": 1.0, "target": [150.0 * (i + 1), None, 10.0 * i]}]
        if with_trajectories and i > 0:
            cons.append({"type": "trajectory", "control_points": (cps * [3.0, 1.0, 1.0]).tolist(), "min_u": 0.0, "weight": 1.0, "granularity": 1000})
        out.append(_Step(_Constraints(cons)))
    return out


def timed(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0)


prev = np.concatenate(([0.0, 90.0, 0.0], np.tile([1.0, 0.0, 0.0, 0.0], (D - 3) // 4)))[None, :]
plain, with_t = of.HipGraphWalkObjective(_Graph(), steps(False), prev), of.HipGraphWalkObjective(_Graph(), steps(True), prev)
for n in (1, 3 * L + 1, N):
    X = 0.7 * np.random.default_rng(n).standard_normal((n, 3 * L))
    f0, f1 = (lambda: plain.residual_vector(X, 2.0)), (lambda: with_t.residual_vector(X, 2.0))
    f0(), f1()
    t0, t1 = [], []
    for _ in range(REPS):
        t0.append(timed(f0))
        t1.append(timed(f1))
    a, b = quartiles(t0), quartiles(t1)
    row = {"n": n, "without_ms": a[1], "without_iqr_ms": a[2] - a[0], "with_ms": b[1], "with_iqr_ms": b[2] - b[0], "verdict": verdict(a, b, "with trajectories")}
    results["objective"].append(row)
    print("three steps, n %4d: without trajectories %8.3f ms (iqr %.3f) | with two %8.3f ms (iqr %.3f) | %s" % (
        n, a[1], a[2] - a[0], b[1], b[2] - b[0], row["verdict"]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(results, f, indent=1)
