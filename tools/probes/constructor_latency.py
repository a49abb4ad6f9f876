"""Latency of HipMotionModelConstructor.construct_model as a whole, and of the two kernels it adds.

New: HipMotionModelConstructor(...).construct_model(name) -- the captures' one upload, mg_align_motions_spatially, forward
kinematics, grids, paths and warp on the device table, mg_prepare_aligned_frames, spline fit, PCA, the temporal fPCA, the
mixture's AIC sweep, the dict.
Loose chain: align_motions_spatially_host (NumPy) -> dtw.align_frames_temporally -> fpca.construct_motion_primitive_model:
what a caller had to write before the class, the spatial alignment on the CPU, every stage uploading its input again.
Both with the same trainer; host wall clock of a synchronised run, median of --reps after --warmup, for N motions of 156 frames
+- 20 % with 19 joints (D = 79).  Kernels alone: spatial_alignment.align_motions_spatially / prepare_aligned_frames (upload,
launches, download) against their NumPy restatements on the same data.

    python tools/probes/constructor_latency.py [--sizes 100,1000] [--reps 5] [--warmup 1] [--out FILE.json]

profiles/constructor_latency.{json,log}: the command above with its defaults and --out.
"""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from morphablegraphs_amd import _capi, dtw, fpca, spatial_alignment as sa  # noqa: E402
from morphablegraphs_amd.motion_model_constructor import HipMotionModelConstructor  # noqa: E402

F, J = 156, 19
CONFIG = {"n_spatial_basis_factor": 0.25, "n_components": None, "fraction": 0.95, "n_basis_functions_temporal": 8, "npc_temporal": None,
          "precision_temporal": 0.99}


def skeleton():
    """19 joints: a spine of 5, two arms of 4, two legs of 3; all animated."""
    joints = [("j0", None, (0.0, 0.0, 0.0))]
    for chain, parent, offset in (("spine", "j0", (0.0, 0.2, 0.0)), ("larm", "spine2", (0.2, 0.05, 0.0)), ("rarm", "spine2", (-0.2, 0.05, 0.0)),
                                  ("lleg", "j0", (0.1, -0.4, 0.0)), ("rleg", "j0", (-0.1, -0.4, 0.0))):
        for i in range({"spine": 4, "larm": 4, "rarm": 4, "lleg": 3, "rleg": 3}[chain]):
            joints.append(("%s%d" % (chain, i), parent if i == 0 else "%s%d" % (chain, i - 1), offset))
    assert len(joints) == J
    return _capi.Skeleton(joints, [j[0] for j in joints])


def captures(n, seed=0):
    rng = np.random.default_rng(seed)
    amp, freq, phase = rng.uniform(0.1, 0.5, (J, 3)), rng.uniform(0.6, 1.6, (J, 3)), rng.uniform(0, 2 * np.pi, (J, 3))
    out = collections.OrderedDict()
    for i in range(n):
        length = F if i == 0 else int(rng.integers(int(0.8 * F), int(1.2 * F) + 1))
        steps = np.exp(0.05 * np.cumsum(rng.standard_normal(length - 1)))
        t = np.concatenate([[0.0], np.cumsum(steps)])
        t /= t[-1]
        frames = np.zeros((length, 3 + 4 * J))
        yaw, shift = rng.uniform(-np.pi, np.pi), rng.uniform(-3.0, 3.0, 2)
        x, z = 0.4 * np.sin(np.pi * t), 2.0 * t
        frames[:, 0] = np.cos(yaw) * x + np.sin(yaw) * z + shift[0]
        frames[:, 1] = 0.9 + 0.04 * np.sin(4 * np.pi * t)
        frames[:, 2] = -np.sin(yaw) * x + np.cos(yaw) * z + shift[1]
        aa = amp[None] * np.sin(2 * np.pi * freq[None] * t[:, None, None] + phase[None]) + 0.01 * rng.standard_normal((length, J, 3))
        aa[:, 0, 1] += yaw
        ang = np.linalg.norm(aa, axis=2)
        q = np.concatenate([np.cos(ang / 2)[..., None], aa / np.maximum(ang, 1e-12)[..., None] * np.sin(ang / 2)[..., None]], axis=2)
        frames[:, 3:] = q.reshape(length, -1)
        out["m%04d" % i] = frames
    return out


def timed(ctx, fn, reps, warmup):
    walls = []
    for rep in range(warmup + reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        if rep >= warmup:
            walls.append(time.perf_counter() - t0)
    return float(np.median(walls)), float(np.min(walls))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="100,1000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _capi.Context(0)
    sk = skeleton()
    out = {"device": ctx.device_info()["name"], "reps": args.reps, "warmup": args.warmup, "frames": F, "joints": J, "results": []}
    for n in [int(s) for s in args.sizes.split(",")]:
        motions = captures(n)

        def new():
            c = HipMotionModelConstructor(sk, CONFIG, ctx=ctx, frame_time=1.0 / 30)
            c.set_motions(motions)
            return c.construct_model("probe")

        def loose():
            aligned = sa.align_motions_spatially_host(motions)
            warped, warps = dtw.align_frames_temporally(sk, sk.names, aligned, ctx=ctx)
            return fpca.construct_motion_primitive_model(warped, warps, CONFIG, animated_joints=sk.animated_joints, name="probe", frame_time=1.0 / 30, ctx=ctx)

        r = {"motions": n, "frames_total": int(sum(len(m) for m in motions.values()))}
        for name, fn in (("constructor", new), ("loose_chain", loose)):
            r[name + "_median_s"], r[name + "_min_s"] = timed(ctx, fn, args.reps, args.warmup)
            print("n=%5d  %-12s median %.4f s (min %.4f)" % (n, name, r[name + "_median_s"], r[name + "_min_s"]), flush=True)
        aligned = sa.align_motions_spatially_host(motions)
        equal = collections.OrderedDict((k, m[:int(0.8 * F)]) for k, m in aligned.items())
        for name, fn in (("align_device", lambda: sa.align_motions_spatially(motions, ctx=ctx)), ("align_numpy", lambda: sa.align_motions_spatially_host(motions)),
                         ("prepare_device", lambda: sa.prepare_aligned_frames(equal, ctx=ctx)), ("prepare_numpy", lambda: sa.prepare_aligned_frames_host(equal))):
            r[name + "_median_s"], r[name + "_min_s"] = timed(ctx, fn, args.reps, args.warmup)
            print("n=%5d  %-14s median %.5f s (min %.5f)" % (n, name, r[name + "_median_s"], r[name + "_min_s"]), flush=True)
        out["results"].append(r)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
