"""Latency of one scaled-fPCA gradient: the 3 + J + 1 objective values of SLSQP's forward difference from ONE mg_sfpca_errors call,
against the host statement (scaled_fpca.sfpca_errors_host: numpy.linalg.svd per weight vector, NumPy forward kinematics) on the
same machine.

    python tools/probes/sfpca_latency.py [--n 100 1000] [--runs 5] [--host-runs 1] [--out profiles/sfpca_latency.json]

Shape: n samples, n_basis = 31, D = 79 (J = 19), F = 156 canonical frames (step 1), npc = 10, all joints of a 19-joint binary-tree
skeleton with an end site per leaf.  Seeded data as tests/scaled_fpca_cases.py draws it.  Device: host wall clock around the call (it
synchronises), the median of --runs after one warm-up; mg_sfpca_create is timed apart (once per data set).  Host statement: the
median of --host-runs.  Prints one JSON line per n and writes them all to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from morphablegraphs_amd import _capi  # noqa: E402
from morphablegraphs_amd import scaled_fpca as sf  # noqa: E402
from morphablegraphs_amd.synthetic import cubic_b_spline_knots  # noqa: E402

N_BASIS, N_ANIMATED, N_FRAMES, NPC = 31, 19, 156, 10
N_DIMS = 3 + 4 * N_ANIMATED


def skeleton():
    rng = np.random.default_rng(5)
    names = ["j%d" % i for i in range(N_ANIMATED)]
    joints = [(names[i], None if i == 0 else names[(i - 1) // 2], (0.0, 0.0, 0.0) if i == 0 else tuple(rng.normal(0.0, 8.0, 3))) for i in range(N_ANIMATED)]
    leaves = [i for i in range(N_ANIMATED) if 2 * i + 1 >= N_ANIMATED]
    joints += [("end%d" % i, names[i], tuple(rng.normal(0.0, 8.0, 3))) for i in leaves]
    return _capi.Skeleton(joints, names)


def draw(n, seed=11):
    rng = np.random.default_rng(seed)
    mean = np.zeros((N_BASIS, N_DIMS))
    mean[:, :3] = np.linspace(0.0, 1.0, N_BASIS)[:, None] * rng.normal(0.0, 30.0, (1, 3))
    for j in range(N_ANIMATED):
        q = rng.normal(0.0, 1.0, 4) + np.array([2.0, 0.0, 0.0, 0.0])
        mean[:, 3 + 4 * j:7 + 4 * j] = q / np.linalg.norm(q)
    n_modes = 24
    modes = rng.normal(0.0, 1.0, (n_modes, N_BASIS, N_DIMS))
    modes[:, :, :3] *= 25.0
    modes[:, :, 3:] *= 0.12
    latents = rng.normal(0.0, 1.0, (n, n_modes)) * 0.85 ** np.arange(n_modes)
    noise = rng.normal(0.0, 0.01, (n, N_BASIS, N_DIMS))
    noise[:, :, :3] *= 50.0
    return np.ascontiguousarray(mean + np.tensordot(latents, modes, axes=1) + noise)


def median_seconds(fn, runs, warm_up):
    for _ in range(warm_up):
        fn()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfpca_latency.json"))
    args = ap.parse_args()
    from morphablegraphs_amd.motion_primitive import get_context
    ctx = get_context(0)
    sk = skeleton()
    knots = cubic_b_spline_knots(N_BASIS, N_FRAMES)
    joints = list(range(len(sk.names)))
    rows = []
    for n in args.n:
        coeffs = draw(n)
        t0 = time.perf_counter()
        obj = sf.HipScaledFunctionalPCA(coeffs, NPC, sk, knots, N_ANIMATED, joints=joints, ctx=ctx)
        create_s = time.perf_counter() - t0
        x = np.exp(np.random.default_rng(3).normal(0.0, 0.3, 3 + N_ANIMATED))
        pts, _ = sf.forward_difference_points(x)
        holder = {}

        def device():
            holder["device"] = obj.errors(pts)
        device_s, device_all = median_seconds(device, args.runs, 1)
        statuses = obj.pca_statuses_.tolist()

        def host():
            holder["host"] = sf.sfpca_errors_host(coeffs, pts, NPC, sk, obj.design, joints)
        row = {"probe": "sfpca_latency", "n": n, "n_basis": N_BASIS, "n_dims": N_DIMS, "n_frames": N_FRAMES, "npc": NPC, "points": len(pts),
               "joints_compared": len(joints), "create_s": create_s, "device_gradient_s": device_s, "device_runs_s": device_all,
               "statuses_converged": int(np.sum(np.array(statuses) == _capi.MG_PCA_CONVERGED))}
        if args.host_runs > 0:
            host_s, host_all = median_seconds(host, args.host_runs, 0)
            d = np.abs(holder["device"] - holder["host"])
            row.update({"host_gradient_s": host_s, "host_runs_s": host_all, "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0),
                        "host_over_device": host_s / device_s, "max_abs_difference": float(d.max()), "max_value": float(np.abs(holder["host"]).max())})
        obj.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
