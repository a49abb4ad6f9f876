"""Latency of the functional PCA of aligned motions on the device against the reference-shaped CPU path on
the same host.

Device: HipPCAFunctionalData(motions, n_basis, fraction) -- upload, spline fit, centring, Jacobi PCA, projection, download
-- host wall clock of a synchronised run, median of --reps after --warmup, on synthetic motions (F = 156, D = 79,
n_basis = 31); and a temporal fit (HipFPCATimeSemantic.functional_pca, n_basis = 8).
CPU: what the reference does, once, with 16 threads (threadpoolctl): scipy splrep per motion and channel on the reference's
knots, centring, scipy.sparse.linalg.svds(A, k = min(A.shape) - 1), projection.

    python tools/probes/fpca_latency.py [--sizes 100,1000] [--reps 5] [--warmup 1] [--no-cpu] [--out FILE.json]

profiles/fpca_latency.{json,log}: the command above with its defaults and --out.  profiles/fpca_kernel_stats.csv: a run of
its own, one spatial fit at N = 1000 and the temporal fit, no warm-up:

    rocprofv3 --kernel-trace --stats -d DIR -o fpca --output-format csv -- \
        python tools/probes/fpca_latency.py --no-cpu --sizes 1000 --reps 1 --warmup 0
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from morphablegraphs_amd import _capi, fpca  # noqa: E402

F, D, NB = 156, 79, 31


def motions(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, F)
    modes = np.stack([np.sin((k + 1) * np.pi * t + 0.3 * k) for k in range(12)])
    mix = rng.standard_normal((12, D))
    latent = rng.standard_normal((n, 12)) * (0.7 ** np.arange(12))
    return np.einsum("nk,kf,kd->nfd", latent, modes, mix) + 0.02 * rng.standard_normal((n, F, D))


def warps(n, seed=1):
    rng = np.random.default_rng(seed)
    steps = np.exp(0.2 * rng.standard_normal((n, F - 1)))
    w = np.concatenate([np.zeros((n, 1)), np.cumsum(steps, axis=1)], axis=1)
    return w / w[:, -1:] * (F - 1)


def cpu_path(X, n_basis, fraction):
    import scipy.interpolate as si
    from scipy.sparse.linalg import svds
    from threadpoolctl import threadpool_limits
    knots = fpca.cubic_b_spline_knots(n_basis, X.shape[1])
    x = list(range(X.shape[1]))
    t0 = time.perf_counter()
    with threadpool_limits(16):
        fd = np.zeros((X.shape[0], n_basis, X.shape[2]))
        for i in range(X.shape[0]):
            fd[i] = np.asarray([si.splrep(x, X[i][:, d], k=3, t=knots[4:-4])[1][:-4] for d in range(X.shape[2])]).T
        t1 = time.perf_counter()
        A = fd.reshape(X.shape[0], -1)
        A = A - A.mean(axis=0)
        _, s, Vt = svds(A, max(1, min(A.shape) - 1))
        order = np.argsort(s)[::-1]
        s, Vt = s[order], Vt[order]
        var = np.cumsum(s ** 2) / np.sum(s ** 2)
        npc = int(np.searchsorted(var, fraction) + 1)
        low = A @ Vt[:npc].T
    t2 = time.perf_counter()
    return t2 - t0, t1 - t0, npc, low.shape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="100,1000")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _capi.Context(0)
    out = {"device": ctx.device_info()["name"], "reps": args.reps, "warmup": args.warmup, "results": []}
    for n in [int(s) for s in args.sizes.split(",")]:
        X = motions(n)
        walls = []
        for rep in range(args.warmup + args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            obj = fpca.HipPCAFunctionalData(X, n_basis=NB, fraction=0.95, ctx=ctx)
            ctx.synchronize()
            if rep >= args.warmup:
                walls.append(time.perf_counter() - t0)
            sweeps, status, npc = obj.n_sweeps_, obj.pca_status_, obj.npc_
            obj.close()
        r = {"kind": "spatial", "samples": n, "frames": F, "dims": D, "n_basis": NB, "device_median_s": float(np.median(walls)),
             "device_min_s": float(np.min(walls)), "sweeps": sweeps, "status": status, "npc": npc}
        print("spatial  n=%5d  device median %.3f s (min %.3f)  %d sweeps  npc %d" % (n, r["device_median_s"], r["device_min_s"], sweeps, npc), flush=True)
        if not args.no_cpu:
            total, spl, cnpc, _ = cpu_path(X, NB, 0.95)
            r.update({"cpu_16_threads_s": total, "cpu_splrep_s": spl, "cpu_npc": cnpc})
            print("spatial  n=%5d  CPU 16 threads %.3f s (splrep %.3f)  npc %d  (%.1fx the device)" % (n, total, spl, cnpc, total / r["device_median_s"]),
                  flush=True)
        out["results"].append(r)
    n = 1000
    W = warps(n)
    walls = []
    for rep in range(args.warmup + args.reps):
        ft = fpca.HipFPCATimeSemantic(8, precision_temporal=0.99, ctx=ctx)
        ft.temporal_semantic_data = W
        ctx.synchronize()
        t0 = time.perf_counter()
        ft.functional_pca()
        ctx.synchronize()
        if rep >= args.warmup:
            walls.append(time.perf_counter() - t0)
    r = {"kind": "temporal", "samples": n, "frames": F, "n_basis": 8, "device_median_s": float(np.median(walls)), "device_min_s": float(np.min(walls)),
         "sweeps": ft.n_sweeps_, "status": ft.pca_status_, "npc": int(ft.npc)}
    print("temporal n=%5d  device median %.4f s (min %.4f)  %d sweeps  npc %d" % (n, r["device_median_s"], r["device_min_s"], ft.n_sweeps_, ft.npc), flush=True)
    out["results"].append(r)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
