"""Latency of training a primitive's Gaussian mixture on the device against sklearn on the same host.

Device: HipGMMTrainer.fit (the 40-fit AIC sweep, one mg_gmm_em_fit call plus its k-means calls, then the refit), host wall
clock of a synchronised run, median of --reps after --warmup, on 'walk' latents (d = 40) drawn on the device.
sklearn: the same 41 fits (GaussianMixture(K, covariance_type='full') for K = 1 .. 40 on the shuffled rows, then the refit
of the chosen K), once with 1 thread and once with 16 (threadpoolctl), where sklearn imports; --sklearn-threads picks which.

    python tools/probes/gmm_train_latency.py [--sizes 1000,10000] [--reps 5] [--warmup 1] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from morphablegraphs_amd import _capi, synthetic  # noqa: E402
from morphablegraphs_amd import gmm_trainer as gt  # noqa: E402


def sklearn_sweep(X, threads):
    import warnings
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.mixture import GaussianMixture
    from threadpoolctl import threadpool_limits
    rng = np.random.RandomState(0)
    obs = rng.permutation(X)
    t0 = time.perf_counter()
    with threadpool_limits(threads), warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        aic = []
        for K in range(1, 41):
            aic.append(GaussianMixture(n_components=K, covariance_type='full', random_state=rng).fit(obs).aic(obs))
            print("  sklearn %2d threads K=%2d  %.1f s" % (threads, K, time.perf_counter() - t0), flush=True)
        K = int(np.argmin(aic)) + 1
        GaussianMixture(n_components=K, covariance_type='full', random_state=rng).fit(X).score(X)
    return time.perf_counter() - t0, K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="1000,10000")
    ap.add_argument("--sklearn-threads", default="1,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _capi.Context(0)
    data = synthetic.make_walk_primitive(seed=0)
    prim = _capi.Primitive(ctx, data)
    out = {"device": ctx.device_info()["name"], "reps": args.reps, "warmup": args.warmup, "results": []}
    for n in [int(s) for s in args.sizes.split(",")]:
        counts = np.random.default_rng(n).multinomial(n, np.asarray(data["gmm_weights"], dtype=np.float64))
        X = np.ascontiguousarray(prim.gmm_sample(counts, 7)[0][:, :40], dtype=np.float64)
        walls = []
        for rep in range(args.warmup + args.reps):
            np.random.seed(rep)
            tr = gt.HipGMMTrainer(seed=3, ctx=ctx)
            ctx.synchronize()
            t0 = time.perf_counter()
            tr.fit(X)
            ctx.synchronize()
            if rep >= args.warmup:
                walls.append(time.perf_counter() - t0)
        r = {"samples": n, "dim": 40, "device_median_s": float(np.median(walls)), "device_min_s": float(np.min(walls)),
             "device_chosen_K": tr.numberOfGaussian, "device_max_n_iter": int(max(g.n_iter_ for g in tr.sweep))}
        print("n=%6d  device  median %.3f s  (min %.3f)  chosen K %d" % (n, r["device_median_s"], r["device_min_s"], r["device_chosen_K"]), flush=True)
        try:
            import sklearn  # noqa: F401
            have = True
        except ImportError:
            have = False
        for th in ([int(t) for t in args.sklearn_threads.split(",") if t] if have else []):
            s, K = sklearn_sweep(X, th)
            r["sklearn_%d_threads_s" % th] = s
            r["sklearn_%d_threads_chosen_K" % th] = K
            print("n=%6d  sklearn %2d threads  %.3f s  chosen K %d  (%.1fx the device)" % (n, th, s, K, s / r["device_median_s"]), flush=True)
        out["results"].append(r)
    prim.close()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
