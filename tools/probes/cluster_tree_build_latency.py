"""End-to-end latency of building the reference's cluster trees on the device: per build, host wall clock
from the call to the finished tree on the host (every mg_kmeans_segments call synchronises), median over --reps builds after
--warmup, on samples of the 'walk' primitive (L = 40) drawn on the device, at 10^4 and 10^5 samples:

  kd        build_kd_cluster_tree, 4 subdivisions x 4 levels, k-means on all 40 dimensions, KD trees below
  feature   build_feature_cluster_tree, 4 subdivisions, features = data (HipClusterTreeBuilder's latent features)

and the share of the k-means calls in it (host wall clock around each mg_kmeans_segments call, summed per build), the
k-means calls (= levels that cluster), their segments and their Lloyd launches' upper bound (the deepest iteration count).

    python tools/probes/cluster_tree_build_latency.py [--reps 5] [--warmup 1] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from morphablegraphs_amd import _capi, synthetic  # noqa: E402
from morphablegraphs_amd import cluster_tree_builder as ctb  # noqa: E402


class _Timed(object):
    """DeviceKMeans with the host wall clock of every call recorded."""

    def __init__(self, ctx, X, k, seed):
        self.km = ctb.DeviceKMeans(ctx, X, k, seed=seed)
        self.seconds, self.calls, self.segments, self.max_iter = 0.0, 0, 0, 0

    def __call__(self, seg_begin, rows, node_ids):
        t0 = time.perf_counter()
        labels = self.km(seg_begin, rows, node_ids)
        self.seconds += time.perf_counter() - t0
        self.calls += 1
        self.segments += len(seg_begin) - 1
        self.max_iter = max(self.max_iter, int(self.km.last["n_iter"].max()))
        return labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _capi.Context(0)
    data = synthetic.make_walk_primitive(seed=0)
    prim = _capi.Primitive(ctx, data)
    out = {"device": ctx.device_info()["name"], "reps": args.reps, "warmup": args.warmup, "results": []}
    for n in [int(s) for s in args.sizes.split(",")]:
        counts = np.random.default_rng(n).multinomial(n, np.asarray(data["gmm_weights"], dtype=np.float64))
        X = np.ascontiguousarray(prim.gmm_sample(counts, 7)[0][:, :40], dtype=np.float64)
        for kind in ("kd", "feature"):
            walls, shares, info = [], [], None
            for rep in range(args.warmup + args.reps):
                km = _Timed(ctx, X, 4, 11)
                t0 = time.perf_counter()
                if kind == "kd":
                    tree = ctb.build_kd_cluster_tree(X, 4, 4, kmeans=km)
                else:
                    tree = ctb.build_feature_cluster_tree(X, X, 4, kmeans=km)
                wall = time.perf_counter() - t0
                km.km.close()
                if rep >= args.warmup:
                    walls.append(wall)
                    shares.append(km.seconds / wall)
                info = {"nodes": int(tree.n_nodes), "depth": int(np.max(tree.depth)), "kmeans_calls": km.calls, "segments": km.segments,
                        "max_lloyd_iterations": km.max_iter, "kmeans_ms": km.seconds * 1e3}
            r = dict(info, kind=kind, samples=n, median_ms=float(np.median(walls) * 1e3), min_ms=float(np.min(walls) * 1e3),
                     kmeans_share=float(np.median(shares)))
            out["results"].append(r)
            print("%-8s n=%6d  median %8.1f ms  (min %8.1f)  k-means %4.0f %%  %5d nodes  depth %2d  %2d calls  %5d segments  <= %3d iterations"
                  % (kind, n, r["median_ms"], r["min_ms"], 100 * r["kmeans_share"], r["nodes"], r["depth"], r["kmeans_calls"], r["segments"],
                     r["max_lloyd_iterations"]), flush=True)
    prim.close()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
