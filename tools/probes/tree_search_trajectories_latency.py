"""Latency of a planner step over 16 cluster-tree options, each with a keyframe constraint and its own root trajectory
constraint, at the walk primitive's shape (L = 40, F = 156), two ways:

  one_launch   HipMotionStateGraph.evaluate_options(use_cluster_trees=True): the 16 descents side by side in ONE
               mg_cluster_tree_search_trajectories launch, the trajectories scored inside it, one read-back
  descent      the host-driven descent option by option (search_best_sample_batched, what such a step took before): per tree
               level one mg_score_constraints launch, one mg_score_trajectory launch, one read-back

in both closest-point searches (MG_OPT_TRAJECTORY_SEARCH 0: the reference's L-BFGS-B, 1: the monotone walk).  A step's time is
the host clock from the call to the results on the host (both ways end in a read-back, a synchronisation), median over --reps
steps after warm-up, the two ways alternating; kernel_ms is the one launch's own time from the device events of profile slot 11.
The two ways must return the same samples and errors, which is checked first.

    python tools/probes/tree_search_trajectories_latency.py [--reps 10] [--samples 2000] [--options 16] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from morphablegraphs_amd import _capi, candidate_scoring, synthetic  # noqa: E402
from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree  # noqa: E402
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraph, HipMotionStateGraphNode  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--options", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _capi.Context(0)
    graph = HipMotionStateGraph(context=ctx)
    options, cons, depths = [], {}, []
    for p in range(args.options):
        node = HipMotionStateGraphNode(context=ctx)
        node.init_from_dict("walk", {"name": "walk%d" % p, "mm": synthetic.make_walk_primitive(seed=p)})
        L = node.get_n_spatial_components()
        samples = np.random.default_rng(p).standard_normal((args.samples, L))
        node.cluster_tree = HipFeatureClusterTree.from_json(synthetic.make_feature_cluster_tree(samples, 4, seed=p), L)
        depths.append(int(node.cluster_tree.depth.max()))
        key = ("walk", "walk%d" % p)
        graph.nodes[key] = node
        options.append(key)
        prim = node.motion_primitive._prim
        path = np.asarray(prim.back_project_frames(np.zeros((1, L), dtype=np.float32)), dtype=np.float64)[0, :, :3]
        pts = path[np.linspace(0, len(path) - 1, 8).round().astype(int)] + np.random.default_rng(100 + p).uniform(-5.0, 5.0, (8, 3))
        cons[key] = [{"type": "position", "t": float(node.get_n_canonical_frames() - 1), "weight": 1.0, "target": [float(pts[-1][0]), None, float(pts[-1][2])]},
                     {"type": "trajectory", "control_points": pts.tolist(), "min_u": 0.0, "weight": 1.0, "granularity": 1000}]
    print("options %d, samples per tree %d, tree depths %s" % (len(options), args.samples, depths))

    def one_launch():
        return graph.evaluate_options(options, cons, 0, use_cluster_trees=True)[1]

    def descent():
        return {key: graph.nodes[key].search_best_sample_batched(cons[key], 1)[::-1] for key in options}

    out = {"options": len(options), "samples": args.samples, "reps": args.reps, "depths": depths, "modes": {}}
    for search, name in ((0, "lbfgsb"), (1, "walk")):
        ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
        a, b = one_launch(), descent()
        for key in options:
            assert np.array_equal(a[key][0], b[key][0]) and a[key][1] == b[key][1], "the two ways disagree on %r" % (key,)
        for _ in range(args.warmup):
            one_launch()
            descent()
        t_one, t_desc = [], []
        for _ in range(args.reps):          # alternating: both see the same machine
            t0 = time.perf_counter()
            one_launch()
            t1 = time.perf_counter()
            descent()
            t2 = time.perf_counter()
            t_one.append(t1 - t0)
            t_desc.append(t2 - t1)
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(max(args.reps // 2, 1)):
            one_launch()
        ms, launches = ctx.profile_get("cluster_tree_search")
        ctx.profile_enable(False)
        row = {"one_launch_ms": 1e3 * float(np.median(t_one)), "one_launch_min_ms": 1e3 * float(np.min(t_one)), "one_launch_max_ms": 1e3 * float(np.max(t_one)),
               "descent_ms": 1e3 * float(np.median(t_desc)), "descent_min_ms": 1e3 * float(np.min(t_desc)), "descent_max_ms": 1e3 * float(np.max(t_desc)),
               "kernel_ms": ms / max(launches, 1), "launches_per_step": launches / max(args.reps // 2, 1)}
        out["modes"][name] = row
        print("%-7s one launch %9.2f ms [%.2f .. %.2f] (kernel %.2f ms, %.0f launch per step)   descent %9.2f ms [%.2f .. %.2f]   ratio %.1f" % (
            name, row["one_launch_ms"], row["one_launch_min_ms"], row["one_launch_max_ms"], row["kernel_ms"], row["launches_per_step"],
            row["descent_ms"], row["descent_min_ms"], row["descent_max_ms"], row["descent_ms"] / row["one_launch_ms"]))
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    candidate_scoring.clear_constraint_cache()
    graph.close()
    ctx.close()


if __name__ == "__main__":
    main()
