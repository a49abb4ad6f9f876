"""Latency of a cluster-tree search whose constraint list holds per-frame constraints: a
collision-avoidance position on a hand and a local trajectory on the hips behind a keyframe constraint, at the walk primitive's
shape (L = 40, F = 156, 19 animated joints), two ways:

  one_launch   search_best_sample_on_device(per_frame=True): the whole descent in ONE mg_cluster_tree_search_frames launch -- the
               children's joint tracks and the chain scorers inside it -- and one read-back
  descent      search_best_sample_batched, what such a search takes without the flag: per tree level one round of uploads,
               mg_score_constraints, mg_joint_tracks, mg_score_frame_constraints and a read-back

A search's time is the host clock from the call to the result on the host (both ways end in a read-back, a synchronisation), median
over --reps searches after warm-up, the two ways alternating; kernel_ms is the one launch's own time from the device events of
profile slot 11.  The two ways must return the same sample and errors within the per-frame scorers' tolerance, which is checked first.

    python tools/probes/tree_search_frames_latency.py [--reps 20] [--fan 8] [--candidates 2] [--out FILE.json]
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
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraphNode  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fan", type=int, default=8)
    ap.add_argument("--candidates", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _capi.Context(0)
    node = HipMotionStateGraphNode(context=ctx)
    node.init_from_dict("walk", {"name": "walk", "mm": synthetic.make_walk_primitive(seed=0)})
    L = node.get_n_spatial_components()
    # a full tree of depth 3: --fan children per node, the leaves on the third level (node 0 the root, breadth first)
    counts = np.array([args.fan] + [args.fan] * args.fan + [args.fan] * args.fan ** 2 + [0] * args.fan ** 3)
    means = np.random.default_rng(0).standard_normal((len(counts), L))
    node.cluster_tree = HipFeatureClusterTree(means, means, np.concatenate([[0], np.cumsum(counts)]), np.arange(1, len(counts)),
                                              np.where(counts == 0, np.arange(len(counts)), -1), n_spatial=L)
    depth = int(node.cluster_tree.depth.max())
    sk = _capi.Skeleton(*synthetic.make_skeleton())
    prim = node.motion_primitive._prim
    F = node.get_n_canonical_frames()
    path = np.asarray(prim.back_project_frames(np.zeros((1, L), dtype=np.float32)), dtype=np.float64)[0, :, :3]
    cons = [{"type": "position", "t": float(F - 1), "weight": 1.0, "target": [float(path[-1][0]) + 2.0, None, float(path[-1][2]) - 1.0]},
            {"type": "frame_ca_position", "joint": "LeftHand", "target": [float(path[60][0]) + 3.0, None, float(path[60][2]) - 2.0], "n_frames": F, "weight": 2.0},
            {"type": "frame_local_trajectory", "joint": "Hips", "control_points": (path[::20] + np.array([0.5, 0.0, -0.5])).tolist(), "granularity": 1000,
             "start_t": 3.0, "n_frames": F, "weight": 0.01}]
    print("tree depth %d, %d nodes, %d candidates kept per level" % (depth, node.cluster_tree.n_nodes, args.candidates))

    def one_launch():
        return node.search_best_sample_on_device(cons, args.candidates, skeleton=sk, per_frame=True)

    def descent():
        return node.search_best_sample_batched(cons, args.candidates, skeleton=sk)

    a, b = one_launch(), descent()
    assert np.array_equal(a[1], b[1]) and abs(a[0] - b[0]) <= 1e-8 + 1e-8 * abs(b[0]), "the two ways disagree: %r, %r" % (a[0], b[0])
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
    out = {"depth": depth, "nodes": int(node.cluster_tree.n_nodes), "candidates": args.candidates, "reps": args.reps, "error": float(a[0]),
           "one_launch_ms": 1e3 * float(np.median(t_one)), "one_launch_min_ms": 1e3 * float(np.min(t_one)), "one_launch_max_ms": 1e3 * float(np.max(t_one)),
           "descent_ms": 1e3 * float(np.median(t_desc)), "descent_min_ms": 1e3 * float(np.min(t_desc)), "descent_max_ms": 1e3 * float(np.max(t_desc)),
           "kernel_ms": ms / max(launches, 1), "launches_per_search": launches / max(args.reps // 2, 1)}
    print("one launch %9.3f ms [%.3f .. %.3f] (kernel %.3f ms, %.0f launch per search)   descent %9.3f ms [%.3f .. %.3f]   ratio %.1f" % (
        out["one_launch_ms"], out["one_launch_min_ms"], out["one_launch_max_ms"], out["kernel_ms"], out["launches_per_search"],
        out["descent_ms"], out["descent_min_ms"], out["descent_max_ms"], out["descent_ms"] / out["one_launch_ms"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    candidate_scoring.clear_constraint_cache()
    node.cluster_tree.close()
    prim.close()
    ctx.close()


if __name__ == "__main__":
    main()
