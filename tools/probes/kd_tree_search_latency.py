"""End-to-end latency of the k-means / KD cluster-tree search: per call, host wall clock from the call to the
answer on the host, median over --reps calls after warm-up, on 10 000-sample trees of the 'walk' primitive (L = 40):

  deep   4 subdivisions, 16 levels (k-means down to a few samples per leaf, one small KD tree each)
  pure   1 subdivision: one KD tree over all samples (a deep KD descent)

  one_launch   mg_cluster_tree_search: the whole descent in one launch, one read-back of the records
  per_step     the same descent driven from the host: one mg_score_constraints call per level and per KD step
               (HipClusterTree.descend_rows with the scorer as objective)
  exhaustive   the default: every stored sample scored, first minimum (mg_best_candidate on the stored rows)

at n_candidates = 1, 2 and 5 for one search, and for 16 searches (four primitives, four constraint sets each, n = 1) in one
call against 16 calls of the other two paths.

    python tools/probes/kd_tree_search_latency.py [--reps 200] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from morphablegraphs_amd import _capi, synthetic  # noqa: E402
from morphablegraphs_amd.cluster_tree import search_on_device  # noqa: E402
from morphablegraphs_amd.kd_cluster_tree import HipClusterTree  # noqa: E402


def _median_us(fn, reps, warmup=20):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts) * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _capi.Context(0)
    searches, trees = [], {}
    for p, data in enumerate([synthetic.make_walk_primitive(seed=0)] + synthetic.make_graph_primitives(3, seed=700)):
        prim = _capi.Primitive(ctx, data)
        samples = np.random.default_rng(p).standard_normal((args.samples, prim.n_components))
        deep = HipClusterTree.from_reference(synthetic.make_kd_cluster_tree(samples, 4, 16, seed=p), prim.n_components)
        if p == 0:
            trees["deep"] = deep
            trees["pure"] = HipClusterTree.from_reference(synthetic.make_kd_cluster_tree(samples, 1, seed=p), prim.n_components)
        t_end = float(prim.n_canonical_frames - 1)
        for q in range(4):
            cons = [{"type": "position", "t": t_end, "weight": 1.0, "target": [20.0 * q - 30.0, None, 15.0 * p]},
                    {"type": "direction", "t": t_end, "weight": 0.3, "target": [0.1 * q, 1.0]}]
            searches.append((deep, prim, _capi.ConstraintSet(prim, cons)))
    print("trees:", {k: {"nodes": t.n_nodes, "kd_nodes": t.n_kd, "depth": t.depth, "kd_depth": t.kd_depth} for k, t in trees.items()})

    def per_step(s, n, steps=None):
        tree, prim, cset = s
        L = prim.n_components

        def score(rows):
            if steps is not None:
                steps.append(len(rows))
            return prim.score_constraints(cset, np.ascontiguousarray(tree.points[rows, :L]))
        return tree.descend_rows(score, n)

    def exhaustive(s):
        tree, prim, cset = s
        return prim.best_candidate(cset, np.ascontiguousarray(tree.data[:, :prim.n_components]))

    out = {"samples": args.samples, "reps": args.reps, "single": {}, "sixteen": {}}
    _, prim0, cset0 = searches[0]
    for name, tree in trees.items():
        s0 = (tree, prim0, cset0)
        for n in (1, 2, 5):
            rec = search_on_device([s0], n)[0]
            steps = []
            ref = per_step(s0, n, steps)
            assert rec["flags"] == 0 and rec["row"] == ref[1] and rec["value"] == ref[0], "paths disagree"
            ctx.profile_enable(True)
            ctx.profile_reset()
            for _ in range(50):
                search_on_device([s0], n)
            ms, launches = ctx.profile_get("cluster_tree_search")
            ctx.profile_enable(False)
            row = {"kernel_us": 1e3 * ms / launches, "one_launch_us": _median_us(lambda: search_on_device([s0], n), args.reps),
                   "per_step_us": _median_us(lambda: per_step(s0, n), args.reps),
                   "exhaustive_us": _median_us(lambda: exhaustive(s0), args.reps),
                   "scoring_calls": len(steps), "evaluations": int(rec["evaluations"])}
            out["single"]["%s_n%d" % (name, n)] = row
            print("%s n=%d  kernel %6.1f us  one launch %8.1f us   per step %8.1f us (%d calls)   exhaustive %8.1f us   (%d evaluations)" % (
                name, n, row["kernel_us"], row["one_launch_us"], row["per_step_us"], row["scoring_calls"], row["exhaustive_us"], row["evaluations"]))
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(50):
        search_on_device(searches, 1)
    ms, launches = ctx.profile_get("cluster_tree_search")
    ctx.profile_enable(False)
    row = {"kernel_us": 1e3 * ms / launches, "one_launch_us": _median_us(lambda: search_on_device(searches, 1), args.reps),
           "per_step_us": _median_us(lambda: [per_step(s, 1) for s in searches], max(args.reps // 10, 10), warmup=3),
           "exhaustive_us": _median_us(lambda: [exhaustive(s) for s in searches], max(args.reps // 10, 10), warmup=3)}
    out["sixteen"] = row
    print("16 searches (deep), n=1  kernel %6.1f us  one launch %8.1f us   per step %8.1f us   exhaustive %8.1f us" % (
        row["kernel_us"], row["one_launch_us"], row["per_step_us"], row["exhaustive_us"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for _, _, c in searches:
        c.close()
    for t in list(trees.values()) + [s[0] for s in searches]:
        t.close()
    ctx.close()


if __name__ == "__main__":
    main()
