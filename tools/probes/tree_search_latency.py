"""End-to-end latency of the cluster-tree search on a 10 000-sample tree: per call, host wall clock
from the call to the answer on the host, median over --reps calls after warm-up.

  one_launch   mg_cluster_tree_search: the whole descent in one launch, one read-back of the records
  per_level    the same descent driven from the host: per level one upload of the children's means, one mg_score_constraints
               launch, one read-back (a synchronisation) -- HipFeatureClusterTree.descend with the scorer as objective
  exhaustive   today's default: every stored sample scored, first minimum (mg_best_candidate on the stored rows)

at n_candidates = 1, 2 and 5 for one search, and for 16 searches (four primitives, four constraint sets each, n = 1) in one
call against 16 calls of the other two paths.

    python tools/probes/tree_search_latency.py [--reps 200] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from morphablegraphs_amd import _capi, synthetic  # noqa: E402
from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree, search_on_device  # noqa: E402


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
    searches, info = [], []
    for p, data in enumerate([synthetic.make_walk_primitive(seed=0)] + synthetic.make_graph_primitives(3, seed=700)):
        prim = _capi.Primitive(ctx, data)
        samples = np.random.default_rng(p).standard_normal((args.samples, prim.n_components))
        t0 = time.perf_counter()
        tree = HipFeatureClusterTree.from_json(synthetic.make_feature_cluster_tree(samples, 4, seed=p), prim.n_components)
        info.append({"L": prim.n_components, "nodes": tree.n_nodes, "depth": int(tree.depth.max()), "build_s": round(time.perf_counter() - t0, 2)})
        t_end = float(prim.n_canonical_frames - 1)
        for q in range(4):
            cons = [{"type": "position", "t": t_end, "weight": 1.0, "target": [20.0 * q - 30.0, None, 15.0 * p]},
                    {"type": "direction", "t": t_end, "weight": 0.3, "target": [0.1 * q, 1.0]}]
            searches.append((tree, prim, _capi.ConstraintSet(prim, cons)))
    print("trees:", info)

    def per_level(s, n):
        tree, prim, cset = s
        return tree.descend(lambda ids: prim.score_constraints(cset, tree.means[ids]), n)

    def exhaustive(s):
        tree, prim, cset = s
        return prim.best_candidate(cset, tree.data[:, :prim.n_components])

    out = {"samples": args.samples, "reps": args.reps, "trees": info, "single": {}, "sixteen": {}}
    s0 = searches[0]
    for n in (1, 2, 5):
        rec = search_on_device([s0], n)[0]
        ref = per_level(s0, n)
        assert rec["leaf"] == ref[2] and rec["value"] == ref[0], "paths disagree"
        levels = []
        s0[0].descend(lambda ids: (levels.append(len(ids)), s0[1].score_constraints(s0[2], s0[0].means[ids]))[1], n)
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(50):
            search_on_device([s0], n)
        ms, launches = ctx.profile_get("cluster_tree_search")
        ctx.profile_enable(False)
        row = {"kernel_us": 1e3 * ms / launches, "one_launch_us": _median_us(lambda: search_on_device([s0], n), args.reps),
               "per_level_us": _median_us(lambda: per_level(s0, n), args.reps),
               "exhaustive_us": _median_us(lambda: exhaustive(s0), args.reps),
               "levels": len(levels), "evaluations": int(rec["evaluations"])}
        out["single"][str(n)] = row
        print("n=%d  kernel %6.1f us  one launch %8.1f us   per level %8.1f us (%d levels)   exhaustive %8.1f us   (%d evaluations)" % (
            n, row["kernel_us"], row["one_launch_us"], row["per_level_us"], row["levels"], row["exhaustive_us"], row["evaluations"]))
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(50):
        search_on_device(searches, 1)
    ms, launches = ctx.profile_get("cluster_tree_search")
    ctx.profile_enable(False)
    row = {"kernel_us": 1e3 * ms / launches, "one_launch_us": _median_us(lambda: search_on_device(searches, 1), args.reps),
           "per_level_us": _median_us(lambda: [per_level(s, 1) for s in searches], max(args.reps // 10, 10), warmup=3),
           "exhaustive_us": _median_us(lambda: [exhaustive(s) for s in searches], max(args.reps // 10, 10), warmup=3)}
    out["sixteen"] = row
    print("16 searches, n=1  kernel %6.1f us  one launch %8.1f us   per level %8.1f us   exhaustive %8.1f us" % (
        row["kernel_us"], row["one_launch_us"], row["per_level_us"], row["exhaustive_us"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for _, _, c in searches:
        c.close()
    for t in {id(s[0]): s[0] for s in searches}.values():
        t.close()
    ctx.close()


if __name__ == "__main__":
    main()
