"""Writes tests/golden/cluster_tree_search.npz: what the reference's own cluster-tree search
(space_partitioning/feature_cluster_tree.py:129-187, FeatureClusterTree.load_from_json(...)
.find_best_example_excluding_search_candidates(obj, args, n)) returns on small synthetic trees, and the objective calls it
makes on the way.

    python tools/gen_cluster_tree_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--out tests/golden/cluster_tree_search.npz]

The reference's feature_cluster_tree.py is imported unmodified through a stub parent package: its sibling `clustering` (tree
construction, unused by load_from_json) and anim_utils' logger are stubs.  The objective is the oracle's keyframe objective
(oracle.mg_oracle.OraclePrimitive.keyframe_errors; the summed aligned_residuals for the case aligned to a previous frame),
wrapped to record every call in order.

Every value the search's heaps compare is checked against the one it is compared with: two values within 1e-7 relative of
each other could be ordered differently by the device's rounding, so such a case is drawn again with the next seed.

Per case `k` the file holds (keys prefixed "c<k>_"): tree_json (the reference's JSON text), means / child_begin / children /
first_index (the flattening of cluster_tree.HipFeatureClusterTree), primitive (JSON: synthetic factory and keyword
arguments), constraints (JSON), prev_frame (empty: local), n_candidates, call_means / call_values (the objective calls in
order), value and row (the reference's answer; row = the index of the returned data row).
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from morphablegraphs_amd import synthetic  # noqa: E402
from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree  # noqa: E402
from oracle import mg_oracle  # noqa: E402

MARGIN = 1e-7


def load_reference_module(reference):
    """feature_cluster_tree.py of the reference, unmodified, as a module of a stub parent package."""
    parent = "_reference_space_partitioning"
    pkg = types.ModuleType(parent)
    pkg.__path__ = []
    sys.modules[parent] = pkg
    clustering = types.ModuleType(parent + ".clustering")

    def _unused(*args, **kwargs):
        raise NotImplementedError("tree construction is not part of the search")
    clustering.find_clusters = clustering.all_equal = _unused
    sys.modules[clustering.__name__] = clustering
    for name in ("anim_utils", "anim_utils.utilities", "anim_utils.utilities.log"):
        sys.modules.setdefault(name, types.ModuleType(name))
    log = sys.modules["anim_utils.utilities.log"]
    log.write_message_to_log = lambda *args, **kwargs: None
    log.LOG_MODE_DEBUG = 0
    path = os.path.join(reference, "morphablegraphs", "space_partitioning", "feature_cluster_tree.py")
    spec = importlib.util.spec_from_file_location(parent + ".feature_cluster_tree", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


class _Tracked(float):
    """A float that notes the values it is compared with (the heaps' tuple comparisons reach the values first)."""
    pairs = []

    def __eq__(self, other):
        _Tracked.pairs.append((float(self), float(other)))
        return float(self) == float(other)

    def __lt__(self, other):
        _Tracked.pairs.append((float(self), float(other)))
        return float(self) < float(other)

    __hash__ = float.__hash__


def _objective(prim_spec, constraints, prev_frame):
    data = getattr(synthetic, prim_spec["factory"])(**prim_spec["kwargs"])
    op = mg_oracle.OraclePrimitive(data)
    if prev_frame is None:
        return lambda S: float(op.keyframe_errors(S, constraints)[0])
    joints, animated = synthetic.make_skeleton(n_animated=(op.n_dim - 3) // 4)
    return lambda S: float(op.aligned_residuals(S, constraints, prev_frame, joints, animated, animated[0]).sum())


def _run_case(ref, tree_json, prim_spec, constraints, prev_frame, n_candidates):
    f = _objective(prim_spec, constraints, prev_frame)
    calls, values = [], []

    def obj(mean, args):
        v = f(np.asarray(mean, dtype=np.float64)[None, :])
        calls.append(np.array(mean, dtype=np.float64))
        values.append(v)
        return _Tracked(v)
    _Tracked.pairs = []
    tree = ref.FeatureClusterTree.load_from_json(json.loads(tree_json))
    value, row = tree.find_best_example_excluding_search_candidates(obj, [], n_candidates)
    data = np.asarray(json.loads(tree_json)["data"], dtype=np.float64)
    hits = np.nonzero(np.all(data == np.asarray(row), axis=1))[0]
    close = [(a, b) for a, b in _Tracked.pairs if np.isfinite(a) and np.isfinite(b) and abs(a - b) <= MARGIN * max(abs(a), abs(b))]
    return float(value), int(hits[0]), np.asarray(calls).reshape(len(calls), data.shape[1]), np.asarray(values), close


def _samples(prim_spec, n, seed):
    data = getattr(synthetic, prim_spec["factory"])(**prim_spec["kwargs"])
    op = mg_oracle.OraclePrimitive(data)
    width = op.n_components + op.n_time_components
    return np.random.default_rng(seed).standard_normal((n, width))


def _nine_singletons_tree(samples, seed):
    """A root whose first child holds rows 0..8 as nine singleton children (the reference's all_equal branch), the rest of
    the rows clustered under the root's other children."""
    rest = synthetic.make_feature_cluster_tree(samples[9:], 4, seed)

    def shift(node):
        node["indices"] = None if node["indices"] is None else [i + 9 for i in node["indices"]]
        for c in node["children"]:
            shift(c)
    shift(rest["root"])
    nine = {"mean": samples[:9].mean(axis=0).tolist(), "indices": list(range(9)),
            "children": [{"mean": samples[i].tolist(), "indices": [i], "children": []} for i in range(9)]}
    return {"data": samples.tolist(), "features": samples.tolist(), "options": rest["options"],
            "root": {"mean": samples.mean(axis=0).tolist(), "indices": None, "children": [nine] + rest["root"]["children"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of dfki-asr/morphablegraphs")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cluster_tree_search.npz"))
    args = ap.parse_args()
    ref = load_reference_module(args.reference)
    tiny = {"factory": "make_tiny_primitive", "kwargs": {"seed": 1}}
    tiny_t = {"factory": "make_tiny_primitive", "kwargs": {"seed": 2, "n_time_components": 2}}
    pos = [{"type": "position", "t": 11.0, "weight": 1.0, "target": [40.0, None, -25.0]},
           {"type": "position", "t": 5.5, "weight": 0.5, "target": [10.0, 3.0, 20.0]}]
    mixed = [{"type": "position", "t": 11.0, "weight": 1.0, "target": [-30.0, None, 60.0]},
             {"type": "direction", "t": 11.0, "weight": 0.4, "target": [0.3, 1.0]}]
    # (name, primitive, tree kind, samples, constraints, previous frame or None, n_candidates)
    specs = [("tiny_n1", tiny, "kmeans", 300, pos, None, 1),
             ("tiny_n2", tiny, "kmeans", 300, pos, None, 2),
             ("tiny_n5", tiny, "kmeans", 300, pos, None, 5),
             ("time_latents", tiny_t, "kmeans", 200, pos, None, 2),
             ("nine_singletons", tiny, "nine", 60, pos, None, 5),
             ("root_only", tiny, "root", 5, pos, None, 1),
             ("aligned", tiny, "kmeans", 200, pos, [12.0, 80.0, -5.0, 0.9, 0.1, 0.3, 0.2], 2),
             ("direction", tiny, "kmeans", 200, mixed, None, 2)]
    out = {"names": np.array([s[0] for s in specs])}
    for k, (name, prim_spec, kind, n, cons, prev, nc) in enumerate(specs):
        for seed in range(100 + 10 * k, 110 + 10 * k):
            samples = _samples(prim_spec, n, seed)
            if kind == "kmeans":
                tree_data = synthetic.make_feature_cluster_tree(samples, 4, seed)
            elif kind == "nine":
                tree_data = _nine_singletons_tree(samples, seed)
            else:
                tree_data = {"data": samples.tolist(), "features": samples.tolist(), "options": {"n_subdivisions": 4, "use_feature_mean": False},
                             "root": {"mean": samples.mean(axis=0).tolist(), "indices": [3, 1], "children": []}}
            tree_json = json.dumps(tree_data)
            prev_frame = None if prev is None else np.asarray(prev, dtype=np.float64)
            value, row, calls, values, close = _run_case(ref, tree_json, prim_spec, cons, prev_frame, nc)
            if not close:
                break
            print("%s: seed %d has %d compared pairs within the margin, next seed" % (name, seed, len(close)))
        else:
            raise RuntimeError("%s: no seed meets the margin" % name)
        flat = HipFeatureClusterTree.from_json(tree_data)
        p = "c%d_" % k
        out.update({p + "tree_json": np.array(tree_json), p + "means": flat.means, p + "child_begin": flat.child_begin,
                    p + "children": flat.children, p + "first_index": flat.first_index, p + "primitive": np.array(json.dumps(prim_spec)),
                    p + "constraints": np.array(json.dumps(cons)), p + "prev_frame": np.zeros(0) if prev is None else prev_frame,
                    p + "n_candidates": np.int64(nc), p + "call_means": calls, p + "call_values": values,
                    p + "value": np.float64(value), p + "row": np.int64(row), p + "seed": np.int64(seed)})
        print("%-16s n=%d  %4d nodes  %3d calls  value %.6g  row %d" % (name, nc, flat.n_nodes, len(values), value, row))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
