"""Writes tests/golden/kd_cluster_tree_search.npz: what the reference's own k-means / KD cluster-tree search
(space_partitioning/cluster_tree.py:117-149, ClusterTree.find_best_example_excluding_search_candidates(obj, data, n)) returns
on small trees its own builder made, and the objective calls it makes on the way.

    python tools/gen_kd_cluster_tree_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--out tests/golden/kd_cluster_tree_search.npz]

The reference's kdtree.py, kdtree_wrapper_node.py, cluster_tree_node.py, cluster_tree_node_builder.py and cluster_tree.py are
imported unmodified as modules of a stub parent package `space_partitioning` (its constants from the reference's
__init__.py); anim_utils' logger is a stub.  Trees are built with sklearn's KMeans under a fixed np.random.seed.  A tree with
one subdivision gets its root from construct_from_data(data, all indices): ClusterTree.construct passes indices=None, and a
root that is a leaf then wraps data[None] -- every row -- into a single KD point.

The objective is the oracle's keyframe objective (the summed aligned_residuals for the case aligned to a previous frame),
wrapped to record every call.  Every value the heaps compare is checked against the one it is compared with: values within
1e-7 relative could be ordered differently by the device's rounding, so such a case is drawn again with the next seed.

The tool also pickles each tree as the reference does (pickle.HIGHEST_PROTOCOL) and checks that cluster_tree_pickle reads the
bytes into the same tables as the flattening of the live objects; no pickle is written.

Per case `k` the file holds (keys prefixed "c<k>_"): the tables of kd_cluster_tree.HipClusterTree (data, points, n_kd,
child_begin, children, leaf, kd_begin, kd_roots, kd_left, kd_right, kd_inner), primitive (JSON: synthetic factory and keyword
arguments), constraints (JSON), prev_frame (empty: local), n_candidates, call_points / call_values (the objective calls in
order), value and sample (the reference's answer), raised (the exception's class name, empty if none).
"""
import argparse
import importlib.util
import json
import os
import pickle
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from morphablegraphs_amd import synthetic  # noqa: E402
from morphablegraphs_amd.cluster_tree_pickle import load_cluster_tree_pickle  # noqa: E402
from morphablegraphs_amd.kd_cluster_tree import HipClusterTree  # noqa: E402
from oracle import mg_oracle  # noqa: E402

MARGIN = 1e-7
TABLES = ("data", "points", "child_begin", "children", "leaf", "kd_begin", "kd_roots", "kd_left", "kd_right", "kd_inner")


def load_reference(reference):
    """The five modules of the reference, unmodified, as modules of a stub package `space_partitioning`."""
    parent = "space_partitioning"
    pkg = types.ModuleType(parent)
    pkg.__path__ = []
    pkg.KDTREE_WRAPPER_NODE, pkg.LEAF_NODE, pkg.INNER_NODE, pkg.ROOT_NODE = "kdtree", "leaf", "inner", "root"
    sys.modules[parent] = pkg
    for name in ("anim_utils", "anim_utils.utilities", "anim_utils.utilities.log"):
        sys.modules.setdefault(name, types.ModuleType(name))
    log = sys.modules["anim_utils.utilities.log"]
    log.write_log = log.write_message_to_log = lambda *args, **kwargs: None
    log.LOG_MODE_DEBUG, log.LOG_MODE_INFO, log.LOG_MODE_ERROR = 0, 1, 2
    mods = {}
    for name in ("kdtree", "kdtree_wrapper_node", "cluster_tree_node", "cluster_tree_node_builder", "cluster_tree"):
        path = os.path.join(reference, "morphablegraphs", "space_partitioning", name + ".py")
        spec = importlib.util.spec_from_file_location(parent + "." + name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        setattr(pkg, name, mod)
        mods[name] = mod
    return mods


class _Tracked(float):
    """A float that notes the values it is compared with."""
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


def _build(mods, samples, kw, seed):
    np.random.seed(seed)
    tree = mods["cluster_tree"].ClusterTree(kw.get("n_subdivisions", 4), kw.get("max_level", 4), samples.shape[1], False, kw.get("use_kd_tree", True))
    if tree.n_subdivisions == 1:
        tree.data, tree.dim = samples, samples.shape[1]
        builder = mods["cluster_tree_node_builder"].ClusterTreeNodeBuilder(1, tree.max_level, tree.dim, False, tree.use_kd_tree)
        tree.root = builder.construct_from_data(samples, list(range(len(samples))))
    else:
        tree.construct(samples)
    return tree


def _run_case(tree, prim_spec, constraints, prev_frame, n_candidates):
    f = _objective(prim_spec, constraints, prev_frame)
    calls, values = [], []

    def obj(x, args):
        v = f(np.asarray(x, dtype=np.float64)[None, :])
        calls.append(np.array(x, dtype=np.float64))
        values.append(v)
        return _Tracked(v)
    _Tracked.pairs = []
    raised, value, sample = "", np.nan, None
    try:
        value, sample = tree.find_best_example_excluding_search_candidates(obj, [], n_candidates)
    except (AttributeError, TypeError) as e:
        raised = type(e).__name__
    close = [(a, b) for a, b in _Tracked.pairs if np.isfinite(a) and np.isfinite(b) and abs(a - b) <= MARGIN * max(abs(a), abs(b))]
    width = tree.data.shape[1]
    return (float(value), np.zeros(0) if sample is None else np.asarray(sample, dtype=np.float64), np.asarray(calls).reshape(len(calls), width),
            np.asarray(values), raised, close)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of dfki-asr/morphablegraphs")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kd_cluster_tree_search.npz"))
    args = ap.parse_args()
    mods = load_reference(args.reference)
    tiny = {"factory": "make_tiny_primitive", "kwargs": {"seed": 1}}
    pos = [{"type": "position", "t": 11.0, "weight": 1.0, "target": [40.0, None, -25.0]},
           {"type": "position", "t": 5.5, "weight": 0.5, "target": [10.0, 3.0, 20.0]}]
    prev = [12.0, 80.0, -5.0, 0.9, 0.1, 0.3, 0.2]
    # (name, tree options, samples, previous frame or None, n_candidates, the exception expected or "")
    specs = [("small_n1", {}, 300, None, 1, ""), ("small_n2", {}, 300, None, 2, ""), ("small_n5", {"max_level": 6}, 300, None, 5, ""),
             ("pure_kd_n1", {"n_subdivisions": 1}, 2000, None, 1, ""), ("pure_kd_n5", {"n_subdivisions": 1}, 2000, None, 5, ""),
             ("kmeans_only_n2", {"use_kd_tree": False}, 200, None, 2, ""), ("kmeans_only_n5", {"use_kd_tree": False}, 200, None, 5, ""),
             ("aligned_n2", {}, 300, prev, 2, ""), ("no_mean_n1", {}, 2000, None, 1, "AttributeError")]
    op = mg_oracle.OraclePrimitive(synthetic.make_tiny_primitive(seed=1))
    width = op.n_components + op.n_time_components
    out = {"names": np.array([s[0] for s in specs])}
    for k, (name, kw, n, prev_frame, nc, expect) in enumerate(specs):
        for seed in range(100 + 10 * k, 110 + 10 * k):
            samples = np.random.default_rng(seed).standard_normal((n, width))
            tree = _build(mods, samples, kw, seed)
            pf = None if prev_frame is None else np.asarray(prev_frame, dtype=np.float64)
            value, sample, calls, values, raised, close = _run_case(tree, tiny, pos, pf, nc)
            if not close and raised == expect:
                break
            print("%s: seed %d: %d compared pairs within the margin, raised %r; next seed" % (name, seed, len(close), raised))
        else:
            raise RuntimeError("%s: no seed gives the case" % name)
        flat = HipClusterTree.from_reference(tree)
        loaded = load_cluster_tree_pickle(pickle.dumps(tree, pickle.HIGHEST_PROTOCOL))
        for t in TABLES:
            assert np.array_equal(getattr(flat, t), getattr(loaded, t)), (name, t)
        p = "c%d_" % k
        out.update({p + t: getattr(flat, t) for t in TABLES})
        out.update({p + "n_kd": np.int64(flat.n_kd), p + "primitive": np.array(json.dumps(tiny)), p + "constraints": np.array(json.dumps(pos)),
                    p + "prev_frame": np.zeros(0) if pf is None else pf, p + "n_candidates": np.int64(nc), p + "call_points": calls,
                    p + "call_values": values, p + "value": np.float64(value), p + "sample": sample, p + "raised": np.array(raised),
                    p + "seed": np.int64(seed)})
        print("%-16s n=%d  %4d nodes %5d KD nodes  %4d calls  value %.6g  %s" % (name, nc, flat.n_nodes, flat.n_kd, len(values), value, raised))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
