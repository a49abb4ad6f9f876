"""Writes tests/golden/cluster_tree_build.npz: the trees the reference's own builders make (space_partitioning/
cluster_tree.py:96-100 ClusterTree.construct, feature_cluster_tree.py:61-98 FeatureClusterTree) on small data, and every
sklearn KMeans call they make on the way.

    python tools/gen_cluster_tree_build_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--out tests/golden/cluster_tree_build.npz]

The reference's kdtree, kdtree_wrapper_node, cluster_tree_node, cluster_tree_node_builder, cluster_tree, clustering and
feature_cluster_tree modules are imported unmodified as modules of a stub package `space_partitioning`; anim_utils' logger is a
stub, np.alltrue (removed in NumPy 2) is np.all, the modules' prints are discarded.  Each tree is built under
np.random.seed(seed) with the installed sklearn on one thread.  For every KMeans call the tool records the node's member
indices (which rows of the data the call clusters, in order), the initial centres sklearn's k-means++ chose (in the data's
coordinates: sklearn clusters X - X.mean(axis=0), so the mean is added back), and sklearn's labels, cluster_centers_, n_iter_
and inertia_.  A case in which any member's two smallest squared distances to the initial or to the final centres lie within
1e-9 relative is drawn again with the next seed: the device, which does not centre the data, could order those differently.

Per case `c<i>_` the file holds: kind ("kd" / "feature"), options (JSON), data, features (feature trees whose features are not
the data), the recorded calls (call_offsets into call_members, call_k, call_init (sum k, dim), call_labels (concatenated),
call_centres, call_n_iter, call_inertia), the tree -- kd: the kd_cluster_tree.HipClusterTree tables (child_begin, children,
leaf, kd_begin, kd_roots, kd_left, kd_right, kd_inner; the points table as the data row of every KD point, kd_point_rows, and
the node means, means); feature: the save_to_json_file dict without
its data and features (the case's arrays) as JSON text (json) -- and seed.  The archive is written with fixed timestamps, so running the tool again gives the identical file.
"""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from morphablegraphs_amd.kd_cluster_tree import HipClusterTree  # noqa: E402

MARGIN = 1e-9
KD_TABLES = ("child_begin", "children", "leaf", "kd_begin", "kd_roots", "kd_left", "kd_right", "kd_inner")
RECORD = {"members": None, "calls": []}


def load_reference(reference):
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
    np.alltrue = np.all
    mods = {}
    for name in ("kdtree", "kdtree_wrapper_node", "cluster_tree_node", "cluster_tree_node_builder", "cluster_tree", "clustering",
                 "feature_cluster_tree"):
        path = os.path.join(reference, "morphablegraphs", "space_partitioning", name + ".py")
        spec = importlib.util.spec_from_file_location(parent + "." + name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        setattr(pkg, name, mod)
        mods[name] = mod
    return mods


def instrument(mods):
    """Record the members of every clustering call and what sklearn's KMeans does with them."""
    from sklearn.cluster import KMeans, _kmeans
    builder = mods["cluster_tree_node_builder"].ClusterTreeNodeBuilder
    detect = builder._detect_clusters

    def _detect_clusters(self, data, indices, n_samples):
        RECORD["members"] = np.arange(len(data)) if indices is None else np.asarray(indices)
        return detect(self, data, indices, n_samples)
    builder._detect_clusters = _detect_clusters
    clustering = mods["clustering"]
    get_labels = clustering._get_labels_from_kmeans

    def _get_labels_from_kmeans(features, indices, n_subdivisions):
        RECORD["members"] = np.arange(len(features)) if indices is None else np.asarray(indices)
        return get_labels(features, indices, n_subdivisions)
    clustering._get_labels_from_kmeans = _get_labels_from_kmeans
    plusplus = _kmeans._kmeans_plusplus

    def _kmeans_plusplus(*args, **kwargs):
        centres, idx = plusplus(*args, **kwargs)
        RECORD["init"] = centres.copy()
        return centres, idx
    _kmeans._kmeans_plusplus = _kmeans_plusplus
    fit = KMeans.fit

    def fit_and_record(self, X, y=None, sample_weight=None):
        X = np.asarray(X, dtype=np.float64)
        out = fit(self, X, y, sample_weight)
        RECORD["calls"].append({"members": RECORD["members"], "k": self.n_clusters, "init": RECORD.pop("init") + X.mean(axis=0),
                                "labels": self.labels_.copy(), "centres": self.cluster_centers_.copy(), "n_iter": int(self.n_iter_),
                                "inertia": float(self.inertia_), "X": X})
        return out
    KMeans.fit = fit_and_record


def _two_best_close(X, centres):
    d = ((X[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2)
    d.sort(axis=1)
    return bool(np.any(d[:, 1] - d[:, 0] <= MARGIN * np.maximum(d[:, 1], 1e-300)))


def _build(mods, kind, opts, data, features, seed):
    from threadpoolctl import threadpool_limits
    RECORD["calls"] = []
    np.random.seed(seed)
    with threadpool_limits(1), contextlib.redirect_stdout(io.StringIO()):
        if kind == "kd":
            tree = mods["cluster_tree"].ClusterTree(opts["n_subdivisions"], opts["max_level"], opts["dim"], False, opts["use_kd_tree"])
            tree.construct(data)
        else:
            options = {"n_subdivisions": opts["n_subdivisions"], "clustering_method": 0, "use_feature_mean": opts["use_feature_mean"]}
            tree = mods["feature_cluster_tree"].FeatureClusterTree(features, data, None, options, [])
    return tree, list(RECORD["calls"])


def _cases():
    rng = np.random.default_rng(2024)

    def blobs(n, d, centres=6, spread=4.0):
        c = rng.standard_normal((centres, d)) * spread
        return c[rng.integers(0, centres, n)] + rng.standard_normal((n, d))
    base = blobs(900, 7)
    # 64 distinct rows in three nested scales (4 x 4 x 4), each repeated 2 .. 9 times: the nodes of a single distinct row
    # are below MAX_SIMILARITY_CHECK, so all_equal splits them without k-means
    levels = [rng.standard_normal((4, 5)) * s for s in (100.0, 10.0, 1.0)]
    distinct = (levels[0][:, None, None] + levels[1][None, :, None] + levels[2][None, None, :]).reshape(64, 5)
    dups = np.repeat(distinct, rng.integers(2, 10, 64), axis=0)
    dups = dups[rng.permutation(len(dups))]
    proj = rng.standard_normal((8, 3))
    fdata = blobs(500, 8)
    return [
        ("kd_4x4", "kd", {"n_subdivisions": 4, "max_level": 4, "dim": 6, "use_kd_tree": True}, blobs(700, 6), None),
        ("kd_2x6", "kd", {"n_subdivisions": 2, "max_level": 6, "dim": 8, "use_kd_tree": True}, blobs(800, 8), None),
        ("kd_4x3_dim5", "kd", {"n_subdivisions": 4, "max_level": 3, "dim": 5, "use_kd_tree": True}, base, None),
        ("kd_no_kd_tree", "kd", {"n_subdivisions": 4, "max_level": 3, "dim": 4, "use_kd_tree": False}, blobs(300, 4), None),
        ("kd_4x4_1200", "kd", {"n_subdivisions": 4, "max_level": 4, "dim": 10, "use_kd_tree": True}, blobs(1200, 10, 8), None),
        ("feature_same", "feature", {"n_subdivisions": 4, "use_feature_mean": False}, blobs(400, 5), None),
        ("feature_projected", "feature", {"n_subdivisions": 4, "use_feature_mean": False}, fdata, fdata @ proj),
        ("feature_duplicates", "feature", {"n_subdivisions": 4, "use_feature_mean": False}, dups, None),
        ("feature_mean_of_features", "feature", {"n_subdivisions": 4, "use_feature_mean": True}, blobs(300, 3), None),
    ]


def _write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of dfki-asr/morphablegraphs")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cluster_tree_build.npz"))
    args = ap.parse_args()
    mods = load_reference(args.reference)
    instrument(mods)
    cases = _cases()
    out = {"names": np.array([c[0] for c in cases])}
    for i, (name, kind, opts, data, features) in enumerate(cases):
        data = np.ascontiguousarray(data, dtype=np.float64)
        feats = data if features is None else np.ascontiguousarray(features, dtype=np.float64)
        for seed in range(10 * i, 10 * i + 10):
            tree, calls = _build(mods, kind, opts, data, feats, seed)
            close = [c for c in calls if _two_best_close(c["X"], c["init"]) or _two_best_close(c["X"], c["centres"])]
            if not close:
                break
            print("%s: seed %d: %d of %d calls with a member near two centres; next seed" % (name, seed, len(close), len(calls)))
        else:
            raise RuntimeError("%s: no seed without near ties" % name)
        p = "c%d_" % i
        sizes = [len(c["members"]) for c in calls]
        out.update({p + "kind": np.array(kind), p + "options": np.array(json.dumps(opts, sort_keys=True)), p + "data": data,
                    p + "seed": np.int64(seed), p + "call_offsets": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                    p + "call_members": np.concatenate([c["members"] for c in calls]).astype(np.int32),
                    p + "call_k": np.array([c["k"] for c in calls], dtype=np.int32),
                    p + "call_init": np.concatenate([c["init"] for c in calls]), p + "call_centres": np.concatenate([c["centres"] for c in calls]),
                    p + "call_labels": np.concatenate([c["labels"] for c in calls]).astype(np.int32),
                    p + "call_n_iter": np.array([c["n_iter"] for c in calls], dtype=np.int32),
                    p + "call_inertia": np.array([c["inertia"] for c in calls], dtype=np.float64)})
        if kind == "kd":
            flat = HipClusterTree.from_reference(tree)
            out.update({p + t: getattr(flat, t) for t in KD_TABLES})
            row_of = {data[r].tobytes(): r for r in range(len(data))}
            out[p + "kd_point_rows"] = np.array([row_of[flat.points[i].tobytes()] for i in range(flat.n_kd)], dtype=np.int32)
            out[p + "means"] = flat.means
            desc = "%d nodes, %d KD nodes, depth %d" % (flat.n_nodes, flat.n_kd, flat.depth)
        else:
            with contextlib.redirect_stdout(io.StringIO()):
                tree_data = {"options": tree._options, "root": tree.node_to_json()}
                desc = "%d leaves" % tree.get_number_of_leafs()
            out[p + "json"] = np.array(json.dumps(tree_data))
            if features is not None:
                out[p + "features"] = feats
        print("%-26s seed %3d  %4d rows  %4d KMeans calls  %s" % (name, seed, len(data), len(calls), desc))
    _write_npz(args.out, out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
