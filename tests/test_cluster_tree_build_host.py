"""The host half of the cluster-tree builders (cluster_tree_builder.py) against the reference's own builders
(tests/golden/cluster_tree_build.npz, tools/gen_cluster_tree_build_golden.py): with the device k-means replaced by the labels
sklearn gave the reference for the same members, the k-means / KD ClusterTree and the FeatureClusterTree come out as the
reference's, table for table and mean for mean bit for bit; the writers' files load back through the project's own loaders;
the pickles name exactly the reference's classes; trees deeper than the search's limits are refused."""
import json
import os

import numpy as np
import pytest

from morphablegraphs_amd import cluster_tree_builder as ctb
from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree
from morphablegraphs_amd.cluster_tree_pickle import SafeUnpickler, load_cluster_tree_pickle
from morphablegraphs_amd.kd_cluster_tree import HipClusterTree

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_tree_build.npz"), allow_pickle=False)
NAMES = [str(n) for n in GOLDEN["names"]]
KD_TABLES = ("points", "child_begin", "children", "leaf", "kd_begin", "kd_roots", "kd_left", "kd_right", "kd_inner")
FEATURE_TABLES = ("means", "child_begin", "children", "first_index", "data")
KD_CASES = [n for i, n in enumerate(NAMES) if str(GOLDEN["c%d_kind" % i]) == "kd"]
FEATURE_CASES = [n for i, n in enumerate(NAMES) if str(GOLDEN["c%d_kind" % i]) == "feature"]


def case(name):
    p = "c%d_" % NAMES.index(name)
    return {k[len(p):]: GOLDEN[k] for k in GOLDEN.files if k.startswith(p)}


def reference_json(c):
    """The reference's save_to_json_file dict of a feature case (the golden keeps its data and features apart)."""
    d = json.loads(str(c["json"]))
    d["data"] = c["data"].tolist()
    d["features"] = (c["features"] if "features" in c else c["data"]).tolist()
    return d


class Recorded(object):
    """The device k-means replaced by the reference's recorded sklearn calls, found by the members a segment holds."""

    def __init__(self, c):
        off, mem, ks = c["call_offsets"], c["call_members"], c["call_k"]
        kofs = np.concatenate([[0], np.cumsum(ks)])
        self.calls = {}
        for i in range(len(ks)):
            key = tuple(mem[off[i]:off[i + 1]].tolist())
            self.calls[key] = {"labels": c["call_labels"][off[i]:off[i + 1]], "init": c["call_init"][kofs[i]:kofs[i + 1]],
                               "centres": c["call_centres"][kofs[i]:kofs[i + 1]], "n_iter": int(c["call_n_iter"][i]),
                               "inertia": float(c["call_inertia"][i])}
        self.used, self.batches = [], []

    def __call__(self, seg_begin, rows, node_ids):
        out = np.empty(len(rows), dtype=np.int32)
        for s in range(len(seg_begin) - 1):
            key = tuple(rows[seg_begin[s]:seg_begin[s + 1]].tolist())
            out[seg_begin[s]:seg_begin[s + 1]] = self.calls[key]["labels"]
            self.used.append(key)
        self.batches.append(len(seg_begin) - 1)
        return out

    def init(self, members):
        return self.calls[tuple(np.asarray(members).tolist())]["init"]


def build(c, kmeans, **kw):
    opts = json.loads(str(c["options"]))
    if str(c["kind"]) == "kd":
        return ctb.build_kd_cluster_tree(c["data"], opts["n_subdivisions"], opts["max_level"], opts["dim"], opts["use_kd_tree"], kmeans=kmeans, **kw)
    features = c["features"] if "features" in c else c["data"]
    return ctb.build_feature_cluster_tree(features, c["data"], opts["n_subdivisions"], opts["use_feature_mean"], kmeans=kmeans, **kw)


def tree_depth(tree):
    return int(np.max(tree.depth))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_is_golden_tree(tree, c):
    if str(c["kind"]) == "kd":
        assert isinstance(tree, HipClusterTree) and tree.n_kd == len(c["kd_point_rows"])
        for t in KD_TABLES:
            got, want = getattr(tree, t), (np.concatenate([c["data"][c["kd_point_rows"]], c["means"]]) if t == "points" else c[t])
            if t == "points":
                got, want = _bits(got), _bits(want)
            np.testing.assert_array_equal(got, want, err_msg=t)
        np.testing.assert_array_equal(_bits(tree.data), _bits(c["data"]))
    else:
        ref = HipFeatureClusterTree.from_json(reference_json(c))
        for t in FEATURE_TABLES:
            got, want = getattr(tree, t), getattr(ref, t)
            if t in ("means", "data"):
                got, want = _bits(got), _bits(want)
            np.testing.assert_array_equal(got, want, err_msg=t)
        # the whole JSON document, indices lists included
        assert json.loads(json.dumps(ctb.feature_cluster_tree_json(tree))) == reference_json(c)


@pytest.mark.parametrize("name", NAMES)
def test_tree_from_the_references_labels_is_the_references_tree(name):
    c = case(name)
    rec = Recorded(c)
    tree = build(c, rec)
    assert_is_golden_tree(tree, c)
    # exactly the reference's clustering calls, each once, one batch per level that clusters
    assert sorted(rec.used) == sorted(rec.calls) and len(rec.used) == len(set(rec.used))
    assert len(rec.batches) <= tree_depth(tree) + 1 and sum(rec.batches) == len(rec.calls)


def test_the_golden_covers_the_quirks():
    """What the cases are there for: 4x4 and 2x6 trees, no KD trees, a k-means width below the data's, features that differ
    from the data, duplicate rows under the all_equal rule, a node whose clusters were all one."""
    opts = {n: json.loads(str(case(n)["options"])) for n in NAMES}
    assert any(o.get("n_subdivisions") == 2 and o.get("max_level") == 6 for o in opts.values())
    assert any(o.get("use_kd_tree") is False for o in opts.values())
    assert any("features" in case(n) for n in FEATURE_CASES)
    dup = case("feature_duplicates")
    tree = build(dup, Recorded(dup))
    counts = np.diff(tree.child_begin)
    # a node of 2 .. 9 identical rows (more than n_subdivisions = 3) split into singletons without a k-means call
    members = [len(ix) if ix is not None else len(tree.data) for ix in tree.indices]
    rows = tree.data
    eq = [i for i, ix in enumerate(tree.indices) if ix is not None and 3 < len(ix) < 10 and np.all(rows[ix] == rows[ix[0]])]
    assert eq and all(counts[i] == members[i] for i in eq)
    kd = case("kd_4x3_dim5")
    assert kd["data"].shape[1] > json.loads(str(kd["options"]))["dim"]


@pytest.mark.parametrize("name", KD_CASES)
def test_kd_pickle_loads_back_and_names_the_references_classes(name, tmp_path):
    c = case(name)
    tree = build(c, Recorded(c))
    path = str(tmp_path / "walk_a_quaternion_cluster_tree.pck")
    ctb.write_cluster_tree(tree, path)
    loaded = load_cluster_tree_pickle(path)
    assert isinstance(loaded, HipClusterTree)
    for t in KD_TABLES + ("data",):
        np.testing.assert_array_equal(_bits(getattr(loaded, t)) if t in ("points", "data") else getattr(loaded, t),
                                      _bits(getattr(tree, t)) if t in ("points", "data") else getattr(tree, t), err_msg=t)
    assert loaded.options == tree.options
    names = _globals(open(path, "rb").read())
    sp = "morphablegraphs.space_partitioning."
    ref = {(m, n) for m, n in names if m.startswith("morphablegraphs")}
    want = {(sp + "cluster_tree", "ClusterTree"), (sp + "cluster_tree_node", "ClusterTreeNode"), (sp + "kdtree_wrapper_node", "KDTreeWrapper"),
            (sp + "kdtree", "KDTree"), (sp + "kdtree", "Node")}
    assert ref == (want if tree.n_kd else want - {(sp + "kdtree_wrapper_node", "KDTreeWrapper"), (sp + "kdtree", "KDTree"), (sp + "kdtree", "Node")})
    assert all(m.startswith("morphablegraphs") or m.startswith("numpy") or m in ("copyreg", "builtins", "_codecs") for m, _ in names)


def _globals(blob):
    import io
    seen = set()

    class Recording(SafeUnpickler):
        def find_class(self, module, name):
            seen.add((module, name))
            return SafeUnpickler.find_class(self, module, name)
    Recording(io.BytesIO(blob), encoding="latin1").load()
    return seen


@pytest.mark.parametrize("name", FEATURE_CASES)
def test_feature_json_and_pickle_load_back(name, tmp_path):
    c = case(name)
    tree = build(c, Recorded(c))
    path = str(tmp_path / "walk_a_quaternion_cluster_tree.json")
    ctb.write_cluster_tree(tree, path, "json")
    with open(path) as f:
        loaded = HipFeatureClusterTree.from_json(json.load(f))
    pck = str(tmp_path / "walk_a_quaternion_cluster_tree.pck")
    ctb.write_cluster_tree(tree, pck, "pck")
    loaded2 = load_cluster_tree_pickle(pck)
    assert isinstance(loaded2, HipFeatureClusterTree)
    assert {n for m, n in _globals(open(pck, "rb").read()) if m.startswith("morphablegraphs")} == {"FeatureClusterTree"}
    for t in FEATURE_TABLES:
        for other in (loaded, loaded2):
            got, want = getattr(other, t), getattr(tree, t)
            if t in ("means", "data"):
                got, want = _bits(got), _bits(want)
            np.testing.assert_array_equal(got, want, err_msg=t)


def _by_position(k):
    return lambda seg_begin, rows, node_ids: np.arange(len(rows)) % k


def test_trees_deeper_than_the_search_allows_are_refused(monkeypatch):
    rows = np.random.default_rng(3).standard_normal((200, 3))
    tree = ctb.build_kd_cluster_tree(rows, 2, 3, use_kd_tree=False, kmeans=_by_position(2))
    assert tree_depth(tree) > 3
    monkeypatch.setattr(ctb, "MG_TREE_MAX_DEPTH", 3)
    with pytest.raises(ValueError, match="deeper than 3 levels"):
        ctb.build_kd_cluster_tree(rows, 2, 3, use_kd_tree=False, kmeans=_by_position(2))
    with pytest.raises(ValueError, match="deeper than 3 levels"):
        ctb.build_feature_cluster_tree(rows, n_subdivisions=2, kmeans=_by_position(2))
    monkeypatch.setattr(ctb, "MG_KD_MAX_DEPTH", 4)
    with pytest.raises(ValueError, match="KD tree deeper than 4 levels"):
        ctb.build_kd_cluster_tree(rows, 1, 4)


def test_node_ids_follow_the_path():
    a = ctb.child_node_id(0, 0)
    assert a == ctb.child_node_id(0, 0) and len({ctb.child_node_id(p, j) for p in (0, a) for j in range(64)}) == 128
    assert all(0 <= ctb.child_node_id(a, j) < 2 ** 64 for j in range(4))
