"""The host side of the cluster-tree search (morphablegraphs_amd/cluster_tree.py): the reference's JSON tree flattened and
validated, and its descent (space_partitioning/feature_cluster_tree.py:129-187) restated for any Python objective, checked
against tests/golden/cluster_tree_search.npz -- the calls, value and row the reference's own method produced
(tools/gen_cluster_tree_golden.py)."""
import copy
import json
import os

import numpy as np
import pytest

from morphablegraphs_amd import model_io, synthetic
from morphablegraphs_amd.cluster_tree import MG_TREE_MAX_CHILDREN, MG_TREE_MAX_DEPTH, HipFeatureClusterTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cluster_tree_search.npz")


def _golden():
    return np.load(GOLDEN, allow_pickle=False)


def _cases():
    g = _golden()
    return list(enumerate(str(n) for n in g["names"]))


def _unflatten(tree):
    """The nested JSON root back from the flattened arrays (means, children, indices[0])."""
    def node(i):
        fi = int(tree.first_index[i])
        return {"mean": tree.means[i].tolist(), "first": None if fi < 0 else fi,
                "children": [node(int(c)) for c in tree.children[tree.child_begin[i]:tree.child_begin[i + 1]]]}
    return node(0)


def _strip(node):
    return {"mean": node["mean"], "first": node["indices"][0] if node["indices"] else None,
            "children": [_strip(c) for c in node["children"]]}


def test_json_round_trip_through_flattening():
    samples = np.random.default_rng(3).standard_normal((500, 6))
    tree_data = json.loads(json.dumps(synthetic.make_feature_cluster_tree(samples, 4, seed=1)))
    tree = HipFeatureClusterTree.from_json(tree_data, n_spatial=4)
    np.testing.assert_array_equal(tree.data, samples)
    assert tree.data.dtype == np.float64 and tree.means.shape == (tree.n_nodes, 6)
    assert _unflatten(tree) == _strip(tree_data["root"])
    assert tree_data["root"]["indices"] is None and tree.first_index[0] == -1   # the reference's root has no indices
    assert tree_data["options"]["use_feature_mean"] is False
    assert tree.depth[0] == 0 and tree.depth.max() >= 3
    # breadth first: node 0 is the root, a node's children are consecutive and every child comes after its parent
    for i in range(tree.n_nodes):
        kids = tree.children[tree.child_begin[i]:tree.child_begin[i + 1]]
        assert np.all(kids > i) and np.all(np.diff(kids) == 1)
        assert np.all(tree.depth[kids] == tree.depth[i] + 1)
    # the fixture's flattened arrays are this flattening of its JSON
    g = _golden()
    for k, _ in _cases():
        t = HipFeatureClusterTree.from_json(json.loads(str(g["c%d_tree_json" % k])))
        for name in ("means", "child_begin", "children", "first_index"):
            np.testing.assert_array_equal(getattr(t, name), g["c%d_%s" % (k, name)], err_msg=name)


def _small_tree():
    data = np.arange(12, dtype=np.float64).reshape(4, 3)
    leaf = lambda i: {"mean": data[i].tolist(), "indices": [i], "children": []}
    return {"data": data.tolist(), "features": [], "options": {}, "root": {"mean": data.mean(0).tolist(), "indices": None, "children": [
        {"mean": data[:2].mean(0).tolist(), "indices": [0, 1], "children": [leaf(0), leaf(1)]}, leaf(2), leaf(3)]}}


def test_malformed_trees_are_rejected():
    HipFeatureClusterTree.from_json(_small_tree(), n_spatial=3)

    def broken(edit):
        t = copy.deepcopy(_small_tree())
        edit(t)
        return t
    cases = {
        "leaf without indices": broken(lambda t: t["root"]["children"][1].update(indices=[])),
        "leaf with null indices": broken(lambda t: t["root"]["children"][1].update(indices=None)),
        "index out of range": broken(lambda t: t["root"]["children"][2].update(indices=[4])),
        "negative index": broken(lambda t: t["root"]["children"][0].update(indices=[-1, 0])),
        "mean narrower than data": broken(lambda t: t["root"]["children"][2].update(mean=[1.0, 2.0])),
        "all means narrower than data": broken(lambda t: t.update(data=[r + [0.0] for r in t["data"]])),
    }
    for what, t in cases.items():
        with pytest.raises(ValueError):
            HipFeatureClusterTree.from_json(t)
            pytest.fail(what)
    with pytest.raises(ValueError):     # means must cover the primitive's spatial latents
        HipFeatureClusterTree.from_json(_small_tree(), n_spatial=4)
    deep = {"mean": [0.0], "indices": [0], "children": []}
    for _ in range(MG_TREE_MAX_DEPTH + 1):
        deep = {"mean": [0.0], "indices": [0], "children": [deep]}
    with pytest.raises(ValueError):
        HipFeatureClusterTree.from_json({"data": [[0.0]], "features": [], "options": {}, "root": deep})
    wide = {"mean": [0.0], "indices": None, "children": [{"mean": [0.0], "indices": [0], "children": []}] * (MG_TREE_MAX_CHILDREN + 1)}
    with pytest.raises(ValueError):
        HipFeatureClusterTree.from_json({"data": [[0.0]], "features": [], "options": {}, "root": wide})
    # flattened arrays: a cycle unreachable from the root, a node with two parents, the root as somebody's child
    data, means = np.zeros((3, 1)), np.zeros((3, 1))
    for cb, ch in (([0, 0, 1, 2], [2, 1]), ([0, 2, 2, 2], [1, 1]), ([0, 1, 2, 2], [1, 0])):
        with pytest.raises(ValueError):
            HipFeatureClusterTree(data, means, cb, ch, [-1, 0, 1])
    HipFeatureClusterTree(data, means, [0, 2, 2, 2], [1, 2], [-1, 0, 1])


@pytest.mark.parametrize("k,name", _cases())
def test_host_descent_reproduces_the_reference(k, name):
    g = _golden()
    tree = HipFeatureClusterTree.from_json(json.loads(str(g["c%d_tree_json" % k])))
    call_means, call_values = g["c%d_call_means" % k], g["c%d_call_values" % k]
    calls = []

    def obj(mean, args):   # the reference's objective, looked up in the order it was called
        j = len(calls)
        assert args == "args"
        np.testing.assert_array_equal(mean, call_means[j], err_msg="call %d" % j)
        calls.append(j)
        return call_values[j]
    value, row = tree.find_best_example_excluding_search_candidates(obj, "args", int(g["c%d_n_candidates" % k]))
    assert len(calls) == len(call_values)
    assert value == g["c%d_value" % k] or (np.isinf(value) and np.isinf(g["c%d_value" % k]))
    np.testing.assert_array_equal(row, tree.data[int(g["c%d_row" % k])])
    # the batched form: one scoring call per level, the same answer and the same number of objectives
    levels = []
    v2, row2, leaf, n_eval = tree.descend(lambda ids: (levels.append(len(ids)), [call_values[sum(levels[:-1]) + i] for i in range(len(ids))])[1],
                                          int(g["c%d_n_candidates" % k]))
    assert v2 == value or np.isinf(value)
    np.testing.assert_array_equal(row2, row)
    assert n_eval == len(call_values) and sum(levels) == n_eval
    assert tree.first_index[leaf] == g["c%d_row" % k]


def test_quirks_of_the_reference():
    tree = HipFeatureClusterTree.from_json(_small_tree())
    # candidates are the heap LIST's prefix: values 3, 1, 2 pushed -> list [1, 3, 2]; n = 2 keeps (1, 3), not (1, 2)
    order = []
    vals = {1: 3.0, 2: 1.0, 3: 2.0, 4: 7.0, 5: 5.0}   # node ids: 1 = inner, 2, 3 = leaves 2, 3; 4, 5 = leaves 0, 1

    def score(ids):
        order.append(list(ids))
        return [vals[i] for i in ids]
    value, row, leaf, n_eval = tree.descend(score, 2)
    assert order == [[1, 2, 3], [4, 5]]      # node 3 (value 2) was dropped although it beats 3.0
    # the leaf's value is the one it was pushed with: node 2, value 1.0, wins over node 1's children
    assert (value, leaf, n_eval) == (1.0, 2, 5)
    np.testing.assert_array_equal(row, tree.data[2])
    # a root that is a leaf: (inf, data[indices[0]]) without a call; TypeError where it has no indices
    root_only = {"data": [[1.0, 2.0], [3.0, 4.0]], "features": [], "options": {}, "root": {"mean": [2.0, 3.0], "indices": [1, 0], "children": []}}
    t = HipFeatureClusterTree.from_json(root_only)
    v, r = t.find_best_example_excluding_search_candidates(lambda m, a: pytest.fail("called"), None, 3)
    assert np.isinf(v) and r.tolist() == [3.0, 4.0]
    root_only["root"]["indices"] = None
    with pytest.raises(TypeError):
        HipFeatureClusterTree.from_json(root_only).find_best_example_excluding_search_candidates(lambda m, a: 0.0, None, 1)


def test_equal_values_raise_type_error_like_the_reference():
    tree = HipFeatureClusterTree.from_json(_small_tree())
    with pytest.raises(TypeError):
        tree.find_best_example_excluding_search_candidates(lambda m, a: 1.0, None, 2)
    # a tie between leaves that only meet in the results heap's pop
    with pytest.raises(TypeError):
        tree.descend(lambda ids: {(1, 2, 3): [2.0, 1.0, 3.0], (4, 5): [1.0, 4.0]}[tuple(ids)], 2)


def test_synthetic_tree_survives_the_graph_zip(tmp_path):
    prims = synthetic.make_graph_primitives(2)
    lists = [{k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in p.items()} for p in prims]
    samples = np.random.default_rng(4).standard_normal((120, len(prims[0]["gmm_means"][0])))
    path = str(tmp_path / "graph.zip")
    synthetic.write_graph_zip(path, {"walk": {"primitives": {"a": lists[0], "b": lists[1]}, "info": {}}},
                              cluster_trees={("walk", "a"): synthetic.make_feature_cluster_tree(samples, 4, seed=2),
                                             ("walk", "b"): samples[:10]})
    nodes = model_io.read_graph_zip(path)["subgraphs"]["walk"]["nodes"]
    tree = HipFeatureClusterTree.from_json(nodes["a"]["space_partition_json"], n_spatial=len(prims[0]["eigen_vectors_spatial"]))
    np.testing.assert_array_equal(tree.data, samples)
    assert tree.n_nodes > 120
    assert nodes["b"]["space_partition_json"]["root"] == {}          # arrays keep today's stub
