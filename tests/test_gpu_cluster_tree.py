"""The reference's cluster-tree search (space_partitioning/feature_cluster_tree.py:129-187) in one launch
(mg_cluster_tree_search), against the reference's own answers (tests/golden/cluster_tree_search.npz) and, bit for bit,
against the host descent scoring each level with mg_score_constraints; its use by the sampling generator
("cluster_tree_search_method": "descend") and by the planner's option evaluation."""
import heapq
import json
import os

import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree, search_on_device
from morphablegraphs_amd.motion_primitive import get_context
from morphablegraphs_amd.motion_primitive_generator import HipMotionPrimitiveGenerator
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraph, HipMotionStateGraphNode
from oracle import mg_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "cluster_tree_search.npz"), allow_pickle=False)
CASES = list(enumerate(str(n) for n in GOLDEN["names"]))


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


class _Constraints(object):
    def __init__(self, cons, name="leftStance"):
        self.constraints, self.min_error, self.evaluations = list(cons), None, 0
        self.motion_primitive_name, self.use_local_optimization = name, False


def _golden_case(k):
    g = GOLDEN
    p = "c%d_" % k
    spec = json.loads(str(g[p + "primitive"]))
    data = getattr(synthetic, spec["factory"])(**spec["kwargs"])
    prev = g[p + "prev_frame"]
    return (data, json.loads(str(g[p + "tree_json"])), json.loads(str(g[p + "constraints"])), prev if prev.size else None,
            int(g[p + "n_candidates"]), g[p + "call_values"], float(g[p + "value"]), int(g[p + "row"]))


def _golden_set(prim, data, cons, prev):
    if prev is None:
        return _capi.ConstraintSet(prim, cons), None
    joints, animated = synthetic.make_skeleton(n_animated=(int(data["n_dim_spatial"]) - 3) // 4)
    sk = _capi.Skeleton(joints, animated)
    return _capi.ConstraintSet(prim, cons, sk, alignment=sk.alignment_to(prev, animated[0])), sk


@pytest.mark.parametrize("k,name", CASES)
def test_device_search_returns_the_references_row(k, name):
    data, tree_json, cons, prev, n, call_values, value, row = _golden_case(k)
    ctx = get_context(0)
    prim = _capi.Primitive(ctx, data)
    tree = HipFeatureClusterTree.from_json(tree_json, prim.n_components)
    cset, _ = _golden_set(prim, data, cons, prev)
    rec = search_on_device([(tree, prim, cset)], n)[0]
    assert rec["flags"] == 0
    assert rec["row"] == row, (name, rec)
    assert rec["evaluations"] == len(call_values)
    if np.isinf(value):
        assert np.isinf(rec["value"])
    else:
        np.testing.assert_allclose(rec["value"], value, rtol=1e-9, atol=1e-8)    # the scorer's contract with the oracle
    v, r = tree.result_of_record(rec)
    np.testing.assert_array_equal(r, tree.data[row])
    cset.close()
    tree.close()
    prim.close()


@pytest.fixture(scope="module")
def walk_tree():
    data = synthetic.make_walk_primitive(seed=0)
    samples = np.random.default_rng(11).standard_normal((10000, 40))
    return data, HipFeatureClusterTree.from_json(synthetic.make_feature_cluster_tree(samples, 4, seed=3), 40)


def test_one_launch_equals_the_host_descent_bit_for_bit(walk_tree):
    data, tree = walk_tree
    ctx = get_context(0)
    prim = _capi.Primitive(ctx, data)
    joints, animated = synthetic.make_skeleton()
    sk = _capi.Skeleton(joints, animated)
    cons = [{"type": "position", "t": 155.0, "weight": 1.0, "target": [60.0, None, -40.0]},
            {"type": "direction", "t": 155.0, "weight": 0.3, "target": [0.2, 1.0]},
            {"type": "joint_position", "joint": "LeftHand", "t": 80.0, "weight": 0.5, "target": [30.0, 100.0, -20.0]}]
    prev = np.zeros(79)
    prev[:3] = [120.0, 90.0, -340.0]
    prev[3::4] = 1.0
    prev[3:7] = [0.3, 0.1, 0.9, -0.2]
    sets = {"local": _capi.ConstraintSet(prim, cons, sk), "aligned": _capi.ConstraintSet(prim, cons, sk, alignment=sk.alignment_to(prev, 0))}
    try:
        for mode, cset in sets.items():
            for n in (1, 2, 5):
                rec = search_on_device([(tree, prim, cset)], n)[0]
                value, row, leaf, n_eval = tree.descend(lambda ids: prim.score_constraints(cset, tree.means[ids]), n)
                assert rec["flags"] == 0, (mode, n)
                assert rec["leaf"] == leaf and rec["row"] == tree.first_index[leaf], (mode, n)
                assert _bits(rec["value"]) == _bits(value), (mode, n, rec["value"], value)
                assert rec["evaluations"] == n_eval
                # the winner's value is what mg_score_constraints gives for its mean
                assert _bits(prim.score_constraints(cset, tree.means[leaf:leaf + 1])[0]) == _bits(rec["value"])
                np.testing.assert_array_equal(tree.result_of_record(rec)[1], row)
            assert search_on_device([(tree, prim, cset)], 5)[0]["evaluations"] > search_on_device([(tree, prim, cset)], 1)[0]["evaluations"]
    finally:
        for c in sets.values():
            c.close()
        prim.close()


def test_sixteen_searches_in_one_launch_equal_sixteen_calls():
    ctx = get_context(0)
    prims, trees, searches = [], [], []
    for p, data in enumerate(synthetic.make_graph_primitives(4, seed=300)):
        prim = _capi.Primitive(ctx, data)
        samples = np.random.default_rng(p).standard_normal((1500, prim.n_components + 2))    # wider than L: time latents
        tree = HipFeatureClusterTree.from_json(synthetic.make_feature_cluster_tree(samples, 4, seed=p), prim.n_components)
        prims.append(prim)
        trees.append(tree)
        t_end = float(prim.n_canonical_frames - 1)
        for q in range(4):
            cons = [{"type": "position", "t": t_end, "weight": 1.0, "target": [20.0 * q - 30.0, None, 15.0 * p]},
                    {"type": "direction", "t": 0.5 * t_end, "weight": 0.2, "target": [0.1 * q, 1.0]}]
            searches.append((tree, prim, _capi.ConstraintSet(prim, cons)))
    ctx.profile_enable(True)
    try:
        for n in (1, 3):
            ctx.profile_reset()
            together = search_on_device(searches, n)
            assert ctx.profile_get("cluster_tree_search")[1] == 1
            singles = np.concatenate([search_on_device([s], n) for s in searches])
            assert ctx.profile_get(11)[1] == 1 + len(searches)
            np.testing.assert_array_equal(together.view(np.uint8), singles.view(np.uint8))
            assert np.all(together["flags"] == 0) and len(set(together["row"].tolist())) > 4
    finally:
        ctx.profile_enable(False)
        for _, _, c in searches:
            c.close()
        for t in trees:
            t.close()
        for p in prims:
            p.close()


def test_generator_descend_and_search_best_sample():
    k = [i for i, nm in CASES if nm == "tiny_n2"][0]
    data, tree_json, cons, prev, n, call_values, value, row = _golden_case(k)
    node = HipMotionStateGraphNode()
    node.init_from_dict("walk", {"name": "leftStance", "mm": data})
    node.cluster_tree = HipFeatureClusterTree.from_json(tree_json, node.get_n_spatial_components())
    cfg = {"n_random_samples": 50, "use_constraints": True, "use_transition_model": False, "use_local_coordinates": True,
           "constrained_sampling_mode": "cluster_tree_search", "n_cluster_search_candidates": n,
           "local_optimization_settings": {"start_error_threshold": 0.0, "error_scale_factor": 1.0, "quality_scale_factor": 0.1,
                                           "method": "leastsq", "max_iterations": 50, "verbose": False}}
    gen = HipMotionPrimitiveGenerator({("walk", "leftStance"): node}, cfg, "walk")
    # default: the exhaustive search over .data, unchanged
    c = _Constraints(cons)
    pick = gen.generate_constrained_sample(node, c)
    op = orc.OraclePrimitive(data)
    stored = node.cluster_tree.data[:, :node.get_n_spatial_components()]
    best_idx, min_error = orc.first_min_argmin(op.keyframe_errors(stored, cons))
    np.testing.assert_array_equal(pick, stored[best_idx])
    assert c.evaluations == len(stored) and abs(c.min_error - min_error) <= 1e-8
    # "descend": the reference's row, min_error and number of objective calls
    gen.set_algorithm_config(dict(cfg, cluster_tree_search_method="descend"))
    c = _Constraints(cons)
    pick = gen.generate_constrained_sample(node, c)
    np.testing.assert_array_equal(pick, node.cluster_tree.data[row])
    np.testing.assert_allclose(c.min_error, value, rtol=1e-9, atol=1e-8)
    assert c.evaluations == len(call_values)
    # the host-driven descent (one scoring call per level) finds the same
    c2 = _Constraints(cons)
    err, s = node.search_best_sample_batched(c2, n)
    np.testing.assert_array_equal(s, node.cluster_tree.data[row])
    assert _bits(err) == _bits(c.min_error) and c2.evaluations == len(call_values)
    # the reference's surface method with a Python objective
    err, s = node.search_best_sample(lambda mean, args: float(op.keyframe_errors(mean[None, :], args)[0]), cons, n)
    assert err == value
    np.testing.assert_array_equal(s, node.cluster_tree.data[row])
    # a node with stored samples only cannot descend
    node.cluster_tree = type("Stub", (object,), {"data": stored})()
    with pytest.raises(NotImplementedError):
        gen.generate_constrained_sample(node, _Constraints(cons))


def test_evaluate_options_with_cluster_trees(tmp_path):
    prims = synthetic.make_graph_primitives(3, seed=500)
    lists = [{k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in p.items()} for p in prims]
    trees = {}
    for i, name in enumerate(("a", "b")):
        samples = np.random.default_rng(40 + i).standard_normal((800, len(prims[i]["gmm_means"][0])))
        trees[("walk", name)] = synthetic.make_feature_cluster_tree(samples, 4, seed=i)
    path = str(tmp_path / "graph.zip")
    synthetic.write_graph_zip(path, {"walk": {"primitives": {"a": lists[0], "b": lists[1], "c": lists[2]}, "info": {}}}, cluster_trees=trees)
    graph = HipMotionStateGraph().load_from_zip(path)
    try:
        for key in trees:
            assert isinstance(graph.nodes[key].cluster_tree, HipFeatureClusterTree)
            np.testing.assert_array_equal(graph.nodes[key].cluster_tree.data, np.asarray(trees[key]["data"]))
        options = [("walk", "a"), ("walk", "b"), ("walk", "c")]
        cons = {}
        for key in options:
            t_end = float(graph.nodes[key].get_n_canonical_frames() - 1)
            cons[key] = [{"type": "position", "t": t_end, "weight": 1.0, "target": [25.0, None, -10.0]}]
        ctx = graph.ctx
        ctx.profile_enable(True)
        ctx.profile_reset()
        try:
            best, results = graph.evaluate_options(options, cons, 64, rng_seed=3, use_cluster_trees=True)
            assert ctx.profile_get(11)[1] == 1          # both tree options in one launch
        finally:
            ctx.profile_enable(False)
        for key in trees:
            err, s = graph.nodes[key].search_best_sample_on_device(cons[key], 1)
            np.testing.assert_array_equal(results[key][0], s)
            assert _bits(results[key][1]) == _bits(err)
        assert np.isfinite(results[("walk", "c")][1])
        assert best == options[int(np.argmin([results[k][1] for k in options]))]
        # without the flag every option is evaluated by sampling, as before
        _, plain = graph.evaluate_options(options, cons, 64, rng_seed=3)
        np.testing.assert_array_equal(plain[("walk", "c")][0], results[("walk", "c")][0])
    finally:
        graph.close()


def test_misuse_returns_status_codes():
    ctx = get_context(0)
    data = synthetic.make_tiny_primitive(seed=1)
    prim = _capi.Primitive(ctx, data)
    other_prim = _capi.Primitive(ctx, synthetic.make_tiny_primitive(seed=2))
    samples = np.random.default_rng(0).standard_normal((50, 3))
    tree = HipFeatureClusterTree.from_json(synthetic.make_feature_cluster_tree(samples, 4, seed=0), 3)
    cset = _capi.ConstraintSet(prim, [{"type": "position", "t": 11.0, "weight": 1.0, "target": [1.0, None, 2.0]}])
    dev = tree.device_tree(prim)
    for n in (0, _capi.MG_TREE_MAX_CANDIDATES + 1, -1):
        with pytest.raises(_capi.MGError) as e:
            _capi.search_cluster_trees([prim], [dev], [cset], n)
        assert e.value.status == _capi.MG_ERR_INVALID_ARGUMENT
    with pytest.raises(_capi.MGError) as e:          # a set of another primitive
        _capi.search_cluster_trees([other_prim], [dev], [cset], 1)
    assert e.value.status == _capi.MG_ERR_INVALID_ARGUMENT
    ctx2 = _capi.Context(0)
    prim2 = _capi.Primitive(ctx2, data)
    dev2 = tree.device_tree(prim2)                     # one copy per context
    assert dev2 is not dev and tree.device_tree(prim) is dev
    with pytest.raises(_capi.MGError) as e:          # a tree uploaded to another context
        _capi.search_cluster_trees([prim], [dev2], [cset], 1)
    assert e.value.status == _capi.MG_ERR_INVALID_ARGUMENT
    # the C side validates the arrays itself: a cycle, a second parent, a leaf without a row, a width below L
    for cb, ch, fi, dim in (([0, 0, 1, 2], [2, 1], [-1, 0, 1], 3), ([0, 2, 2, 2], [1, 1], [-1, 0, 1], 3),
                            ([0, 2, 2, 2], [1, 2], [-1, 0, -1], 3), ([0, 2, 2, 2], [1, 2], [-1, 0, 1], 2)):
        with pytest.raises(_capi.MGError) as e:
            _capi.ClusterTree(prim, np.zeros((3, dim)), cb, ch, fi, 2)
        assert e.value.status == _capi.MG_ERR_INVALID_ARGUMENT
    ok = _capi.ClusterTree(prim, np.zeros((3, 3)), [0, 2, 2, 2], [1, 2], [-1, 0, 1], 2)
    ok.close()
    tree.close()
    cset.close()
    prim2.close()
    ctx2.close()
    other_prim.close()
    prim.close()


# ---- pins of the level loop's boundaries: hand-made trees on the tiny primitive, the device record against `descend` ----
_PIN_CONS = [{"type": "position", "t": 11.0, "weight": 1.0, "target": [40.0, None, -25.0]},
             {"type": "position", "t": 5.5, "weight": 0.5, "target": [10.0, 3.0, 20.0]}]


def _flat_tree(counts, means):
    """A feature tree from its nodes' child counts in breadth-first order (node 0 the root, children numbered consecutively);
    data = the means, and every leaf's row is its own node."""
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.sum() == len(counts) - 1 and means.shape[0] == len(counts)
    first = np.where(counts == 0, np.arange(len(counts)), -1)
    first[0] = -1 if counts[0] else 0
    return HipFeatureClusterTree(means, means, np.concatenate([[0], np.cumsum(counts)]), np.arange(1, len(counts)), first, n_spatial=3)


def _distinct_means(seed, n, dim=3):
    means = np.random.default_rng(seed).standard_normal((n, dim))
    assert len(np.unique(means, axis=0)) == n
    return means


def _by_score(score, means):
    """The rows of means, lowest objective first (the objectives all different)."""
    v = np.asarray(score(means))
    assert len(set(v.tolist())) == len(v)
    return means[np.argsort(v)]


def _spanning_tree(score, seed=7):
    """A root with three inner children whose 130 leaves the second level scores as chunks 64 | 64 | 2: in the frontier's order
    the nodes have 50, 14 and 66 children, so a node's last child falls inside a chunk (slot 49), on a chunk's last slot (63)
    and on the last slot in use of a short chunk, and the second and third chunk begin inside a node."""
    means = _distinct_means(seed, 134)
    heap = []
    for i, v in enumerate(score(means[1:4])):
        heapq.heappush(heap, (v, i))
    counts = [3, 0, 0, 0] + [0] * 130
    for rank, size in enumerate((50, 14, 66)):
        counts[1 + heap[rank][1]] = size
    return _flat_tree(counts, means)


def _tie_tree(score, at_pop):
    """at_pop False: a root with two leaves of one mean (heappush compares them).  True: three leaves a, b, b with a the
    strictly lowest: nothing compares the two b before the final heappop's _siftdown."""
    a, b = _by_score(score, _distinct_means(3, 2))
    means = np.stack([np.zeros(3), a, b, b] if at_pop else [np.zeros(3), a, a])
    return _flat_tree([len(means) - 1] + [0] * (len(means) - 1), means)


def _assert_record_is_descent(tree, prim, cset, n):
    rec = search_on_device([(tree, prim, cset)], n)[0]
    value, row, leaf, n_eval = tree.descend(lambda ids: prim.score_constraints(cset, np.ascontiguousarray(tree.means[ids, :prim.n_components])), n)
    assert rec["flags"] == 0
    assert (rec["leaf"], rec["row"], rec["evaluations"]) == (leaf, tree.first_index[leaf], n_eval)
    assert _bits(rec["value"]) == _bits(value)
    np.testing.assert_array_equal(tree.result_of_record(rec)[1], row)
    return rec


@pytest.fixture(scope="module")
def tiny():
    prim = _capi.Primitive(get_context(0), synthetic.make_tiny_primitive(seed=1))
    cset = _capi.ConstraintSet(prim, _PIN_CONS)
    yield prim, cset, lambda x: prim.score_constraints(cset, np.ascontiguousarray(x))
    cset.close()
    prim.close()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("children", [64, 65])
def test_a_level_of_one_chunk_and_of_one_more_child(tiny, children, n):
    prim, cset, _ = tiny
    tree = _flat_tree([children] + [0] * children, _distinct_means(children, children + 1))
    try:
        assert _assert_record_is_descent(tree, prim, cset, n)["evaluations"] == children
    finally:
        tree.close()


def test_chunks_that_span_frontier_nodes(tiny):
    prim, cset, score = tiny
    tree = _spanning_tree(score)
    try:
        assert _assert_record_is_descent(tree, prim, cset, 3)["evaluations"] == 133
    finally:
        tree.close()


@pytest.mark.parametrize("at_pop", [False, True])
def test_equal_values_flag_a_tie_at_push_and_at_the_final_pop(tiny, monkeypatch, at_pop):
    prim, cset, score = tiny
    tree = _tie_tree(score, at_pop)
    try:
        rec = search_on_device([(tree, prim, cset)], 3)[0]
        assert rec["flags"] & _capi.MG_TREE_TIE
        with pytest.raises(TypeError):
            tree.result_of_record(rec)
        with pytest.raises(TypeError):
            tree.descend(lambda ids: score(tree.means[ids]), 3)
        if at_pop:      # heappush alone never compares the two equal entries: only the last line of descend, the heappop, raises
            pushed, real = [], heapq.heappush
            monkeypatch.setattr(heapq, "heappush", lambda h, x: (real(h, x), pushed.append(x))[0])
            with pytest.raises(TypeError):
                tree.descend(lambda ids: score(tree.means[ids]), 3)
            monkeypatch.undo()
            assert len(pushed) == 9     # three pushes each on the node's, the level's and the results' heap: all went through
    finally:
        tree.close()


def test_w_read_from_memory_beyond_64_latents():
    data = synthetic.make_primitive(seed=5, n_components=68, n_frames=12, n_basis=7, n_dim=7, n_gmm=2, name="wide")
    prim = _capi.Primitive(get_context(0), data)
    cset = _capi.ConstraintSet(prim, _PIN_CONS)
    counts = [3, 2, 2, 2] + [0] * 6
    means = _distinct_means(68, len(counts), 68)
    first = np.where(np.asarray(counts) == 0, np.arange(len(counts)), -1)
    tree = HipFeatureClusterTree(means, means, np.concatenate([[0], np.cumsum(counts)]), np.arange(1, len(counts)), first, n_spatial=68)
    try:
        for n in (1, 2):
            _assert_record_is_descent(tree, prim, cset, n)
    finally:
        tree.close()
        cset.close()
        prim.close()
