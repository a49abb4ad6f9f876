"""Cluster trees built on the device (mg_kmeans_segments, cluster_tree_builder.py): every k-means call the reference made
(tests/golden/cluster_tree_build.npz) replayed from its initial centres gives sklearn's labels, iteration counts, centres and
inertia; whole trees built from those initial centres, a level per call, are the reference's trees; the default seeded build
of 10 000 device samples is bit-reproducible, valid, a Lloyd fixed point per node and searchable; n_init keeps the best run;
unsupported shapes are refused; a graph without trees gets both kinds from HipClusterTreeBuilder and evaluate_options searches
them."""
import json
import os
import sys
import zipfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_cluster_tree_build_host import NAMES, Recorded, assert_is_golden_tree, build, case, tree_depth  # noqa: E402

from morphablegraphs_amd import _capi, synthetic  # noqa: E402
from morphablegraphs_amd import cluster_tree_builder as ctb  # noqa: E402
from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree, search_on_device  # noqa: E402
from morphablegraphs_amd.cluster_tree_pickle import load_cluster_tree_pickle  # noqa: E402
from morphablegraphs_amd.kd_cluster_tree import HipClusterTree  # noqa: E402
from morphablegraphs_amd.motion_primitive import get_context  # noqa: E402
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraph  # noqa: E402

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def _inertia_ok(got, want, x):
    """Within 1e-12 relative -- of the segment's total sum of squares where sklearn's inertia is (near) zero: a cluster of
    identical rows has inertia 0 in sklearn's centred coordinates and a few ulps of the rows' magnitude here."""
    tss = float(((x - x.mean(axis=0)) ** 2).sum())
    return abs(float(got) - float(want)) <= 1e-12 * max(abs(float(want)), tss)


def _points(c):
    opts = json.loads(str(c["options"]))
    if str(c["kind"]) == "kd":
        return np.ascontiguousarray(c["data"][:, :opts["dim"]]), opts["n_subdivisions"]
    return np.ascontiguousarray(c["features"] if "features" in c else c["data"]), opts["n_subdivisions"]


@pytest.mark.parametrize("name", NAMES)
def test_every_recorded_call_in_one_invocation(name):
    """All of a case's sklearn calls as the segments of ONE mg_kmeans_segments call, from sklearn's initial centres."""
    c = case(name)
    rec = Recorded(c)
    X, k = _points(c)
    ctx = get_context(0)
    keys = list(rec.calls)
    rows = np.concatenate([np.asarray(key, dtype=np.int64) for key in keys])
    seg_begin = np.concatenate([[0], np.cumsum([len(key) for key in keys])])
    init = np.stack([rec.calls[key]["init"] for key in keys])
    d_x = ctx.upload(X)
    try:
        labels, centres, inertia, n_iter = _capi.kmeans_segments(ctx, d_x, X.shape[0], X.shape[1], seg_begin, rows, k, init=init)
    finally:
        d_x.free()
    for s, key in enumerate(keys):
        want = rec.calls[key]
        np.testing.assert_array_equal(labels[seg_begin[s]:seg_begin[s + 1]], want["labels"], err_msg="%s call %d" % (name, s))
        assert n_iter[s] == want["n_iter"], (name, s, n_iter[s], want["n_iter"])
        assert _rel(centres[s], want["centres"]) <= 1e-12, (name, s)
        assert _inertia_ok(inertia[s], want["inertia"], X[list(key)]), (name, s, inertia[s], want["inertia"])


class Checked(object):
    """A DeviceKMeans from the recorded initial centres whose answers, a level per call, are compared with sklearn's."""

    def __init__(self, c):
        self.rec = Recorded(c)
        X, k = _points(c)
        self.X = X
        self.km = ctb.DeviceKMeans(get_context(0), X, k, init=self.rec.init)
        self.levels = 0

    def __call__(self, seg_begin, rows, node_ids):
        labels = self.km(seg_begin, rows, node_ids)
        last = self.km.last
        for s in range(len(seg_begin) - 1):
            want = self.rec.calls[tuple(rows[seg_begin[s]:seg_begin[s + 1]].tolist())]
            np.testing.assert_array_equal(labels[seg_begin[s]:seg_begin[s + 1]], want["labels"])
            assert last["n_iter"][s] == want["n_iter"]
            assert _rel(last["centres"][s], want["centres"]) <= 1e-12
            assert _inertia_ok(last["inertia"][s], want["inertia"], self.X[rows[seg_begin[s]:seg_begin[s + 1]]])
        self.levels += 1
        return labels


@pytest.mark.parametrize("name", NAMES)
def test_device_build_from_the_recorded_inits_is_the_references_tree(name):
    c = case(name)
    km = Checked(c)
    try:
        tree = build(c, km)
    finally:
        km.km.close()
    assert_is_golden_tree(tree, c)
    assert km.levels == km.km.calls and km.levels <= tree_depth(tree) + 1


@pytest.fixture(scope="module")
def walk():
    data = synthetic.make_walk_primitive(seed=0)
    ctx = get_context(0)
    prim = _capi.Primitive(ctx, data)
    counts = np.random.default_rng(5).multinomial(10000, np.asarray(data["gmm_weights"], dtype=np.float64))
    X, _ = prim.gmm_sample(counts, 5)
    yield ctx, prim, np.ascontiguousarray(X[:, :40], dtype=np.float64)
    prim.close()


class Logged(object):
    def __init__(self, ctx, X, k, **kw):
        self.km = ctb.DeviceKMeans(ctx, X, k, **kw)
        self.log = []

    def __call__(self, seg_begin, rows, node_ids):
        labels = self.km(seg_begin, rows, node_ids)
        self.log.append((np.array(seg_begin), np.array(rows), labels.copy(), self.km.last["centres"].copy(), self.km.last["n_iter"].copy()))
        return labels


def _tables(tree):
    names = ("points", "child_begin", "children", "leaf", "kd_begin", "kd_roots", "kd_left", "kd_right", "kd_inner") if isinstance(tree, HipClusterTree) \
        else ("means", "child_begin", "children", "first_index")
    return [np.ascontiguousarray(getattr(tree, n)).tobytes() for n in names]


def _outcome(fn):
    try:
        value, sample = fn()
    except (AttributeError, TypeError) as e:
        return ("raised", type(e).__name__)
    return ("answer", np.float64(value).view(np.uint64).item(), np.asarray(sample, dtype=np.float64).tobytes())


@pytest.mark.parametrize("kind", ["kd", "feature"])
def test_seeded_build_of_the_walk_primitive(walk, kind):
    ctx, prim, X = walk

    def make(**kw):
        if kind == "kd":
            return ctb.build_kd_cluster_tree(X, 4, 4, ctx=ctx, seed=11, n_spatial=40, **kw)
        return ctb.build_feature_cluster_tree(X, X, 4, ctx=ctx, seed=11, n_spatial=40, **kw)
    t1, t2 = make(), make()
    assert _tables(t1) == _tables(t2)
    t1.validate(40)
    assert t1.n_nodes > 50
    # every node's k-means: the labels are the nearest centres, and with tol = 0 (strict convergence) the centres are the
    # members' means
    km = Logged(ctx, X, 4, seed=11, tol=0.0)
    try:
        if kind == "kd":
            ctb.build_kd_cluster_tree(X, 4, 4, kmeans=km)
        else:
            ctb.build_feature_cluster_tree(X, X, 4, kmeans=km)
    finally:
        km.km.close()
    checked = 0
    for seg_begin, rows, labels, centres, n_iter in km.log:
        for s in range(len(seg_begin) - 1):
            x = X[rows[seg_begin[s]:seg_begin[s + 1]]]
            lab = labels[seg_begin[s]:seg_begin[s + 1]]
            d = ((x[:, None, :] - centres[s][None, :, :]) ** 2).sum(axis=2)
            np.testing.assert_array_equal(np.argmin(d, axis=1), lab)
            assert n_iter[s] < 300
            for j in np.unique(lab):
                assert _rel(centres[s][j], x[lab == j].mean(axis=0)) <= 1e-12
            checked += 1
    assert checked > 10
    # the built tree searched in one launch: the host descent's answer (with 4 levels over 10 000 samples a node at depth 4
    # has KD-tree children and no leaf flag, so both raise the reference's AttributeError where the search reaches one; a
    # 16-level tree ends in leaves)
    trees = [t1] + ([ctb.build_kd_cluster_tree(X, 4, 16, ctx=ctx, seed=11, n_spatial=40)] if kind == "kd" else [])
    joints, animated = synthetic.make_skeleton()
    sk = _capi.Skeleton(joints, animated)
    answers = 0
    for cons in ([{"type": "position", "t": 155.0, "weight": 1.0, "target": [60.0, None, -40.0]}],
                 [{"type": "position", "t": 80.0, "weight": 1.0, "target": [10.0, 90.0, 30.0]},
                  {"type": "direction", "t": 155.0, "weight": 0.3, "target": [0.2, 1.0]}]):
        cset = _capi.ConstraintSet(prim, cons, sk)
        try:
            def obj(x, data):
                return float(prim.score_constraints(cset, np.ascontiguousarray(np.asarray(x, dtype=np.float64)[None, :40]))[0])
            for tree in trees:
                for n in (1, 3):
                    rec = search_on_device([(tree, prim, cset)], n)[0]
                    got, want = _outcome(lambda: tree.result_of_record(rec)), _outcome(lambda: tree.find_best_example_excluding_search_candidates(obj, None, n))
                    assert got == want, (kind, n)
                    answers += got[0] == "answer"
        finally:
            cset.close()
    assert answers >= 2
    for tree in trees[1:]:
        tree.close()
    t1.close()
    t2.close()


def test_n_init_keeps_the_least_inertia_run(walk):
    ctx, _, X = walk
    rng = np.random.default_rng(8)
    rows = np.concatenate([rng.permutation(10000)[:n] for n in (3000, 500, 64, 700)]).astype(np.int64)
    seg_begin = np.array([0, 3000, 3500, 3564, 4264])
    d_x = ctx.upload(X)
    try:
        one = _capi.kmeans_segments(ctx, d_x, 10000, 40, seg_begin, rows, 6, n_init=1, seed=3)
        many = _capi.kmeans_segments(ctx, d_x, 10000, 40, seg_begin, rows, 6, n_init=8, seed=3)
        again = _capi.kmeans_segments(ctx, d_x, 10000, 40, seg_begin, rows, 6, n_init=8, seed=3)
    finally:
        d_x.free()
    for a, b in zip(many, again):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    # run 0 of eight is the single run (the same Philox key): the best of eight is never worse, here better somewhere
    assert np.all(many[2] <= one[2]) and np.any(many[2] < one[2])
    for s in range(4):
        x = X[rows[seg_begin[s]:seg_begin[s + 1]]]
        lab = many[0][seg_begin[s]:seg_begin[s + 1]]
        assert _rel(((x - many[1][s][lab]) ** 2).sum(), many[2][s]) <= 1e-10


def test_unsupported_shapes_are_refused_and_the_context_stays_usable(walk):
    ctx, _, X = walk
    d_x = ctx.upload(X)
    try:
        rows = np.arange(200, dtype=np.int64)
        for k, n_init in ((1, 1), (65, 1), (4, 17)):
            with pytest.raises(_capi.MGError) as e:
                _capi.kmeans_segments(ctx, d_x, 10000, 40, [0, 200], rows, k, n_init=n_init)
            assert e.value.status == _capi.MG_ERR_UNSUPPORTED
        wide = ctx.upload(np.zeros((10, 129)))
        try:
            with pytest.raises(_capi.MGError) as e:
                _capi.kmeans_segments(ctx, wide, 10, 129, [0, 10], np.arange(10), 2)
            assert e.value.status == _capi.MG_ERR_UNSUPPORTED
        finally:
            wide.free()
        with pytest.raises(_capi.MGError) as e:
            _capi.kmeans_segments(ctx, d_x, 10000, 40, [0, 3], np.arange(3), 4)     # fewer rows than k
        assert e.value.status == _capi.MG_ERR_INVALID_ARGUMENT
        labels, centres, inertia, n_iter = _capi.kmeans_segments(ctx, d_x, 10000, 40, [0, 200], rows, 4)
        assert labels.shape == (200,) and set(np.unique(labels)) <= set(range(4)) and np.isfinite(inertia).all()
    finally:
        d_x.free()


def _graph_zip(path):
    prims = synthetic.make_graph_primitives(3, seed=500)
    lists = [{k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in p.items()} for p in prims]
    synthetic.write_graph_zip(path, {"walk": {"primitives": {"a": lists[0], "b": lists[1], "c": lists[2]}, "info": {}}}, format_version=4.0)
    with zipfile.ZipFile(path, "r") as z:
        entries = {n: z.read(n) for n in z.namelist()}
    entries["graph_definition.json"] = b'{"formatVersion": 4.0, "transitions": {}}'
    with zipfile.ZipFile(path, "w") as z:
        for n, b in entries.items():
            z.writestr(n, b)


def test_builder_gives_a_graph_without_trees_both_kinds(tmp_path):
    path = str(tmp_path / "graph.zip")
    _graph_zip(path)
    graph = HipMotionStateGraph().load_from_zip(path)
    try:
        assert all(node.cluster_tree is None for node in graph.nodes.values())
        config = {"model_data_dir": str(tmp_path), "n_random_samples": 2000, "n_subdivisions_per_level": 4, "n_levels": 4, "random_seed": 7,
                  "only_spatial_parameters": True, "store_data_indices_in_nodes": False, "use_kd_tree": True}
        kd = ctb.HipClusterTreeBuilder({"tree_type": ctb.TREE_TYPE_CLUSTER_TREE, "feature_type": ctb.FEATURE_TYPE_S_VECTOR, "output_mode": "pck"})
        kd.set_config(config)
        ft = ctb.HipClusterTreeBuilder({"tree_type": ctb.TREE_TYPE_FEATURE_CLUSTER_TREE, "feature_type": ctb.FEATURE_TYPE_S_VECTOR,
                                        "output_mode": "json"})
        ft.set_config(config)
        np.random.seed(1)
        a, b = graph.nodes[("walk", "a")], graph.nodes[("walk", "b")]
        assert isinstance(kd.build_for_node(a), HipClusterTree)
        assert isinstance(ft.build_for_node(b), HipFeatureClusterTree)
        assert a.cluster_tree.data.shape[0] == 2000 and b.cluster_tree.data.shape[0] == 2000
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
            assert ctx.profile_get(11)[1] == 2          # one launch per tree kind
        finally:
            ctx.profile_enable(False)
        for key in options[:2]:
            err, s = graph.nodes[key].search_best_sample_on_device(cons[key], 1)
            np.testing.assert_array_equal(np.asarray(results[key][0]), np.asarray(s))
            assert np.float64(results[key][1]).view(np.uint64) == np.float64(err).view(np.uint64)
        # the reference's search with a Python objective, through search_best_sample
        prim = a.motion_primitive._prim
        cset = _capi.ConstraintSet(prim, cons[("walk", "a")])
        try:
            L = a.get_n_spatial_components()
            v, sample = a.search_best_sample(lambda x, data: float(prim.score_constraints(cset, np.asarray(x, dtype=np.float64)[None, :L])[0]), None, 1)
            assert np.isfinite(v) and len(sample) == a.cluster_tree.data.shape[1]
        finally:
            cset.close()
        # the writers: the reference's file names, loaded back into the same tables
        os.makedirs(str(tmp_path / "walk"), exist_ok=True)
        t_kd = kd._build_tree(str(tmp_path / "walk"), "walk_a_quaternion", a.cluster_tree.data, a)
        t_ft = ft._build_feature_tree("walk", "walk_b_quaternion", b.cluster_tree.data, b)
        assert _tables(t_kd) == _tables(a.cluster_tree) and _tables(t_ft) == _tables(b.cluster_tree)
        back = load_cluster_tree_pickle(str(tmp_path / "walk" / "walk_a_quaternion_cluster_tree.pck"))
        assert _tables(back) == _tables(t_kd)
        with open(str(tmp_path / "walk" / "walk_b_quaternion_cluster_tree.json")) as f:
            assert _tables(HipFeatureClusterTree.from_json(json.load(f))) == _tables(t_ft)
    finally:
        graph.close()
