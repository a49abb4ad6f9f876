"""Root trajectory constraints inside the one-launch cluster-tree search (mg_cluster_tree_search_trajectories), for both tree
kinds.  The yardstick is the host-driven descent (search_best_sample_batched), which scores every level through
errors_of_samples: mg_score_constraints, then mg_score_trajectory(..., accumulate = 1) per trajectory.  The one launch must
return the same sample, the same bits of the error and the same number of evaluations.  Inputs are seeded and continuous, so no
two children tie (flags == 0 is asserted)."""
import numpy as np
import pytest

from morphablegraphs_amd import _capi, candidate_scoring, synthetic
from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree, search_on_device
from morphablegraphs_amd.kd_cluster_tree import HipClusterTree
from morphablegraphs_amd.motion_primitive import get_context
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraph, HipMotionStateGraphNode

pytestmark = pytest.mark.gpu

KINDS = ("feature", "kd")
SPLINES = (_capi.MG_SPLINE_CATMULL_ROM, _capi.MG_SPLINE_BSPLINE, _capi.MG_SPLINE_FITTED_BSPLINE)
ALIGNMENTS = ("none", "previous", "start_pose")


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


class _Constraints(object):
    def __init__(self, cons, start_pose=None):
        self.constraints, self.min_error, self.evaluations = list(cons), None, 0
        self.motion_primitive_name, self.use_local_optimization = "tiny", False
        self.is_local, self.start_pose = False, start_pose


def _make_tree(kind, samples, n_spatial, seed):
    if kind == "feature":
        return HipFeatureClusterTree.from_json(synthetic.make_feature_cluster_tree(samples, 8, seed=seed), n_spatial)
    return HipClusterTree.from_reference(synthetic.make_kd_cluster_tree(samples, 8, 6, seed=seed), n_spatial)


def _make_node(ctx, data, kind, seed, n_samples=700):
    node = HipMotionStateGraphNode(context=ctx)
    node.init_from_dict("walk", {"name": str(data.get("name", "tiny")), "mm": data})
    L = node.get_n_spatial_components()
    node.cluster_tree = _make_tree(kind, np.random.default_rng(seed).standard_normal((n_samples, L)), L, seed)
    return node


def _mean_path(node):
    """the root path of the zero latent: what the trajectories are laid along"""
    prim = node.motion_primitive._prim
    return np.asarray(prim.back_project_frames(np.zeros((1, prim.n_components), dtype=np.float32)), dtype=np.float64)[0, :, :3]


def _trajectory(path, seed, spline_type=0, min_u=0.0, weight=1.0, offset=(0.0, 0.0, 0.0), part=1.0, n_points=6):
    """n_points control points along the first `part` of `path`, jittered (seeded) and moved by `offset`"""
    rng = np.random.default_rng(seed)
    last = max(int(round(part * (len(path) - 1))), 1)
    pts = path[np.linspace(0, last, n_points).round().astype(int)] + rng.uniform(-3.0, 3.0, (n_points, 3)) + np.asarray(offset)
    c = {"type": "trajectory", "control_points": pts.tolist(), "min_u": float(min_u), "weight": float(weight), "granularity": 1000}
    if spline_type:
        c["spline_type"] = int(spline_type)
    return c


def _lists(path, spline_type):
    kf = [{"type": "position", "t": 11.0, "weight": 1.0, "target": [40.0, None, -25.0]},
          {"type": "direction", "t": 5.5, "weight": 0.3, "target": [0.2, 1.0]}]
    return {"trajectory_only": [_trajectory(path, 1, spline_type)],
            "two_keyframes_one_trajectory": kf + [_trajectory(path, 2, spline_type)],
            "one_keyframe_two_trajectories": [kf[0], _trajectory(path, 3, spline_type, min_u=0.15, weight=0.7),
                                              _trajectory(path, 4, spline_type, min_u=0.05, weight=2.5, offset=(10.0, 0.0, -6.0))]}


def _alignment_args(mode):
    """(prev_frames, start_pose) of an alignment mode"""
    if mode == "previous":
        return np.asarray([12.0, 80.0, -5.0, 0.9, 0.1, 0.3, 0.2]), None
    if mode == "start_pose":
        return None, {"position": [3.0, 7.5, -2.0], "orientation": [0.0, 35.0, 0.0]}
    return None, None


def _device_record(node, cons, n, prev, start_pose):
    c = _Constraints(cons, start_pose)
    sset = node._tree_search_set(c, prev, None)
    assert sset is not None, "the one launch does not take this list"
    try:
        rec = search_on_device([(node.cluster_tree, node.motion_primitive._prim, sset)], n)[0]
    finally:
        sset.release()
    assert rec["flags"] == 0, "a tie or an overflow: pick another seed"
    return rec


def _assert_same_as_batched(node, cons, n, prev=None, start_pose=None, what=""):
    rec = _device_record(node, cons, n, prev, start_pose)
    c = _Constraints(cons, start_pose)
    value, sample = node.search_best_sample_batched(c, n, prev)
    np.testing.assert_array_equal(np.asarray(node.cluster_tree.result_of_record(rec)[1]), np.asarray(sample), err_msg=what)
    assert _bits(rec["value"]) == _bits(value), (what, rec["value"], value)
    assert rec["evaluations"] == c.evaluations, what
    return rec


@pytest.fixture(scope="module")
def ctx():
    c = get_context(0)
    yield c
    c.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
    candidate_scoring.clear_constraint_cache()


@pytest.fixture(scope="module")
def nodes(ctx):
    out = {kind: _make_node(ctx, synthetic.make_tiny_primitive(seed=1), kind, 21 + i) for i, kind in enumerate(KINDS)}
    yield out
    candidate_scoring.clear_constraint_cache()
    for node in out.values():
        node.cluster_tree.close()
        node.motion_primitive._prim.close()


def test_search_best_sample_on_device_takes_a_trajectory_list(ctx, nodes):
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
    node = nodes["feature"]
    cons = _lists(_mean_path(node), 0)["two_keyframes_one_trajectory"]
    c1, c2 = _Constraints(cons), _Constraints(cons)
    err, sample = node.search_best_sample_on_device(c1, 2)
    value, row = node.search_best_sample_batched(c2, 2)
    np.testing.assert_array_equal(sample, row)
    assert _bits(err) == _bits(value) and c1.evaluations == c2.evaluations > 0


@pytest.mark.parametrize("search", [0, 1])
@pytest.mark.parametrize("alignment", ALIGNMENTS)
@pytest.mark.parametrize("kind", KINDS)
def test_one_launch_equals_the_batched_descent(ctx, nodes, kind, alignment, search):
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
    node = nodes[kind]
    path = _mean_path(node)
    prev, start_pose = _alignment_args(alignment)
    for spline_type in SPLINES:
        for name, cons in _lists(path, spline_type).items():
            for n in (1, 2, 9):
                _assert_same_as_batched(node, cons, n, prev, start_pose, what=(kind, alignment, search, spline_type, name, n))


@pytest.mark.parametrize("kind", KINDS)
def test_nine_candidates_score_a_level_in_two_chunks(ctx, nodes, kind, monkeypatch):
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
    node = nodes[kind]
    sizes, real = [], candidate_scoring.errors_of_samples
    monkeypatch.setattr(candidate_scoring, "errors_of_samples", lambda prim, form, sk, al, S: (sizes.append(len(S)), real(prim, form, sk, al, S))[1])
    _assert_same_as_batched(node, _lists(_mean_path(node), 0)["two_keyframes_one_trajectory"], 9)
    assert max(sizes) > 64, sizes


@pytest.mark.parametrize("search", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_far_trajectories_and_paths_that_run_past_the_end(ctx, nodes, kind, search):
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
    node = nodes[kind]
    path = _mean_path(node)
    far = [_trajectory(path, 5, offset=(4000.0, 0.0, -2500.0))]                     # long walks from every child's path
    short = [_trajectory(path, 6, part=0.3, n_points=4), {"type": "position", "t": 11.0, "weight": 0.5, "target": [10.0, None, 5.0]}]
    for name, cons in (("far", far), ("past_the_end", short)):
        for n in (1, 2):
            _assert_same_as_batched(node, cons, n, what=(kind, search, name, n))


@pytest.mark.parametrize("kind", KINDS)
def test_three_searches_side_by_side_equal_each_alone(ctx, kind):
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
    made = [_make_node(ctx, data, kind, 70 + i, n_samples=300) for i, data in enumerate(synthetic.make_graph_primitives(3, seed=900))]
    sets = []
    try:
        for i, node in enumerate(made):
            cons = [{"type": "position", "t": float(node.get_n_canonical_frames() - 1), "weight": 1.0, "target": [20.0 * i, None, -10.0]},
                    _trajectory(_mean_path(node), 30 + i, SPLINES[i], min_u=0.1 * i, weight=1.0 + i)]
            sets.append(node._tree_search_set(_Constraints(cons), None, None))
        searches = [(node.cluster_tree, node.motion_primitive._prim, s) for node, s in zip(made, sets)]
        together = search_on_device(searches, 2)
        alone = np.concatenate([search_on_device([s], 2) for s in searches])
        assert np.all(together["flags"] == 0)
        np.testing.assert_array_equal(together.view(np.uint8), alone.view(np.uint8))
    finally:
        for s in sets:
            s.release()
        candidate_scoring.clear_constraint_cache()
        for node in made:
            node.cluster_tree.close()
            node.motion_primitive._prim.close()


def test_a_single_search_is_one_launch(ctx, nodes):
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
    node = nodes["feature"]
    cons = _lists(_mean_path(node), 0)["one_keyframe_two_trajectories"]
    node.search_best_sample_on_device(_Constraints(cons), 2)      # (the device objects exist before the counted call)
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        node.search_best_sample_on_device(_Constraints(cons), 2)
        assert ctx.profile_get("cluster_tree_search")[1] == 1 and ctx.profile_get(10)[1] == 0
    finally:
        ctx.profile_enable(False)


def test_evaluate_options_with_trajectories_is_one_launch(tmp_path):
    prims = synthetic.make_graph_primitives(3, seed=500)
    lists = [{k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in p.items()} for p in prims]
    trees = {}
    for i, name in enumerate(("a", "b")):
        samples = np.random.default_rng(40 + i).standard_normal((400, len(prims[i]["gmm_means"][0])))
        trees[("walk", name)] = synthetic.make_feature_cluster_tree(samples, 4, seed=i)
    path = str(tmp_path / "graph.zip")
    synthetic.write_graph_zip(path, {"walk": {"primitives": {"a": lists[0], "b": lists[1], "c": lists[2]}, "info": {}}}, cluster_trees=trees)
    graph = HipMotionStateGraph().load_from_zip(path)
    ctx = graph.ctx
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
    try:
        options = [("walk", "a"), ("walk", "b"), ("walk", "c")]
        cons = {}
        for i, key in enumerate(options):
            node = graph.nodes[key]
            t_end = float(node.get_n_canonical_frames() - 1)
            cons[key] = [{"type": "position", "t": t_end, "weight": 1.0, "target": [25.0, None, -10.0]}]
            if key in trees:
                cons[key].append(_trajectory(_mean_path(node), 50 + i))
        ctx.profile_enable(True)
        ctx.profile_reset()
        try:
            best, results = graph.evaluate_options(options, cons, 64, rng_seed=3, use_cluster_trees=True)
            # both tree options in one launch, their trajectories scored inside it
            assert ctx.profile_get(11)[1] == 1 and ctx.profile_get(10)[1] == 0
        finally:
            ctx.profile_enable(False)
        for key in trees:
            c = _Constraints(cons[key])
            err, s = graph.nodes[key].search_best_sample_batched(c, 1)
            np.testing.assert_array_equal(results[key][0], s)
            assert _bits(results[key][1]) == _bits(err)
        assert np.isfinite(results[("walk", "c")][1])
        assert best == options[int(np.argmin([results[k][1] for k in options]))]
    finally:
        candidate_scoring.clear_constraint_cache()
        graph.close()


@pytest.mark.parametrize("kind", KINDS)
def test_zero_trajectories_give_the_records_of_the_plain_entry_point(ctx, nodes, kind):
    node = nodes[kind]
    prim = node.motion_primitive._prim
    cset = _capi.ConstraintSet(prim, _lists(_mean_path(node), 0)["two_keyframes_one_trajectory"][:2])
    dev = node.cluster_tree.device_tree(prim)
    try:
        for n in (1, 3):
            plain = _capi.search_cluster_trees([prim, prim], [dev, dev], [cset, cset], n)
            new = _capi.search_cluster_trees([prim, prim], [dev, dev], [cset, cset], n, trajectories=[[], []], alignments=[None, None])
            np.testing.assert_array_equal(plain.view(np.uint8), new.view(np.uint8))
    finally:
        cset.close()


def test_misuse_returns_status_codes(ctx, nodes):
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
    node, kd = nodes["feature"], nodes["kd"]
    prim, kd_prim = node.motion_primitive._prim, kd.motion_primitive._prim
    path = _mean_path(node)
    cset = _capi.ConstraintSet(prim, [{"type": "position", "t": 11.0, "weight": 1.0, "target": [1.0, None, 2.0]}])
    kd_cset = _capi.ConstraintSet(kd_prim, [{"type": "position", "t": 11.0, "weight": 1.0, "target": [1.0, None, 2.0]}])
    traj = _capi.Trajectory(prim, _trajectory(path, 8)["control_points"])
    kd_traj = _capi.Trajectory(kd_prim, _trajectory(path, 8)["control_points"])
    dev, kd_dev = node.cluster_tree.device_tree(prim), kd.cluster_tree.device_tree(kd_prim)
    one = [(traj, 0.0, 1.0)]
    root_record = {"joint": 0, "position": (1.0, 2.0, 3.0), "heading": (0.6, 0.8), "ref_dir": (0.0, 0.0, 1.0)}

    def status(prims, devs, csets, trajectories, alignments):
        with pytest.raises(_capi.MGError) as e:
            _capi.search_cluster_trees(prims, devs, csets, 1, trajectories=trajectories, alignments=alignments)
        return e.value.status
    try:
        ctx.profile_enable(True)
        ctx.profile_reset()
        assert status([prim], [dev], [cset], [one * (_capi.MG_TREE_MAX_TRAJECTORIES + 1)], [None]) == _capi.MG_ERR_INVALID_ARGUMENT
        assert status([prim], [dev], [cset], [[(None, 0.0, 1.0)]], [None]) == _capi.MG_ERR_INVALID_ARGUMENT
        assert status([prim], [dev], [cset], [[(kd_traj, 0.0, 1.0)]], [None]) == _capi.MG_ERR_INVALID_ARGUMENT      # another primitive's
        assert status([prim], [dev], [cset], [one], [dict(root_record, joint=2)]) == _capi.MG_ERR_UNSUPPORTED
        assert status([prim, kd_prim], [dev, kd_dev], [cset, kd_cset], [one, [(kd_traj, 0.0, 1.0)]], [None, None]) == _capi.MG_ERR_INVALID_ARGUMENT
        assert ctx.profile_get(11)[1] == 0           # nothing was launched
        ctx.profile_enable(False)
        rec = _capi.search_cluster_trees([prim], [dev], [cset], 1, trajectories=[one * _capi.MG_TREE_MAX_TRAJECTORIES], alignments=[root_record])
        assert rec["flags"][0] == 0 and np.isfinite(rec["value"][0])
        # a full list, one wave per trajectory: the host-driven descent's record
        # (the set aligned like the trajectories, as the descent's scorers build it)
        tree, form = node.cluster_tree, [{"type": "position", "t": 11.0, "weight": 1.0, "target": [1.0, None, 2.0]}] + [_trajectory(path, 8)] * 4
        aligned = _capi.ConstraintSet(prim, form[:1], None, root_record)
        try:
            rec = _capi.search_cluster_trees([prim], [dev], [aligned], 1, trajectories=[one * _capi.MG_TREE_MAX_TRAJECTORIES], alignments=[root_record])
        finally:
            aligned.close()
        assert rec["flags"][0] == 0
        value, _, leaf, n_eval = tree.descend(lambda ids: candidate_scoring.errors_of_samples(prim, form, None, root_record, tree.means[ids, :prim.n_components]), 1)
        assert (rec["leaf"][0], rec["row"][0], rec["evaluations"][0]) == (leaf, tree.first_index[leaf], n_eval)
        assert _bits(rec["value"][0]) == _bits(value), (rec["value"][0], value)
    finally:
        ctx.profile_enable(False)
        for obj in (traj, kd_traj, cset, kd_cset):
            obj.close()
