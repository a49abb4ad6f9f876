"""The one-launch tree search with per-frame constraint lists (mg_cluster_tree_search_frames): the GPU half of
tests/tree_search_frames_cases.py.  Every row of the table: the plan query of the actual call equals the row's claim; the one launch
returns the leaf, the sample and the evaluation count of the host-driven descent (search_best_sample_batched's scoring path) on the same
tree; its error agrees with errors_of_samples of the returned sample and with oracle.mg_oracle's value, under the tolerance
tests/test_gpu_frame_constraints.py holds the per-frame scorers to against the oracle.  Then: one launch mixing searches with and without
lists against the same searches alone, and a shape no rung takes (MG_ERR_UNSUPPORTED, the Python route falls back)."""
import types

import numpy as np
import pytest

import tree_search_cases as sc
import tree_search_frames_cases as fc
from morphablegraphs_amd import _capi, candidate_scoring, frame_constraints
from morphablegraphs_amd.candidate_scoring import alignment_from_start_pose, errors_of_samples
from morphablegraphs_amd.cluster_tree import TreeSearchSet, frames_search_plan, search_on_device
from morphablegraphs_amd.motion_primitive_generator import HipMotionPrimitiveGenerator
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraphNode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    candidate_scoring.clear_constraint_cache()
    c.close()


@pytest.fixture(scope="module")
def prims(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _capi.Primitive(ctx, fc.model(name))
        return made[name]
    yield get
    candidate_scoring.clear_constraint_cache()
    for p in made.values():
        p.close()


def alignment(r, sk):
    if r["align"] == 1:
        al = sk.alignment_to(fc.PREV[r["prim"]], 0)
        return {"joint": 0, "position": al["position"], "heading": al["heading"]}
    return alignment_from_start_pose(sc.START_POSE) if r["align"] == 2 else None


class Search(object):
    """One row's device objects: the tree, the keyframe set, the trajectories, the per-frame list"""

    def __init__(self, prim, r, with_frames=True):
        self.prim, self.r = prim, r
        self.sk = _capi.Skeleton(*fc.SKELETONS[r["prim"]])
        self.al = alignment(r, self.sk)
        self.cons = fc.constraints_of(r)
        frames = [c for c in self.cons if frame_constraints.is_frame_constraint(c)]
        if not with_frames:
            self.cons = [c for c in self.cons if not frame_constraints.is_frame_constraint(c)]
        self.kf, self.trajs = candidate_scoring.split_trajectories([c for c in self.cons if not frame_constraints.is_frame_constraint(c)])
        self.tree = fc.kd_tree(r) if r["kind"] == "kd" else fc.host_tree(r)
        self.cset = _capi.ConstraintSet(prim, self.kf, self.sk, self.al)
        self.handles = [_capi.Trajectory(prim, t["control_points"], granularity=t.get("granularity", 1000)) for t in self.trajs]
        flist = frame_constraints.TreeFrameList(prim, frames, self.sk, self.al) if with_frames and frames else None
        self.sset = TreeSearchSet(self.cset, [(h, t["min_u"], t["weight"]) for h, t in zip(self.handles, self.trajs)], self.al, flist)

    def triple(self):
        return (self.tree, self.prim, self.sset)

    def table(self):
        return self.tree.points if self.r["kind"] == "kd" else self.tree.means

    def errors(self, rows):
        return errors_of_samples(self.prim, self.cons, self.sk, self.al, np.ascontiguousarray(rows[:, :self.prim.n_components]))

    def descent(self, n):
        """(value, row, leaf, evaluations) of the host-driven descent: every level through candidate_scoring.errors_of_samples, as
        HipMotionStateGraphNode.search_best_sample_batched scores it"""
        table = self.table()
        score = lambda ids: self.errors(table[ids])
        if self.r["kind"] == "kd":
            return self.tree.descend_rows(score, n)
        value, _, leaf, n_eval = self.tree.descend(score, n)
        return value, int(self.tree.first_index[leaf]), leaf, n_eval

    def close(self):
        if self.sset.frame_constraints is not None:
            self.sset.frame_constraints.release()
        for h in self.handles + [self.cset, self.tree]:
            h.close()


def close_to(r, got, want):
    return abs(got - want) <= fc.tolerance(r, want)


@pytest.mark.parametrize("name", fc.ROW_IDS)
def test_every_row_is_the_batched_descent_and_the_oracles_value(ctx, prims, name):
    r = fc.BY_NAME[name]
    s = Search(prims(r["prim"]), r)
    try:
        want = fc.row_plan(r, s.cons)
        got = frames_search_plan([s.triple()], r["n_cand"])
        assert got == want, (name, got, want)
        rec = search_on_device([s.triple()], r["n_cand"])[0]
        value, row, leaf, n_eval = s.descent(r["n_cand"])
        sample = s.table()[row if r["kind"] == "kd" else leaf]
        again = s.errors(sample[None, :])[0]
        oracle_all = fc.oracle_values(r, s.cons, fc.host_tree(r).means)
        o_value, o_leaf, _, _ = fc.replay(fc.host_tree(r), oracle_all, r["n_cand"])
        print("%s: plan %d bytes (group %d, tables %s), slab %d bytes; leaf %d, value %.15g, descent %.15g, errors_of_samples %.15g, oracle %.15g (leaf %d)"
              % (name, got["lds_bytes"], got["track_group"], got["tables_lds"], got["scratch_bytes"], rec["leaf"], rec["value"], value, again, o_value, o_leaf))
        assert rec["flags"] == 0
        assert (rec["row"], rec["leaf"], rec["evaluations"]) == (row, leaf, n_eval), (name, rec, row, leaf, n_eval)
        assert close_to(r, rec["value"], value) and close_to(r, rec["value"], again), (name, rec["value"], value, again)
        if r["kind"] != "kd":
            assert rec["leaf"] == o_leaf
        assert close_to(r, rec["value"], o_value), (name, rec["value"], o_value)
    finally:
        s.close()


def test_one_launch_mixing_searches_with_and_without_lists_is_each_search_alone(ctx, prims):
    rows = [fc.BY_NAME[n] for n in ("flat65-local-short", "mixed_list", "flat3-ca-one_frame", "tables_memory")]
    searches = [Search(prims(r["prim"]), r, with_frames=(i != 1)) for i, r in enumerate(rows)]
    try:
        assert searches[1].sset.frame_constraints is None and searches[1].sset.trajectories
        together = search_on_device([s.triple() for s in searches], 2)
        for s, rec in zip(searches, together):
            alone = search_on_device([s.triple()], 2)[0]
            assert rec["flags"] == 0 and rec.tobytes() == alone.tobytes(), (s.r["name"], rec, alone)
    finally:
        for s in searches:
            s.close()


def test_a_shape_no_rung_takes_is_refused_and_the_python_route_falls_back(ctx):
    prim = _capi.Primitive(ctx, sc.refused_model())
    node = None
    try:
        L = prim.n_components
        means = np.concatenate([np.zeros((1, L)), np.random.default_rng(5).standard_normal((6, L))])
        from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree
        tree = HipFeatureClusterTree(means, means, [0, 6] + [6] * 6, np.arange(1, 7), [-1] + list(range(1, 7)), n_spatial=L)
        path = sc.mean_path("refused", sc.refused_model())
        kf = sc.keyframes(sc.REFUSED["n_keyframes"], 3, path)
        ca = {"type": "frame_ca_position", "joint": "Hips", "target": [float(path[5][0]) + 3.0, None, float(path[5][2])], "n_frames": 12, "weight": 1.0}
        sk = _capi.Skeleton(*sc.HIPS)
        flist = frame_constraints.TreeFrameList(prim, [ca], sk, None)
        cset = _capi.ConstraintSet(prim, kf, sk, None)
        sset = TreeSearchSet(cset, [], None, flist)
        try:
            assert frames_search_plan([(tree, prim, sset)], 2)["refused"]
            with pytest.raises(_capi.MGError) as e:
                search_on_device([(tree, prim, sset)], 2)
            assert e.value.status == _capi.MG_ERR_UNSUPPORTED
        finally:
            sset.release()
            cset.close()
        # the Python route: no search set, the batched descent
        node = object.__new__(HipMotionStateGraphNode)
        node.name, node.motion_primitive, node.cluster_tree = "refused", types.SimpleNamespace(_prim=prim, get_n_spatial_components=lambda: L), tree
        cons = types.SimpleNamespace(constraints=kf + [ca], hip_skeleton=sk, min_error=None, evaluations=0, is_local=True)
        assert node._tree_search_set(cons, per_frame=True) is None
        gen = types.SimpleNamespace(cluster_tree_search_method="descend", n_cluster_search_candidates=2, cluster_tree_search_per_frame=True)
        # (40 keyframes over 280 latents are beyond mg_score_constraints as well, so the descent itself is not run here: the route is
        # what is checked -- the generator asks for the set, gets None and calls the batched descent with its arguments)
        calls = []
        node.search_best_sample_batched = lambda c, n, prev=None, skel=None: (calls.append((c, n, skel)), (0.5, means[3]))[1]
        sample = HipMotionPrimitiveGenerator._get_best_fit_sample_using_cluster_tree(gen, node, cons, None)
        assert calls == [(cons, 2, sk)] and cons.min_error == 0.5 and np.array_equal(sample, means[3])
        tree.close()
    finally:
        candidate_scoring.clear_constraint_cache()
        prim.close()
