"""The trajectory tree search (mg_cluster_tree_search_trajectories) across its LDS ladder and shape edges: the GPU half of
tests/tree_search_cases.py.  Every row of the table: the plan query of the actual call equals the row's claim (staging state, bytes,
opt-in); the record equals the host-driven descent through the library's own scorers bit for bit (where those take the shape); the
winner is the argmin of oracle.mg_oracle's objective over the leaves and its value lies within the bound
tests/test_gpu_trajectory_shapes.py holds the root-path scorer to.  Then: the same search on every rung gives the same bytes, mixed
launches equal each search alone, the level and candidate edges with trajectories, KD rows without a mean, the trajectory edges, the
refusal, and both orders of a small and a large plan on fresh contexts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tree_search_cases as sc
from morphablegraphs_amd import _capi, candidate_scoring, synthetic
from morphablegraphs_amd.candidate_scoring import alignment_from_start_pose
from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree, TreeSearchSet, search_on_device
from morphablegraphs_amd.kd_cluster_tree import HipClusterTree
from test_gpu_cluster_tree import _spanning_tree
from test_gpu_kd_cluster_tree import _kd_tree

pytestmark = pytest.mark.gpu
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tree_search_optin_child.py")
WORST = [0.0, ""]       # the worst |device - oracle| / bound over the table, and its row
RAN = set()             # (state, kind, search, over 64 KiB) the plan query proved


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def flat_tree(kind, leaves):
    """A root whose children are the rows of `leaves`, all leaves (node i + 1 is row i)"""
    n, L = leaves.shape
    means = np.concatenate([np.zeros((1, L)), leaves])
    counts = np.array([n] + [0] * n)
    if kind == "kd":
        return _kd_tree(counts, [0] + [1] * n, means, n_spatial=L)
    first = np.where(counts == 0, np.arange(n + 1), -1)
    return HipFeatureClusterTree(means, means, np.concatenate([[0], np.cumsum(counts)]), np.arange(1, n + 1), first, n_spatial=L)


def alignment(mode):
    if mode == 1:
        al = _capi.Skeleton(*sc.HIPS).alignment_to(sc.PREV7, 0)
        return {"joint": 0, "position": al["position"], "heading": al["heading"]}
    return alignment_from_start_pose(sc.START_POSE) if mode == 2 else None


class Search(object):
    """One search's device objects: the tree, the keyframe set, the trajectories"""

    def __init__(self, prim, kind, kf, trajs, leaves, align=0, tree=None):
        self.prim, self.kind, self.kf, self.trajs, self.al = prim, kind, kf, trajs, alignment(align)
        self.tree = flat_tree(kind, leaves) if tree is None else tree
        self.cset = _capi.ConstraintSet(prim, kf, None, self.al)
        self.handles = [_capi.Trajectory(prim, t["control_points"], granularity=t.get("granularity", 1000), spline_type=t.get("spline_type", 0)) for t in trajs]
        self.sset = TreeSearchSet(self.cset, [(h, t["min_u"], t["weight"]) for h, t in zip(self.handles, trajs)], self.al)

    def triple(self):
        return (self.tree, self.prim, self.sset)

    def plan(self, n, others=()):
        all_ = [self] + list(others)
        return _capi.cluster_tree_search_plan([s.prim for s in all_], [s.tree.device_tree(s.prim) for s in all_], [s.cset for s in all_], n,
                                              trajectories=[s.sset.trajectories for s in all_], alignments=[s.al for s in all_])

    def descent(self, n):
        """(value, row, leaf, evaluations) of the host-driven descent: every level through candidate_scoring.errors_of_samples"""
        L = self.prim.n_components
        table = self.tree.points if self.kind == "kd" else self.tree.means
        score = lambda ids: candidate_scoring.errors_of_samples(self.prim, self.kf + self.trajs, None, self.al, np.ascontiguousarray(table[ids, :L]))
        if self.kind == "kd":
            return self.tree.descend_rows(score, n)
        value, _, leaf, n_eval = self.tree.descend(score, n)
        return value, int(self.tree.first_index[leaf]), leaf, n_eval

    def close(self):
        for h in self.handles + [self.cset, self.tree]:
            h.close()


def assert_is_descent(s, rec, n, what=""):
    value, row, leaf, n_eval = s.descent(n)
    assert rec["flags"] == 0, what
    assert (rec["row"], rec["leaf"], rec["evaluations"]) == (row, leaf, n_eval), (what, rec, row, leaf, n_eval)
    assert _bits(rec["value"]) == _bits(value), (what, rec["value"], value)


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
            made[name] = _capi.Primitive(ctx, sc.model(name))
        return made[name]
    yield get
    candidate_scoring.clear_constraint_cache()
    for p in made.values():
        p.close()


def row_search(prims, r):
    data, kf, trajs, leaves = sc.row_inputs(r)
    return Search(prims(r["prim"]), r["kind"], kf, trajs, leaves, r["align"]), data


@pytest.mark.parametrize("name", sc.ROW_IDS)
def test_every_row_runs_on_its_rung_and_gives_the_descents_bits_and_the_oracles_winner(ctx, prims, name):
    r = sc.BY_NAME[name]
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, r["search"])
    s, data = row_search(prims, r)
    try:
        want = sc.row_plan(r)
        got = s.plan(r["n_cand"])
        assert got == {k: v for k, v in want.items() if k != "state"}, (name, got, want)
        assert (want["state"], want["lds_opt_in"]) == (r["state"], r["over64"])
        rec = search_on_device([s.triple()], r["n_cand"])[0]
        assert rec["flags"] == 0 and rec["evaluations"] == r["n_leaves"] + (r["n_cand"] if r["kind"] == "kd" else 0)
        if r["yardstick"] == "batched":
            assert_is_descent(s, rec, r["n_cand"], name)
        values, bounds = sc.oracle_objectives(data, s.kf, s.trajs, sc.row_inputs(r)[3], r["align"], r["search"])
        best = int(np.argmin(values))
        ratio = abs(rec["value"] - values[best]) / bounds[best]
        print("%s: plan %d bytes, %s; leaf %d, value %.12g, oracle %.12g, |difference| / bound %.3g" % (name, got["lds_bytes"], want["state"], rec["leaf"],
                                                                                                  rec["value"], values[best], ratio))
        if ratio > WORST[0]:
            WORST[:] = [ratio, name]
        assert rec["leaf"] == best + 1, (name, rec["leaf"], best + 1)
        assert ratio <= 1.0, (name, rec["value"], values[best], bounds[best])
        RAN.add((r["state"], r["kind"], r["search"], r["over64"]))
    finally:
        ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
        s.close()


def test_every_rung_ran_for_both_kinds_and_searches_on_both_sides_of_64_kib():
    """Runs behind the table: what the plan queries proved."""
    assert {x[:3] for x in RAN} == {(st, k, q) for st in sc.STATES for k in sc.KINDS for q in (0, 1)}
    assert {(x[0], x[3]) for x in RAN} == {(st, side) for st in sc.STATES for side in (False, True)}
    print("worst |device - oracle| / bound over the table: %.3g (%s)" % (WORST[0], WORST[1]))


@pytest.mark.parametrize("search", [0, 1])
@pytest.mark.parametrize("kind", sc.KINDS)
def test_one_search_gives_the_same_bytes_on_every_rung(ctx, prims, kind, search):
    """The same search alone (everything staged) and beside a second search that only pushes the call's maxima over the limit, so the
    first runs with W, then the polynomials, then the root rows read from memory: its record is the same bytes every time."""
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
    first = sc.BY_NAME["four_trajectories-%s-s%d" % (kind, search)]
    s, _ = row_search(prims, first)
    try:
        assert s.plan(2)["lds_bytes"] == sc.row_plan(first)["lds_bytes"] and sc.row_plan(first)["state"] == "all_staged"
        alone = search_on_device([s.triple()], 2)
        assert alone["flags"][0] == 0
        for family, state in (("w_leaves", "w_memory"), ("three_long", "polynomials_memory"), ("root_rows_leave", "root_rows_memory")):
            pr = sc.BY_NAME["%s-%s-s%d" % (family, kind, search)]
            p, _ = row_search(prims, pr)
            try:
                want = sc.plan_fit(kind, sc.call_shape([sc.row_shape(first), sc.row_shape(pr)]))
                assert want["state"] == state and s.plan(2, [p]) == {k: v for k, v in want.items() if k != "state"}, (family, want)
                both = search_on_device([s.triple(), p.triple()], 2)
                np.testing.assert_array_equal(both[:1].view(np.uint8), alone.view(np.uint8), err_msg="%s: %s" % (family, state))
                np.testing.assert_array_equal(both[1:].view(np.uint8), search_on_device([p.triple()], 2).view(np.uint8), err_msg=family)
            finally:
                p.close()
    finally:
        ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
        s.close()


def _mixed(prims, kind):
    """Four searches with 0, 4, 1 and 3 trajectories over primitives of different L and NB, and tables of different lengths"""
    out = []
    for i, (prim, n_kf, align, segs) in enumerate((("tiny", 2, 0, []), ("wide60", 3, 0, [5, 40, 1, 17]), ("basis31", 1, 1, [90]), ("tiny", 2, 2, [3, 64, 9]))):
        path = sc.mean_path(prim)
        trajs = [{"type": "trajectory", "control_points": sc.control_points(path, n, 40 + 5 * i + j).tolist(), "min_u": 0.05 * j, "weight": 0.5 + j,
                  "granularity": 1000} for j, n in enumerate(segs)]
        leaves = np.random.default_rng(600 + i).standard_normal((20 + 7 * i, sc.PRIMS[prim][0]))
        out.append(Search(prims(prim), kind, sc.keyframes(n_kf, 50 + i, path), trajs, leaves, align))
    return out


@pytest.mark.parametrize("search", [0, 1])
@pytest.mark.parametrize("kind", sc.KINDS)
def test_mixed_launches_equal_each_search_alone(ctx, prims, kind, search):
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
    ss = _mixed(prims, kind)
    try:
        for n in (1, 3):
            together = search_on_device([s.triple() for s in ss], n)
            assert np.all(together["flags"] == 0)
            for i, s in enumerate(ss):
                np.testing.assert_array_equal(together[i:i + 1].view(np.uint8), search_on_device([s.triple()], n).view(np.uint8), err_msg="search %d" % i)
                assert_is_descent(s, together[i], n, (kind, search, n, i))
            plain = _capi.search_cluster_trees([ss[0].prim], [ss[0].tree.device_tree(ss[0].prim)], [ss[0].cset], n)
            np.testing.assert_array_equal(together[:1].view(np.uint8), plain.view(np.uint8))
    finally:
        ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
        for s in ss:
            s.close()


def _edge_trajs(path, specs):
    """specs: (n_points, spline type, min_u, weight, granularity)"""
    return [{"type": "trajectory", "control_points": sc.control_points(path, n - 1, 70 + i).tolist(), "min_u": mu, "weight": w, "granularity": G,
             "spline_type": st} for i, (n, st, mu, w, G) in enumerate(specs)]


_PIN_KF = [{"type": "position", "t": 11.0, "weight": 1.0, "target": [40.0, None, -25.0]},
           {"type": "position", "t": 5.5, "weight": 0.5, "target": [10.0, 3.0, 20.0]}]


@pytest.mark.parametrize("search", [0, 1])
@pytest.mark.parametrize("shape", ["feature-64", "feature-65", "feature-spanning", "kd-64", "kd-65", "kd-32-descents", "kd-33-descents", "kd-33-deep", "n-64"])
def test_level_and_candidate_edges_with_trajectories(ctx, prims, shape, search):
    """The pins of the level loop (64 and 65 children, chunks 64 | 64 | 2 that span frontier nodes), of the KD groups (32 and 33
    descents per leaf) and n_candidates = 64 with four trajectories, against the host-driven descent."""
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
    prim = prims("tiny")
    path = sc.mean_path("tiny")
    trajs = _edge_trajs(path, [(6, 0, 0.0, 1.0, 1000), (5, 0, 0.1, 0.6, 1000)])
    kind, n = shape.split("-")[0], 3
    means = lambda k: np.random.default_rng(k).standard_normal((k + 1, 3))
    if shape in ("feature-64", "feature-65", "kd-64", "kd-65"):
        k = int(shape[-2:])
        tree = flat_tree(kind, means(k)[1:])
    elif shape == "feature-spanning":
        tree = _spanning_tree(lambda x: candidate_scoring.errors_of_samples(prim, _PIN_KF + trajs, None, None, np.ascontiguousarray(x)))
    elif shape.startswith("kd-3"):
        per, levels = (32, 0) if "32" in shape else (33, 2 if "deep" in shape else 0)
        tree, n = _kd_tree([0], [1], np.zeros((1, 3)), kd_per_leaf=per, kd_levels=levels, seed=per + levels), 2
    else:
        kind, n = "feature", 64
        trajs = _edge_trajs(path, [(6, 0, 0.0, 1.0, 1000), (5, 0, 0.1, 0.6, 1000), (9, 0, 0.0, 2.0, 1000), (4, 0, 0.3, 0.2, 1000)])
        counts = [70] + [3] * 70 + [0] * 210
        m = np.random.default_rng(64).standard_normal((len(counts), 3))
        first = np.where(np.asarray(counts) == 0, np.arange(len(counts)), -1)
        tree = HipFeatureClusterTree(m, m, np.concatenate([[0], np.cumsum(counts)]), np.arange(1, len(counts)), first, n_spatial=3)
    s = Search(prim, kind, _PIN_KF, trajs, None, 0, tree=tree)
    try:
        rec = search_on_device([s.triple()], n)[0]
        assert_is_descent(s, rec, n, (shape, search))
        if shape == "n-64":
            assert rec["evaluations"] == 70 + 64 * 3 and s.plan(64)["trajectory_slots"] == 4
    finally:
        ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
        s.close()


@pytest.mark.parametrize("search", [0, 1])
def test_kd_rows_without_a_mean_with_trajectories(ctx, prims, search):
    """A level chunk that holds an inner node whose children are KD trees: the reference raises AttributeError there, the launch flags
    MG_TREE_NO_MEAN -- with trajectories the lanes of such rows walk zeros (the monotone search) or nothing (the reference's)."""
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
    prim = prims("tiny")
    samples = np.random.default_rng(9).standard_normal((2000, 3))
    tree = HipClusterTree.from_reference(synthetic.make_kd_cluster_tree(samples, 4, 2, seed=0), 3)      # KD children below depth 2
    trajs = _edge_trajs(sc.mean_path("tiny"), [(6, 0, 0.0, 1.0, 1000), (5, 0, 0.1, 0.6, 1000)])
    s = Search(prim, "kd", _PIN_KF[:1], trajs, None, 0, tree=tree)
    try:
        for n in (1, 2, 4):
            rec = search_on_device([s.triple()], n)[0]
            assert rec["flags"] == _capi.MG_TREE_NO_MEAN and rec["row"] == -1
            with pytest.raises(AttributeError):
                tree.result_of_record(rec)
            with pytest.raises(AttributeError):
                s.descent(n)
    finally:
        ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
        s.close()


@pytest.mark.parametrize("search", [0, 1])
@pytest.mark.parametrize("kind", sc.KINDS)
def test_trajectory_edges(ctx, prims, kind, search):
    """The shortest spline of each type, min_u = 0 and 1, weights 0 and -1, granularities 2 and 257: the host-driven descent's bits; a
    zero weight gives the keyframe-only record."""
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
    prim = prims("tiny")
    path = sc.mean_path("tiny")
    leaves = np.random.default_rng(81).standard_normal((30, 3))
    lists = {"shortest": [(2, _capi.MG_SPLINE_CATMULL_ROM, 0.0, 1.0, 1000), (4, _capi.MG_SPLINE_BSPLINE, 0.0, 1.0, 1000),
                          (4, _capi.MG_SPLINE_FITTED_BSPLINE, 0.0, 0.7, 1000)],
             "bounds": [(6, 0, 0.0, 1.0, 1000), (6, 0, 1.0, 1.0, 1000)],
             "negative_weight": [(6, 0, 0.2, -1.0, 1000), (5, _capi.MG_SPLINE_BSPLINE, 0.0, 0.5, 1000)],
             "granularities": [(6, 0, 0.0, 1.0, 2), (7, _capi.MG_SPLINE_FITTED_BSPLINE, 0.1, 1.0, 257)],
             "zero_weight": [(6, 0, 0.0, 0.0, 1000)]}
    try:
        for name, specs in lists.items():
            s = Search(prim, kind, _PIN_KF, _edge_trajs(path, specs), leaves, 0)
            try:
                for n in (1, 3):
                    rec = search_on_device([s.triple()], n)
                    assert_is_descent(s, rec[0], n, (kind, search, name, n))
                    if name == "zero_weight":
                        plain = _capi.search_cluster_trees([prim], [s.tree.device_tree(prim)], [s.cset], n)
                        np.testing.assert_array_equal(rec.view(np.uint8), plain.view(np.uint8))
            finally:
                s.close()
    finally:
        ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_a_plan_that_fits_on_no_rung_is_refused_before_any_launch(ctx, prims, kind):
    R = sc.REFUSED
    prim = _capi.Primitive(ctx, sc.refused_model())
    data = sc.refused_model()
    path = sc.mean_path("refused", data)
    trajs = [{"type": "trajectory", "control_points": sc.control_points(path, 5, 19).tolist(), "min_u": 0.0, "weight": 1.0, "granularity": 1000}]
    s = Search(prim, kind, sc.keyframes(R["n_keyframes"], 19, path), trajs, np.random.default_rng(19).standard_normal((R["n_leaves"], R["L"])), 0)
    small, _ = row_search(prims, sc.BY_NAME["small-%s-s0" % kind])
    try:
        want = sc.plan_fit(kind, sc.refused_shape(kind))
        assert want["refused"] and s.plan(2) == {k: v for k, v in want.items() if k != "state"}
        ctx.profile_enable(True)
        ctx.profile_reset()
        with pytest.raises(_capi.MGError) as e:
            search_on_device([s.triple()], 2)
        assert e.value.status == _capi.MG_ERR_UNSUPPORTED and "beyond 160 KiB" in str(e.value)
        assert ctx.profile_get("cluster_tree_search")[1] == 0
        ctx.profile_enable(False)
        rec = search_on_device([small.triple()], 2)[0]
        assert_is_descent(small, rec, 2, "after the refusal")
    finally:
        ctx.profile_enable(False)
        small.close()
        s.close()
        prim.close()


@pytest.mark.parametrize("order", ["small-first", "large-first"])
@pytest.mark.parametrize("kind", sc.KINDS)
def test_a_small_and_a_large_plan_in_both_orders_on_a_fresh_context(ctx, prims, kind, order):
    """The large-LDS opt-in of the <true> kernels is made at the first plan beyond 64 KiB: a process that has launched neither runs
    a plan under 64 KiB and the largest plan of the table in the order given (tests/tree_search_optin_child.py) and prints the records,
    which are this process's."""
    done = subprocess.run([sys.executable, CHILD, kind, order], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = done.stdout.decode("utf-8", "replace")
    assert done.returncode == 0, out
    got = dict(line.split()[1:3] for line in out.splitlines() if line.startswith("record "))
    for family in ("small", "last_under_limit"):
        r = sc.BY_NAME["%s-%s-s0" % (family, kind)]
        s, _ = row_search(prims, r)
        try:
            rec = search_on_device([s.triple()], r["n_cand"])
            assert got[family] == rec.tobytes().hex(), (family, out)
        finally:
            s.close()
