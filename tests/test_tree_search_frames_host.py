"""The one-launch tree search with per-frame constraint lists (mg_cluster_tree_search_frames), without a device: which lists take the
launch (HipMotionStateGraphNode._tree_search_set(per_frame=...), the generator's new algorithm_config key, the graph's
evaluate_options), with the device calls stubbed as tests/test_cluster_tree_trajectories_host.py stubs them; the restated plan of
tests/tree_search_frames_cases.py against csrc/mg_tree_plan.h through tests/native/tree_frames_plan_check; and the conditioning of every row
of the case table for the oracle."""
import os
import subprocess
import types

import numpy as np
import pytest

import tree_search_cases as sc
import tree_search_frames_cases as fc
from morphablegraphs_amd import _capi, candidate_scoring, cluster_tree, frame_constraints, motion_state_graph
from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree, TreeSearchSet
from morphablegraphs_amd.motion_primitive_generator import HipMotionPrimitiveGenerator
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraph, HipMotionStateGraphNode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")

KEYFRAME = {"type": "position", "t": 5.0, "weight": 1.0, "target": [1.0, None, 2.0]}
CA = {"type": "frame_ca_position", "joint": "Hips", "target": [0.0, 0.0, 0.0], "n_frames": 12, "weight": 1.0}
LOCAL = {"type": "frame_local_trajectory", "joint": "Hips", "control_points": [[0.0, 0.0, 0.0], [1.0, 0.0, 1.0], [2.0, 0.0, 1.0]], "granularity": 1000, "start_t": 0.0,
         "n_frames": 12, "weight": 1.0}


def _traj(i):
    return {"type": "trajectory", "control_points": [[0.0, 0.0, float(i)], [1.0, 0.0, float(i)], [2.0, 0.0, float(i)]], "min_u": 0.1 * i, "weight": 1.0 + i,
            "granularity": 1000}


class _Stubs(object):
    """candidate_scoring's and frame_constraints' device objects, stubbed: every pin, list and release is counted"""

    def __init__(self, monkeypatch, refused=False, uncovered=False, fail_list=False):
        self.pinned, self.released, self.lists, self.list_releases, self.plans = [], [], [], [], []
        monkeypatch.setattr(candidate_scoring, "cached_constraint_set", lambda prim, clist, skeleton=None, alignment=None: ("cset", list(clist)))
        monkeypatch.setattr(candidate_scoring, "cached_trajectory", self._trajectory)
        monkeypatch.setattr(candidate_scoring, "release_trajectory", self.released.append)
        monkeypatch.setattr(candidate_scoring, "alignment_from_prev_frames", lambda prev, constraints=None, skeleton=None: None)

        def tree_frame_list(prim, frames, skeleton, alignment):
            if fail_list:
                raise RuntimeError("no device memory")
            if uncovered:
                return None
            fl = types.SimpleNamespace(constraints=list(frames), release=lambda: self.list_releases.append(fl))
            self.lists.append(fl)
            return fl
        monkeypatch.setattr(frame_constraints, "tree_frame_list", tree_frame_list)
        monkeypatch.setattr(cluster_tree, "frames_search_plan", lambda searches, n: (self.plans.append(searches), {"refused": refused})[1])

    def _trajectory(self, prim, c, pin=False):
        assert pin
        t = types.SimpleNamespace(record=c)
        self.pinned.append(t)
        return t


@pytest.fixture
def node():
    n = object.__new__(HipMotionStateGraphNode)
    n.name, n.motion_primitive = "stub", types.SimpleNamespace(_prim="prim")
    means = np.asarray([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    n.cluster_tree = HipFeatureClusterTree(means, means, [0, 2, 2, 2], [1, 2], [-1, 0, 1], n_spatial=2)
    return n


def _record(row=1, evaluations=2):
    rec = np.zeros(1, dtype=_capi.TREE_SEARCH_RECORD)
    rec["row"], rec["leaf"], rec["evaluations"], rec["value"] = row, row + 1, evaluations, 0.25
    return rec


def test_per_frame_lists_make_a_search_set_only_when_asked(node, monkeypatch):
    stubs = _Stubs(monkeypatch)
    cons = [KEYFRAME, _traj(0), CA, LOCAL]
    assert node._tree_search_set(cons) is None and node._tree_search_set(cons, per_frame=False) is None        # the routing there always was
    assert stubs.pinned == [] and stubs.lists == []
    sset = node._tree_search_set(cons, per_frame=True)
    assert isinstance(sset, TreeSearchSet) and sset.cset == ("cset", [KEYFRAME]) and len(sset.trajectories) == 1
    assert sset.frame_constraints is stubs.lists[0] and sset.frame_constraints.constraints == [CA, LOCAL]       # the list, in list order
    assert len(stubs.plans) == 1 and stubs.plans[0][0][2] is sset                                              # the plan was asked
    sset.release()
    sset.release()                                                                                             # once
    assert len(stubs.released) == 1 and stubs.list_releases == [stubs.lists[0]] and sset.frame_constraints is None
    # a list without per-frame constraints is the set it always was, whatever the flag
    plain = node._tree_search_set([KEYFRAME, _traj(1)], per_frame=True)
    assert plain.frame_constraints is None and len(stubs.lists) == 1
    plain.release()


def test_what_the_frames_launch_still_refuses(node, monkeypatch):
    stubs = _Stubs(monkeypatch)
    assert node._tree_search_set([CA] * (_capi.MG_FRAME_LIST_MAX + 1), per_frame=True) is None                 # a list beyond the cap
    assert node._tree_search_set([CA] + [_traj(i) for i in range(_capi.MG_TREE_MAX_TRAJECTORIES + 1)], per_frame=True) is None
    assert stubs.pinned == [] and stubs.lists == []
    monkeypatch.setattr(candidate_scoring, "alignment_from_prev_frames", lambda prev, constraints=None, skeleton=None: {"joint": 3, "position": (0, 0, 0), "heading": (1, 0)})
    assert node._tree_search_set([_traj(0), CA], prev_frames=np.zeros(7), per_frame=True) is None              # trajectories aligned to another joint
    assert node._tree_search_set([KEYFRAME, CA], prev_frames=np.zeros(7), per_frame=True) is not None          # (tracks align through any joint)
    # a refused plan and an uncovered list: None, with everything handed back
    for kw in (dict(refused=True), dict(uncovered=True)):
        s = _Stubs(monkeypatch, **kw)
        assert node._tree_search_set([_traj(0), _traj(1), CA], per_frame=True) is None
        assert len(s.pinned) == len(s.released) == 2 and s.list_releases == s.lists
    s = _Stubs(monkeypatch, fail_list=True)
    with pytest.raises(RuntimeError):
        node._tree_search_set([_traj(0), CA], per_frame=True)
    assert len(s.pinned) == len(s.released) == 1


def test_the_generator_routes_by_the_new_key(node, monkeypatch):
    stubs = _Stubs(monkeypatch)
    calls = []
    node.search_best_sample_batched = lambda c, n, prev=None, sk=None: (calls.append(("batched", n)), (0.5, np.zeros(2)))[1]
    monkeypatch.setattr(motion_state_graph, "search_on_device", lambda searches, n: (calls.append(("device", n, searches[0][2].frame_constraints)), _record())[1])
    config = {"n_random_samples": 4, "local_optimization_settings": {"start_error_threshold": 1.0}, "constrained_sampling_mode": "cluster_tree_search",
              "cluster_tree_search_method": "descend"}
    gen = object.__new__(HipMotionPrimitiveGenerator)
    gen.set_algorithm_config(config)
    assert gen.cluster_tree_search_per_frame is False                                                          # off by default
    cons = types.SimpleNamespace(constraints=[KEYFRAME, CA], min_error=None, evaluations=0)
    gen._get_best_fit_sample_using_cluster_tree(node, cons, None)
    assert calls[-1] == ("batched", 2) and stubs.lists == []
    gen.set_algorithm_config(dict(config, cluster_tree_search_per_frame=True))
    gen._get_best_fit_sample_using_cluster_tree(node, cons, None)
    assert calls[-1][0] == "device" and calls[-1][2] is stubs.lists[0] and cons.evaluations == 2 and cons.min_error == 0.25
    assert stubs.list_releases == stubs.lists                                                                  # released by the search
    # the launch refuses: the batched descent
    _Stubs(monkeypatch, refused=True)
    gen._get_best_fit_sample_using_cluster_tree(node, cons, None)
    assert calls[-1] == ("batched", 2)
    # lists without per-frame constraints take the launch whatever the key says
    gen.set_algorithm_config(config)
    gen._get_best_fit_sample_using_cluster_tree(node, types.SimpleNamespace(constraints=[KEYFRAME], min_error=None, evaluations=0), None)
    assert calls[-1][0] == "device" and calls[-1][2] is None


def test_lists_and_trajectories_are_released_after_the_call_and_after_an_exception(node, monkeypatch):
    stubs = _Stubs(monkeypatch)
    monkeypatch.setattr(motion_state_graph, "search_on_device", lambda searches, n: _record())
    err, sample = node.search_best_sample_on_device([_traj(0), CA], 2, per_frame=True)
    assert err == 0.25 and len(stubs.pinned) == len(stubs.released) == 1 and stubs.list_releases == stubs.lists and len(stubs.lists) == 1
    with pytest.raises(NotImplementedError):
        node.search_best_sample_on_device([_traj(0), CA], 2)                                                   # not asked for: not covered

    def fails(searches, n):
        raise RuntimeError("launch failed")
    monkeypatch.setattr(motion_state_graph, "search_on_device", fails)
    with pytest.raises(RuntimeError):
        node.search_best_sample_on_device([_traj(0), _traj(1), LOCAL], 1, per_frame=True)
    assert len(stubs.pinned) == len(stubs.released) == 3 and stubs.list_releases == stubs.lists and len(stubs.lists) == 2


def test_evaluate_options_forwards_the_flag(node, monkeypatch):
    stubs = _Stubs(monkeypatch)
    graph = object.__new__(HipMotionStateGraph)
    graph.nodes = {"a": node}
    seen = []
    node.search_best_sample_batched = lambda c, n, prev=None, sk=None: (seen.append("batched"), (0.5, np.zeros(2)))[1]
    monkeypatch.setattr(motion_state_graph, "search_on_device", lambda searches, n: (seen.append(len(searches)), _record())[1])
    cons = {"a": types.SimpleNamespace(constraints=[KEYFRAME, CA], evaluations=0)}
    graph.evaluate_options(["a"], cons, 8, use_cluster_trees=True)
    assert seen == ["batched"] and stubs.lists == []
    best, results = graph.evaluate_options(["a"], cons, 8, use_cluster_trees=True, per_frame=True)
    assert seen == ["batched", 1] and best == "a" and results["a"][1] == 0.25 and cons["a"].evaluations == 2
    assert stubs.list_releases == stubs.lists and len(stubs.lists) == 1


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def _native(*args):
    subprocess.check_call(["make", "-s", "-C", NATIVE, "-f", "tree_frames_plan_check.mk", "tree_frames_plan_check"])
    done = subprocess.run([os.path.join(NATIVE, "tree_frames_plan_check")] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert done.returncode == 0, done.stdout.decode("utf-8", "replace")
    return done.stdout.decode()


def test_frames_plan_header_alone():
    """The per-frame part of csrc/mg_tree_plan.h is host code (no HIP call) and holds what tests/native/tree_frames_plan_check.cpp restates;
    a program of its own, nothing is loaded into this process."""
    header = open(os.path.join(ROOT, "morphablegraphs_amd", "csrc", "mg_tree_plan.h")).read()
    assert "hip_runtime" not in header and "hipLaunch" not in header and "mg_tree_frames_fit" in header
    assert "tree_frames_plan_check: ok" in _native()
    assert "int mg_cluster_tree_search_frames(" in open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert (_capi.MG_TREE_TRACK_GROUP, _capi.MG_FRAME_LIST_MAX) == (fc.TRACK_GROUP, fc.LIST_MAX)


def test_restated_frames_plan_is_the_headers():
    """frames_fit of tests/tree_search_frames_cases.py against mg_tree_frames_fit on the rows' shapes and on shapes around every further rung"""
    shapes = []
    for r in fc.ROWS + fc.SWEEP_ROWS:
        cons = fc.constraints_of(r)
        c = fc.call_of(r, len([k for k in cons if k["type"] == "position"]), [len(k["control_points"]) - 1 for k in cons if k["type"] == "trajectory"])
        shapes.append((r["kind"], c, fc.PRIMS[r["prim"]][1] * r["n_chan"], fc.table_bytes(r["tables"])))
    base = sc.call_shape([sc.search_shape("feature", "tiny", 2, 0, [5], 24, 2)])
    for kind in sc.KINDS:
        for ncp in (0, 49, 3400, 6000, 12000, 30000):
            for tables in (0, 8064, 60000, 150000):
                shapes.append((kind, base, ncp, tables))
        wide = sc.call_shape([sc.search_shape(kind, "wide60", 30, 0, [600], 24, 2)])
        shapes += [(kind, wide, 49, 8064), (kind, wide, 49, 60000), (kind, wide, 6000, 60000)]
    args = []
    for kind, c, ncp, tables in shapes:
        args += [sc.KINDS.index(kind), c["L"], c["nc"], c["n_cand"], c["children"], c["depth"], c["kd_children"], c["kd_depth"], c["traj"], c["wrows"],
                 c["cp_rows"], c["poly_doubles"], ncp, tables]
    lines = _native(*args).strip().splitlines()
    assert len(lines) == len(shapes)
    seen = set()
    for (kind, c, ncp, tables), line in zip(shapes, lines):
        p = fc.frames_fit(kind, c, ncp, tables)
        got = [int(v) for v in line.split()]
        assert got == [p["lds_bytes"], p["w_rows"], p["root_rows"], p["poly_doubles"], p["trajectory_slots"], p["track_group"], int(p["tables_lds"]), p["table_bytes"]], \
            (kind, c, ncp, tables, line, p)
        seen.add((p["track_group"], p["tables_lds"], p["refused"]))
    assert {(4, True, False), (4, False, False), (2, False, False), (1, False, False), (1, False, True), (0, False, False)} <= seen


def test_the_rows_stand_where_the_table_says():
    plans = {r["name"]: fc.row_plan(r) for r in fc.ROWS}
    assert all(not p["refused"] and p["track_group"] == fc.TRACK_GROUP for p in plans.values())
    assert not plans["tables_memory"]["tables_lds"] and fc.table_bytes(fc.BY_NAME["tables_memory"]["tables"]) == 0
    assert all(plans[n]["tables_lds"] for n in ("flat65-local-short", "two_level-n1-set", "list_at_cap", "mixed_list", "last_under_64k", "first_over_64k"))
    assert not plans["last_under_64k"]["lds_opt_in"] and plans["first_over_64k"]["lds_opt_in"]
    assert 0 < plans["first_over_64k"]["lds_bytes"] - plans["last_under_64k"]["lds_bytes"] <= 16
    assert {r["tree"][1] for r in fc.ROWS if r["tree"][0] == "flat"} >= {3, 64, 65}
    assert {r["n_cand"] for r in fc.ROWS if r["tree"][0] == "two_level"} == {1, 2} and {r["align"] for r in fc.ROWS} == {0, 1, 2}
    assert max(len([b for b in r["build"] if b.split(":")[0] not in ("keyframe", "trajectory")]) for r in fc.ROWS) == fc.LIST_MAX


@pytest.mark.parametrize("name", fc.ROW_IDS)
def test_every_row_is_conditioned_for_the_oracle(name):
    """At every level the kept and the dropped children, and the two best children, are more than 1000 tolerances apart by the
    oracle's objective: a device value within the tolerance descends the same way."""
    r = fc.BY_NAME[name]
    tree = fc.host_tree(r)
    values = fc.oracle_values(r, fc.constraints_of(r), tree.means)
    value, leaf, n_eval, gaps = fc.replay(tree, values, r["n_cand"])
    assert np.isfinite(value) and len(gaps) == (1 if r["tree"][0] == "flat" else 2)
    for level, kept_dropped, best_second, largest in gaps:
        need = 1000.0 * fc.tolerance(r, largest)
        print("%s level %d: kept-dropped %.3g, best-second %.3g, needed %.3g" % (name, level, kept_dropped, best_second, need))
        assert kept_dropped > need and best_second > need, (name, level, kept_dropped, best_second, need)


# ---- the sweep (fc.SWEEP_ROWS): where its rows stand, the ledger, the conditioning --------------------------------------------------------
def _family(name, kind=None):
    return [r for r in fc.SWEEP_ROWS if r["family"] == name and kind in (None, r["kind"])]


def test_the_sweeps_rows_stand_where_the_table_says():
    plans = {r["name"]: fc.row_plan(r) for r in fc.SWEEP_ROWS}
    assert len(set(plans)) == len(fc.SWEEP_ROWS) and not set(plans) & set(fc.ROW_IDS)
    for kind in sc.KINDS:
        one = lambda name: plans[_family(name, kind)[0]["name"]]
        stay, leave = one("tables_stay"), one("tables_leave")
        assert stay["tables_lds"] and stay["table_bytes"] == 144336 and stay["lds_opt_in"] and stay["track_group"] == 4
        assert not leave["tables_lds"] and leave["table_bytes"] == 0 and not leave["lds_opt_in"] and leave["track_group"] == 4
        assert fc.n_keyframes_of(_family("tables_leave", kind)[0]["build"]) == fc.n_keyframes_of(_family("tables_stay", kind)[0]["build"]) + 1
        # a staging rung moved by the lists' regions alone: the search without its list keeps what the search with it loses
        for name, key, keeps in (("lists_push_w", "w_rows", ("all_staged",)), ("lists_push_polynomials", "poly_doubles", ("all_staged", "w_memory")),
                                 ("lists_push_root_rows", "root_rows", ("all_staged", "w_memory", "polynomials_memory"))):
            r = _family(name, kind)[0]
            bare = sc.plan_fit(kind, fc.call_of(r, fc.n_keyframes_of(r["build"]), fc.segments_of(r["build"])))
            assert bare["state"] in keeps and bare[key] > 0 and one(name)[key] == 0 and one(name)["tables_lds"] and one(name)["track_group"] == 4, (name, kind, bare)
            assert one(name.replace("push", "keep"))[key] > 0
        assert one("lists_push_polynomials")["root_rows"] > 0 and len(fc.segments_of(_family("lists_push_root_rows", kind)[0]["build"])) == 2
        # every rung of the ladder, in one search
        r = _family("everything_left", kind)[0]
        c, p = fc.call_of(r, fc.n_keyframes_of(r["build"]), fc.segments_of(r["build"])), one("everything_left")
        assert c["wrows"] > 0 and c["poly_doubles"] > 0 and c["cp_rows"] > 0 and fc.table_bytes(r["tables"]) > 0
        assert (p["w_rows"], p["poly_doubles"], p["root_rows"], p["tables_lds"]) == (0, 0, 0, False) and p["track_group"] in (1, 2) and not p["refused"]
        assert set(fc.row_trace(r)) >= {"w", "poly", "cp", "tables", "group4"} and all(fc.row_trace(r)[k][1] for k in ("w", "poly", "cp", "tables", "group4"))
        # the groups, for the Hips skeleton (49 control points) and the chain (77)
        for fam, ncp in (("hips", 49), ("chain", 77)):
            got = {r["family"]: plans[r["name"]] for r in fc.SWEEP_ROWS if r["kind"] == kind and ("-%s-" % fam) in r["name"]}
            assert [got[n]["track_group"] for n in ("group4_last", "group2_first", "group1_first", "group1_last")] == [4, 2, 1, 1]
            assert all(p["control_points"] == ncp and not p["refused"] for n, p in got.items() if n != "refused_by_group")
        assert one("group2_65_children")["track_group"] == 2 and _family("group2_65_children", kind)[0]["tree"] == ("flat", 65)
        assert one("refused_by_group")["refused"] and _family("refused_by_group", kind)[0]["refused"]
        halved = [r for r in fc.SWEEP_ROWS if r["kind"] == kind and plans[r["name"]]["track_group"] in (1, 2)]
        assert {r["align"] for r in halved} >= {1, 2}
        assert any(r["tree"][1] % 2 for r in halved if plans[r["name"]]["track_group"] == 2)          # a count the group does not divide: a tail of one
    # the KD descents: one group of descents and one more, one and two levels, each on group 4 and on a halved group
    for fam, groups in (("kd_descents_group4", (4,)), ("kd_descents_halved", (1, 2))):
        rows = _family(fam)
        assert {r["kd"] for r in rows} == {(n, lv) for n in (1, 32, 33) for lv in (1, 2)} and all(plans[r["name"]]["track_group"] in groups for r in rows)
        assert all(len(r["build"]) == 2 and r["kind"] == "kd" for r in rows)
    assert max(r["kd"][0] for r in fc.SWEEP_ROWS) > sc.KD_GROUP
    # the yardstick: scorer_refuses on both sides of the VALU kernel's 150 KiB (64 rows of L + 1 latents and of max(n, 1) residuals), for
    # the wide primitives by the latent and for the tiny one by the keyframe; the GPU file asserts the refusal itself for every such row
    assert not fc.scorer_refuses(298, 1) and fc.scorer_refuses(299, 1) and not fc.scorer_refuses(3, 296) and fc.scorer_refuses(3, 297)
    assert not fc.scorer_refuses(296, 3) and fc.scorer_refuses(297, 3)
    for r in fc.SWEEP_ROWS:
        L, n = fc.PRIMS[r["prim"]][0], fc.n_keyframes_of(r["build"])
        assert (r["yardstick"] == "oracle") == ((64 * (L + 1) + max(n, 1) * 64) * 8 > 150 * 1024), r["name"]
    assert {r["yardstick"] for r in fc.SWEEP_ROWS} == {"oracle", "batched"}
    # a halved row's winner is decided by a score that only a group of that size forms: its place among the level's children -- for a
    # KD descent its start's place, or the pair of slots of the step that scored it -- lies in the second pair of a stride of four on
    # group 2, behind the first of four on group 1.  The record shows the winner alone, so this is where a wrong stride must show.
    halved = [r for r in fc.SWEEP_ROWS if not r["refused"] and plans[r["name"]]["track_group"] in (1, 2)]
    assert len(halved) == 22 and sum(plans[r["name"]]["track_group"] == 2 for r in halved) == 14
    for r in halved:
        assert fc.in_later_group(fc.oracle_of(r)["slot"], plans[r["name"]]["track_group"]), (r["name"], fc.oracle_of(r)["slot"], r["seed"])
    assert [fc.in_later_group(k, 2) for k in range(8)] == [False, False, True, True] * 2 and [fc.in_later_group(k, 1) for k in range(4)] == [False, True, True, True]


def _ledger_problems(rows):
    problems = []
    for e in fc.LEDGER:
        for side in ("below", "above"):
            listed = [r for r in rows if r["family"] in e[side]]
            for r in listed:
                got = fc.row_trace(r).get(e["comparison"])
                if got is None or got[1] != (side == "above"):
                    problems.append("%s: %s is not %s (%s)" % (e["boundary"], r["name"], side, got))
            for kind in sc.KINDS:
                if not any(r["kind"] == kind for r in listed):
                    problems.append("%s: nothing %s for %s" % (e["boundary"], side, kind))
    return problems


def test_the_ledger_lands_on_both_sides_of_every_comparison():
    rows = fc.ROWS + fc.SWEEP_ROWS
    assert _ledger_problems(rows) == []
    assert {e["comparison"] for e in fc.LEDGER} == {"64k", "w", "poly", "cp", "tables", "group4", "group2", "refused"}      # every comparison ladder_trace makes
    # ... and notices a side that goes missing
    for e in fc.LEDGER:
        for side in ("below", "above"):
            rest = [r for r in rows if r["family"] not in e[side]]
            assert any(p.startswith(e["boundary"]) and ("nothing %s" % side) in p for p in _ledger_problems(rest)), (e["boundary"], side)
    # the distance from the boundary: one step of what the shapes move the plan by there
    for e in fc.LEDGER:
        if e["step"] is None:
            continue
        limit = sc.LDS_MAX
        for kind in sc.KINDS:
            for side in ("below", "above"):
                bs = [fc.row_trace(r)[e["comparison"]][0] for r in rows if r["family"] in e[side] and r["kind"] == kind]
                assert min(abs(b - limit) for b in bs) <= e["step"], (e["boundary"], kind, side, bs)


def test_the_restated_kd_descent_is_the_trees_own():
    """kd_replay against HipClusterTree.descend_rows on seeded values: the same value, row, leaf and evaluation count"""
    for r in fc.SWEEP_ROWS:
        if r["kind"] != "kd" or r["refused"]:
            continue
        tree = fc.kd_tree(r)
        values = np.random.default_rng(len(r["name"])).uniform(1.0, 2.0, len(tree.points))
        value, row, leaf, n_eval, groups = fc.kd_replay(tree, values, r["n_cand"])
        assert (value, row, leaf, n_eval) == tuple(tree.descend_rows(lambda rows: values[rows], r["n_cand"])), r["name"]
        assert tree.kd_depth == r["kd"][1] and sum(len(g) == 2 for g in groups) >= r["kd"][0] * r["kd"][1]


@pytest.mark.parametrize("name", [r["name"] for r in fc.SWEEP_ROWS if not r["refused"]])
def test_every_sweep_row_is_conditioned_for_the_oracle(name):
    """Any two values the search compares among themselves -- a node's children, right against left at every KD step, a descent's heap,
    the descents of a leaf, the leaves' results -- are more than 1000 tolerances apart by the oracle's objective: a device value within
    the tolerance descends the same way.  (A refused row launches nothing: it has no descent to condition.)"""
    r = fc.BY_NAME[name]
    o = fc.oracle_of(r)
    assert np.isfinite(o["value"]) and np.all(np.isfinite(o["values"]))
    if o["groups"] is None:         # no KD descents: the levels' gaps, as test_every_row_is_conditioned_for_the_oracle takes them
        assert len(o["gaps"]) == 1
        for level, kept_dropped, best_second, largest in o["gaps"]:
            need = 1000.0 * fc.tolerance(r, largest)
            print("%s level %d: kept-dropped %.3g, best-second %.3g, needed %.3g" % (name, level, kept_dropped, best_second, need))
            assert kept_dropped > need and best_second > need, (name, level, kept_dropped, best_second, need)
        return
    gap, largest = fc.smallest_gap(o["groups"])
    need = 1000.0 * fc.tolerance(r, largest)
    print("%s: smallest gap %.3g over %d comparisons' values, needed %.3g; value %.15g at row %d" % (name, gap, len(o["groups"]), need, o["value"], o["row"]))
    assert gap > need, (name, gap, need)
