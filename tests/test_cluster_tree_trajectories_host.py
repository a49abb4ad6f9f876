"""Which constraint lists the one-launch cluster-tree search takes now that it scores root trajectory constraints
(HipMotionStateGraphNode._tree_search_set, the generator's routing), with the device calls stubbed: trajectory lists within
MG_TREE_MAX_TRAJECTORIES take the one launch; per-frame constraints, a fifth trajectory and an aligning node other than the root
keep the host-driven descent; the pinned device trajectories are handed back after the call and after an exception.  And the
stand-alone check of csrc/mg_tree_plan.h (the LDS plans, their ladder, the flattened trajectory lists)."""
import os
import subprocess
import types

import numpy as np
import pytest

from morphablegraphs_amd import _capi, candidate_scoring, motion_state_graph
from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree, TreeSearchSet
from morphablegraphs_amd.motion_primitive_generator import HipMotionPrimitiveGenerator
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraphNode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEYFRAME = {"type": "position", "t": 5.0, "weight": 1.0, "target": [1.0, None, 2.0]}


def _traj(i):
    return {"type": "trajectory", "control_points": [[0.0, 0.0, float(i)], [1.0, 0.0, float(i)], [2.0, 0.0, float(i)]], "min_u": 0.1 * i,
            "weight": 1.0 + i, "granularity": 1000}


class _Pins(object):
    """candidate_scoring's device objects, stubbed: every pin and release is counted"""

    def __init__(self, monkeypatch, fail_at=None):
        self.pinned, self.released, self.sets, self.fail_at = [], [], [], fail_at
        monkeypatch.setattr(candidate_scoring, "cached_constraint_set", self._cset)
        monkeypatch.setattr(candidate_scoring, "cached_trajectory", self._trajectory)
        monkeypatch.setattr(candidate_scoring, "release_trajectory", self.released.append)

    def _cset(self, prim, clist, skeleton=None, alignment=None):
        self.sets.append((list(clist), alignment))
        return "cset%d" % len(self.sets)

    def _trajectory(self, prim, c, pin=False):
        assert pin, "a handle kept beyond the call must be pinned"
        if self.fail_at is not None and len(self.pinned) == self.fail_at:
            raise RuntimeError("no device memory")
        t = types.SimpleNamespace(record=c)
        self.pinned.append(t)
        return t


@pytest.fixture
def node():
    n = object.__new__(HipMotionStateGraphNode)      # (no device: the node's constructor makes a context)
    n.name, n.motion_primitive = "stub", types.SimpleNamespace(_prim="prim")
    means = np.asarray([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    n.cluster_tree = HipFeatureClusterTree(means, means, [0, 2, 2, 2], [1, 2], [-1, 0, 1], n_spatial=2)
    return n


def _record(row=1, evaluations=2, flags=0):
    rec = np.zeros(1, dtype=_capi.TREE_SEARCH_RECORD)
    rec["row"], rec["leaf"], rec["evaluations"], rec["value"], rec["flags"] = row, row + 1, evaluations, 0.25, flags
    return rec


def test_lists_with_up_to_four_trajectories_make_a_search_set(node, monkeypatch):
    pins = _Pins(monkeypatch)
    for n_traj in range(0, _capi.MG_TREE_MAX_TRAJECTORIES + 1):
        cons = [KEYFRAME] + [_traj(i) for i in range(n_traj)]
        sset = node._tree_search_set(cons)
        assert isinstance(sset, TreeSearchSet) and sset.alignment is None
        assert pins.sets[-1][0] == [KEYFRAME]                       # the keyframe set holds no trajectory
        assert [(t.record, u, w) for t, u, w in sset.trajectories] == [(_traj(i), 0.1 * i, 1.0 + i) for i in range(n_traj)]
        before = len(pins.released)
        sset.release()
        sset.release()                                              # once
        assert len(pins.released) - before == n_traj and sset.trajectories == []
    assert len(pins.pinned) == len(pins.released) == 10


def test_what_the_launch_does_not_cover_keeps_the_batched_descent(node, monkeypatch):
    pins = _Pins(monkeypatch)
    five = [KEYFRAME] + [_traj(i) for i in range(_capi.MG_TREE_MAX_TRAJECTORIES + 1)]
    per_frame = [KEYFRAME, _traj(0), {"type": "frame_ca_position", "joint": "Hips", "target": [0.0, 0.0, 0.0], "n_frames": 12, "weight": 1.0}]
    assert node._tree_search_set(five) is None and node._tree_search_set(per_frame) is None
    monkeypatch.setattr(candidate_scoring, "alignment_from_prev_frames", lambda prev, constraints=None, skeleton=None: {"joint": 3, "position": (0, 0, 0), "heading": (1, 0)})
    assert node._tree_search_set([KEYFRAME, _traj(0)], prev_frames=np.zeros(7)) is None
    assert node._tree_search_set([KEYFRAME], prev_frames=np.zeros(7)) is not None           # (keyframe sets align to any joint)
    assert pins.pinned == []
    with pytest.raises(NotImplementedError):
        node.search_best_sample_on_device(five, 2)
    # the generator's routing
    gen = types.SimpleNamespace(cluster_tree_search_method="descend", n_cluster_search_candidates=2)
    calls = []
    monkeypatch.setattr(candidate_scoring, "alignment_from_prev_frames", lambda prev, constraints=None, skeleton=None: None)
    node.search_best_sample_batched = lambda c, n, prev=None, sk=None: (calls.append(("batched", n)), (0.5, np.zeros(2)))[1]
    monkeypatch.setattr(motion_state_graph, "search_on_device", lambda searches, n: (calls.append(("device", n, searches[0][2])), _record())[1])
    for cons, route in ((five, "batched"), (per_frame, "batched"), ([KEYFRAME, _traj(0), _traj(1)], "device"), ([_traj(2)], "device"), ([KEYFRAME], "device")):
        c = types.SimpleNamespace(constraints=cons, min_error=None, evaluations=0)
        HipMotionPrimitiveGenerator._get_best_fit_sample_using_cluster_tree(gen, node, c, None)
        assert calls[-1][0] == route and calls[-1][1] == 2
        if route == "device":
            assert c.evaluations == 2 and c.min_error == 0.25 and len(calls[-1][2].trajectories) == 0    # released by the search
    assert len(pins.pinned) == len(pins.released) == 3


def test_trajectories_are_released_after_the_call_and_after_an_exception(node, monkeypatch):
    pins = _Pins(monkeypatch)
    seen = []
    monkeypatch.setattr(motion_state_graph, "search_on_device", lambda searches, n: (seen.append(len(searches[0][2].trajectories)), _record())[1])
    err, sample = node.search_best_sample_on_device([KEYFRAME, _traj(0), _traj(1)], 2)
    assert seen == [2] and err == 0.25 and len(pins.pinned) == len(pins.released) == 2
    np.testing.assert_array_equal(sample, node.cluster_tree.data[1])

    def fails(searches, n):
        raise RuntimeError("launch failed")
    monkeypatch.setattr(motion_state_graph, "search_on_device", fails)
    with pytest.raises(RuntimeError):
        node.search_best_sample_on_device([_traj(0), _traj(1), _traj(2)], 1)
    assert len(pins.pinned) == len(pins.released) == 5
    # a tie in the record raises in result_of_record, after the release
    monkeypatch.setattr(motion_state_graph, "search_on_device", lambda searches, n: _record(flags=_capi.MG_TREE_TIE))
    with pytest.raises(TypeError):
        node.search_best_sample_on_device([_traj(0)], 1)
    assert len(pins.pinned) == len(pins.released) == 6
    # the second trajectory cannot be made: the first is handed back
    failing = _Pins(monkeypatch, fail_at=1)
    with pytest.raises(RuntimeError):
        node._tree_search_set([_traj(0), _traj(1)])
    assert len(failing.pinned) == len(failing.released) == 1


def test_tree_plan_header_alone():
    """csrc/mg_tree_plan.h states the search kernels' LDS plans, the ladder a plan beyond the workgroup's LDS is retried by and
    the flattening of the per-search trajectory lists without a HIP call; tests/native/tree_plan_check.cpp holds them to a
    restatement.  A program of its own (under the host sanitizers where the compiler has them): nothing is loaded into this
    process."""
    header = open(os.path.join(ROOT, "morphablegraphs_amd", "csrc", "mg_tree_plan.h")).read()
    assert "hip_runtime" not in header and "hipLaunch" not in header
    native = os.path.join(ROOT, "tests", "native")
    subprocess.check_call(["make", "-s", "-C", native, "-f", "tree_plan_check.mk", "tree_plan_check"])
    done = subprocess.run([os.path.join(native, "tree_plan_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert done.returncode == 0, done.stdout.decode("utf-8", "replace")
