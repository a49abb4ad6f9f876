"""The host logic of trajectory constraints inside the chained graph-walk objectives, on a stub primitive that records its calls
(no GPU): _global_blocks' column order, the error it reports against the sum of its columns, which scorer a step's trajectories
go to, the raise that stays, and HipGraphWalkObjective's pins on its trajectories."""
import numpy as np
import pytest

from morphablegraphs_amd import _capi
from morphablegraphs_amd import candidate_scoring
from morphablegraphs_amd import objective_functions as of

T = 6           # canonical samples of the stub primitive
REF_DIR = (0.0, 0.0, 1.0)


class _StubSet(object):
    def __init__(self, clist, alignment):
        self.clist, self.alignment, self.n, self.handle, self.cached_values, self.closed = list(clist), alignment, len(clist), 1, None, 0

    def close(self):
        self.closed += 1


class _StubTrajectory(object):
    def __init__(self, c):
        self.c, self.pins, self.evicted, self.closed, self.handle = c, 0, False, 0, 1

    def close(self):
        self.closed += 1
        self.handle = None


class _StubPrimitive(object):
    """Residual of keyframe k: 10 k + 1 + candidate / 100; exit columns: the step's number; a trajectory of tag g: residual columns
    g + frame, error g / 2 (so that error != sum of the columns)."""
    n_canonical_frames = T

    def __init__(self, name):
        self.name, self.calls, self.step = name, [], 0

    def _grid_size(self, grid):
        return T

    def _keyframes(self, cset, S, how, state=None):
        self.calls.append((how, [c["type"] for c in cset.clist], cset.alignment, None if state is None else state.copy()))
        out = np.empty((len(S), cset.n))
        for k, c in enumerate(cset.clist):
            out[:, k] = (10.0 * c["tag"] + 1.0 + np.arange(len(S)) / 100.0) if c["type"] == "position" else float(c["t"])
        return out

    def score_constraint_residuals(self, cset, S):
        return self._keyframes(cset, S, "plain")

    def score_constraint_residuals_chained(self, cset, S, state):
        return self._keyframes(cset, S, "chained", state)

    def score_trajectory(self, trajectory, S, min_u=0.0, weight=1.0, alignment=None, residuals=False, grid=None):
        self.calls.append(("trajectory", trajectory.c["tag"], alignment, None))
        g = float(trajectory.c["tag"])
        return np.full(len(S), g / 2.0), g + np.tile(np.arange(T, dtype=np.float64), (len(S), 1))

    def score_trajectory_chained(self, trajectory, S, align_cand, template, min_u=0.0, weight=1.0, residuals=False, grid=None):
        self.calls.append(("trajectory_chained", trajectory.c["tag"], template, np.array(align_cand)))
        g = float(trajectory.c["tag"])
        return np.full(len(S), g / 2.0), g + np.tile(np.arange(T, dtype=np.float64), (len(S), 1))


class _Skeleton(object):
    def __init__(self, node="root"):
        self.aligning_root_node, self.aligning_root_dir, self.root = node, REF_DIR, "root"


class _Constraints(object):
    def __init__(self, cons, is_local=False):
        self.constraints, self.is_local, self.hip_skeleton, self.skeleton, self.start_pose = cons, is_local, None, _Skeleton(), None


class _Step(object):
    def __init__(self, key, L, cons):
        self.node_key, self.parameters, self.n_spatial_components, self.motion_primitive_constraints = key, np.zeros(L), L, cons


class _Graph(object):
    def __init__(self, nodes, node="root", hip_skeleton=None):
        self.nodes, self.skeleton, self.hip_skeleton = nodes, _Skeleton(node), hip_skeleton


def _position(tag):
    return {"type": "position", "t": 3.0, "weight": 1.0, "target": [1.0, None, 2.0], "tag": tag}


def _trajectory(tag):
    return {"type": "trajectory", "control_points": [[0.0, 0.0, 0.0], [1.0, 0.0, 1.0]], "min_u": 0.0, "weight": 1.0, "tag": tag}


@pytest.fixture
def stubbed(monkeypatch):
    """of's device objects replaced by stubs; -> the list of trajectories handed out."""
    handed = []

    def cached_trajectory(prim, c, pin=False):
        for t in handed:
            if t.c is c and t.handle:
                break
        else:
            t = _StubTrajectory(c)
            handed.append(t)
        if pin:
            t.pins += 1
        return t
    monkeypatch.setattr(of, "_prim_of", lambda node: node)
    monkeypatch.setattr(of, "cached_constraint_set", lambda prim, clist, sk, alignment: _StubSet(clist, alignment))
    monkeypatch.setattr(of, "cached_trajectory", cached_trajectory)
    return handed


def _walk(local=(), first=True):
    prims = {"a": _StubPrimitive("a"), "b": _StubPrimitive("b")}
    lists = [[_position(0)] + ([_trajectory(100)] if first else []), [_trajectory(200), _position(1), _trajectory(300)], [_position(2), _trajectory(400)]]
    steps = [_Step(k, 4, _Constraints(lists[i], i in local)) for i, k in enumerate(("a", "b", "a"))]
    return _Graph(prims), steps, prims


PREV = np.array([[1.0, 2.0, 3.0, 1.0, 0.0, 0.0, 0.0]])


def test_column_order_and_the_error_beside_the_column_sum(stubbed):
    graph, steps, _ = _walk()
    n = 3
    states = []
    S, single, blocks, errors = of._global_blocks(np.zeros((n, 12)), graph, steps, PREV, "frames", states=states)
    assert not single and [b.shape for b in blocks] == [(n, 1 + T), (n, 1 + 2 * T), (n, 1 + T)]
    # the grouped keyframe columns first, then T columns per trajectory in list order -- whatever the order in the list
    np.testing.assert_array_equal(blocks[1][:, 0], 11.0 + np.arange(n) / 100.0)
    np.testing.assert_array_equal(blocks[1][0, 1:], np.concatenate([200.0 + np.arange(T), 300.0 + np.arange(T)]))
    np.testing.assert_array_equal(blocks[2][0, 1:], 400.0 + np.arange(T))
    # the error: keyframe columns' sum + each trajectory's own error (here tag / 2), not the sum of its T columns
    np.testing.assert_array_equal(errors[1], blocks[1][:, 0] + 100.0 + 150.0)
    assert (errors[1] != blocks[1].sum(axis=1)).all()
    total = of.obj_global_error_sum(np.zeros((n, 12)), (graph, steps, 1.0, 0.1, PREV))
    np.testing.assert_array_equal(total, errors[0] + errors[1] + errors[2])
    rv = of.obj_global_residual_vector(np.zeros((n, 12)), (graph, steps, 1.0, 0.1, PREV, 2.0))
    assert rv.shape == (n, (1 + T) + (1 + 2 * T) + (1 + T))      # blocks wider than the steps' 4 latents are not padded
    np.testing.assert_array_equal(rv[:, :1 + T], blocks[0] / 2.0)
    assert len(states) == 3 and all(st.shape == (n, 4) for st in states)
    assert isinstance(of.obj_global_error_sum(np.zeros(12), (graph, steps, 1.0, 0.1, PREV)), float)


def test_first_and_local_steps_take_the_single_record_scorer(stubbed):
    graph, steps, prims = _walk(local=(1,))
    states = []
    of._global_blocks(np.zeros((2, 12)), graph, steps, PREV, "frames", states=states)
    a, b = prims["a"].calls, prims["b"].calls
    # step 0 (primitive a): the walk's own record for the trajectory and for the keyframe set
    assert a[0][0] == "trajectory" and a[0][1] == 100 and a[0][2] is not None and a[0][2]["joint"] == 0
    assert a[1][0] == "plain" and a[1][2] == a[0][2]
    # step 1 (b, local): both trajectories through score_trajectory without a record, in list order; the exits chained
    assert [c[:3] for c in b[:2]] == [("trajectory", 200, None), ("trajectory", 300, None)]
    assert b[2][0] == "plain" and b[2][2] is None and b[3][0] == "chained"
    # step 2 (a again): chained, on the state step 1 handed on, with the keyframe set's template
    assert a[2][0] == "trajectory_chained" and a[2][1] == 400
    np.testing.assert_array_equal(a[2][3], states[1])
    assert a[3][0] == "chained" and a[3][2] == a[2][2] and a[2][2]["heading"] == (0.0, 1.0) and a[2][2]["joint"] == 0
    np.testing.assert_array_equal(a[3][3], states[1])
    # not local: step 1's trajectories are chained on step 0's state
    graph, steps, prims = _walk()
    states = []
    of._global_blocks(np.zeros((2, 12)), graph, steps, PREV, "frames", states=states)
    chained = [c for c in prims["b"].calls if c[0] == "trajectory_chained"]
    assert [c[1] for c in chained] == [200, 300] and all(np.array_equal(c[3], states[0]) for c in chained)
    # a local first step: no record at all
    graph, steps, prims = _walk(local=(0,))
    of._global_blocks(np.zeros((2, 12)), graph, steps, PREV, "frames")
    assert prims["a"].calls[0][:3] == ("trajectory", 100, None)


def test_a_non_root_aligning_node_with_a_trajectory_is_refused(stubbed):
    graph, steps, _ = _walk(first=False)
    graph = _Graph(graph.nodes, "Spine", hip_skeleton=object())
    with pytest.raises(NotImplementedError, match="trajectory constraints in global coordinates need the root joint as aligning node"):
        of._global_blocks(np.zeros((2, 12)), graph, steps, None, "frames")
    # ... and not where every step with a trajectory is local, or there is none
    for st in steps[1:]:
        st.motion_primitive_constraints.is_local = True
    of._global_blocks(np.zeros((2, 12)), graph, steps, None, "frames")
    # without a skeleton the existing raise comes first
    with pytest.raises(NotImplementedError, match="is not the root joint"):
        of._global_blocks(np.zeros((2, 12)), _Graph(graph.nodes, "Spine"), steps, None, "frames")


class _StubTable(object):
    def __init__(self, records):
        self.records, self.ctx = records, None


def test_pins_balance_over_rebuilds_and_close(stubbed, monkeypatch):
    monkeypatch.setattr(of._capi, "WalkScoreTable", _StubTable)

    def _set(self, prim, clist, sk, alignment, taken):
        cs = _StubSet(clist, alignment)
        self._shared.append((cs, None))
        return cs
    monkeypatch.setattr(of.HipGraphWalkObjective, "_set", _set)
    graph, steps, _ = _walk(local=(1,))
    obj = of.HipGraphWalkObjective(graph, steps, PREV, "frames")
    assert [t.c["tag"] for t in stubbed] == [100, 200, 300, 400] and [t.pins for t in stubbed] == [1, 1, 1, 1]
    # (trajectory, min_u, weight, step, column in the step's block, record, chained)
    assert [(t[0].c["tag"], t[3], t[4], t[6]) for t in obj._trajectories] == [(100, 0, 1, False), (200, 1, 1, False), (300, 1, 1 + T, False), (400, 2, 1, True)]
    assert obj._trajectories[0][5] is not None and obj._trajectories[1][5] is None and obj._trajectories[3][5]["heading"] == (0.0, 1.0)
    # a second objective on the same trajectories: a pin each
    other = of.HipGraphWalkObjective(graph, steps, PREV, "frames")
    assert [t.pins for t in stubbed] == [2, 2, 2, 2]
    # a shared set rewritten for another caller: _ensure rebuilds -- the pins are handed back and taken again
    obj._shared[0][0].cached_values = "other values"
    obj._ensure()
    assert [t.pins for t in stubbed] == [2, 2, 2, 2] and len(obj._trajectories) == 4
    # the cache lets go of one while it is pinned: closed by the last release
    stubbed[3].evicted = True
    other.close()
    assert [t.pins for t in stubbed] == [1, 1, 1, 1] and stubbed[3].closed == 0
    obj.close()
    assert [t.pins for t in stubbed] == [0, 0, 0, 0] and [t.closed for t in stubbed] == [0, 0, 0, 1]
    obj.close()      # twice is once
    assert [t.pins for t in stubbed] == [0, 0, 0, 0]
    # the raise that stays, before anything is left pinned
    graph2 = _Graph(graph.nodes, "Spine", hip_skeleton=object())
    for st in steps:
        st.motion_primitive_constraints.is_local = False
    with pytest.raises(NotImplementedError, match="trajectory constraints in global coordinates need the root joint as aligning node"):
        of.HipGraphWalkObjective(graph2, steps, None, "frames")
    import gc
    gc.collect()
    assert all(t.pins == 0 for t in stubbed)
