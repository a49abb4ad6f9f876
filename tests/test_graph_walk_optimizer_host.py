"""graph_walk_optimizer.py without a device: HipGraphWalkOptimizer's control flow (reference
motion_generator/graph_walk_optimizer.py:39-154) and TimeConstraintsBuilder (constraints/time_constraints_builder.py:27-63)
against stub graphs, walks and minimisers.  No objective is evaluated on a device here."""
import numpy as np
import pytest

from morphablegraphs_amd import graph_walk_optimizer as gwo
from morphablegraphs_amd import objective_functions as of


class _Constraint(object):
    def __init__(self, constraint_type, annotation=None, desired_time=None, canonical_keyframe=0):
        self.constraint_type, self.semantic_annotation = constraint_type, dict(annotation or {})
        self.weight_factor, self.desired_time, self.canonical_keyframe = 1.0, desired_time, canonical_keyframe


class _MPConstraints(object):
    def __init__(self, constraints):
        self.constraints = list(constraints)


class _Step(object):
    def __init__(self, constraints, n_spatial=2, n_time=1, start_frame=0):
        self.motion_primitive_constraints = None if constraints is None else _MPConstraints(constraints)
        self.parameters = np.arange(n_spatial + n_time, dtype=np.float64)
        self.n_spatial_components, self.n_time_components, self.start_frame, self.node_key = n_spatial, n_time, start_frame, ("a", "b")


class _Action(object):
    def __init__(self, start_step, end_step):
        self.start_step, self.end_step = start_step, end_step


class _Walk(object):
    def __init__(self, steps):
        self.steps, self.calls, self.elementary_action_list = steps, [], []

    def get_global_spatial_parameter_vector(self, start_step=0):
        out = []
        for st in self.steps[start_step:]:
            out += st.parameters[:st.n_spatial_components].tolist()
        return out

    def get_quat_frames(self):
        return np.zeros((100, 7))

    def update_spatial_parameters(self, x, start_step=0):
        self.calls.append(("update_spatial", np.asarray(x).copy(), start_step))

    def update_time_parameters(self, x, start_step, end_step):
        self.calls.append(("update_time", list(x), start_step, end_step))

    def convert_graph_walk_to_quaternion_frames(self, start_step=0, use_time_parameters=False):
        self.calls.append(("convert", start_step, use_time_parameters))


class _Minimizer(object):
    def __init__(self, objective=None, result=None):
        self._objective_function, self.result, self.data, self.runs, self.objective_calls = self._call, result, None, [], []
        self._objective = objective

    def _call(self, s, data):
        self.objective_calls.append((list(s), data))
        return self._objective(s, data)

    def set_objective_function_parameters(self, data):
        self.data = data

    def run(self, x0):
        self.runs.append((list(x0), self.data))
        return np.asarray(x0, dtype=np.float64) + 1.0 if self.result is None else self.result


class _ActionConstraints(object):
    contains_user_constraints, contains_two_hands_constraints, root_trajectory, collision_avoidance_constraints = True, False, None, None


def _config(mode="all", max_steps=2, optimized_actions=2):
    return {"global_spatial_optimization_mode": mode, "optimize_collision_avoidance_constraints_extra": False,
            "global_spatial_optimization_settings": {"max_steps": max_steps, "position_weight": 7.0, "orientation_weight": 3.0, "error_scale_factor": 0.8,
                                                     "quality_scale_factor": 0.05},
            "global_time_optimization_settings": {"optimized_actions": optimized_actions, "error_scale_factor": 2.0, "quality_scale_factor": 0.3}}


def _optimizer(mode="all", objective=None, **kw):
    mins = {"time": _Minimizer(), "global": _Minimizer(objective or (lambda s, data: np.array([-2.0, -1.5]))), "collision_avoidance": _Minimizer()}
    return gwo.HipGraphWalkOptimizer("graph", _config(mode, **kw), minimizers=mins), mins


def test_constants_are_the_references():
    assert gwo.CONSTRAINT_FILTER_LIST == ["keyframe_pose", "trajectory", "trajectory_set", "ca_constraint"]
    assert (gwo.GRAPH_WALK_OPTIMIZATION_ALL, gwo.GRAPH_WALK_OPTIMIZATION_TWO_HANDS, gwo.GRAPH_WALK_OPTIMIZATION_END_POINT) == ("all", "two_hands", "trajectory_end")


def test_filter_constraints_drops_exactly_the_four_filtered_types_and_counts_the_rest():
    opt, _ = _optimizer()
    kinds = ["keyframe_position", "keyframe_pose", "trajectory", "keyframe_2d_direction", "trajectory_set", "ca_constraint", "keyframe_two_hands",
             "keyframe_look_at", "keyframe_feet", "keyframe_relative_position"]
    walk = _Walk([_Step([_Constraint("keyframe_pose")]), _Step([_Constraint(k) for k in kinds]), _Step([_Constraint("keyframe_position"), _Constraint("trajectory")])])
    assert opt._filter_constraints(walk, 1) == 6 + 1
    assert [c.constraint_type for c in walk.steps[0].motion_primitive_constraints.constraints] == ["keyframe_pose"]      # before start_step: untouched
    assert [c.constraint_type for c in walk.steps[1].motion_primitive_constraints.constraints] == [k for k in kinds if k not in gwo.CONSTRAINT_FILTER_LIST]
    assert [c.constraint_type for c in walk.steps[2].motion_primitive_constraints.constraints] == ["keyframe_position"]


@pytest.mark.parametrize("mode", ["all", "two_hands"])
def test_adapt_constraint_weights_skips_generated_constraints(mode):
    opt, _ = _optimizer(mode)
    walk = _Walk([_Step([_Constraint("keyframe_position")]),
                  _Step([_Constraint("keyframe_position"), _Constraint("keyframe_2d_direction", {"generated": True})]),
                  _Step([_Constraint("keyframe_two_hands", {"keyframeLabel": "end"})])])
    opt._adapt_constraint_weights(walk, 1)
    weights = [[c.weight_factor for c in st.motion_primitive_constraints.constraints] for st in walk.steps]
    assert weights == [[1.0], [7.0, 1.0], [7.0]]


def test_adapt_constraint_weights_for_the_trajectory_end_touches_the_last_step_only():
    opt, _ = _optimizer("trajectory_end")
    last = [_Constraint("keyframe_position"), _Constraint("keyframe_2d_direction"), _Constraint("keyframe_two_hands")]
    walk = _Walk([_Step([_Constraint("keyframe_position"), _Constraint("keyframe_2d_direction")]), _Step(last)])
    opt._adapt_constraint_weights(walk, 0)
    assert [c.weight_factor for c in walk.steps[0].motion_primitive_constraints.constraints] == [1.0, 1.0]
    assert [c.weight_factor for c in last] == [7.0, 3.0, 1.0]


def test_optimize_picks_the_start_step_of_its_mode_and_does_nothing_without_a_reason(monkeypatch):
    walk = _Walk([_Step([_Constraint("keyframe_position")]) for _ in range(7)])
    state = _Action(5, 6)
    seen = []
    for mode, ac_kw, want in (("all", {}, [5 - 2]), ("two_hands", {"contains_two_hands_constraints": True}, [5 - 2]),
                              ("trajectory_end", {"root_trajectory": object()}, [7 - 2]),
                              ("all", {"contains_user_constraints": False}, []), ("two_hands", {}, []), ("trajectory_end", {}, []), ("none", {}, [])):
        opt, mins = _optimizer(mode)
        monkeypatch.setattr(opt, "optimize_spatial_parameters_over_graph_walk", lambda gw_, start_step=0: seen.append(start_step) or gw_)
        ac = _ActionConstraints()
        for k, v in ac_kw.items():
            setattr(ac, k, v)
        del seen[:]
        assert opt.optimize(walk, state, ac) is walk
        assert seen == want, (mode, ac_kw)
        assert not mins["global"].runs and not walk.calls
    opt, _ = _optimizer("all", max_steps=9)           # looking back further than the walk is long: from step 0
    monkeypatch.setattr(opt, "optimize_spatial_parameters_over_graph_walk", lambda gw_, start_step=0: seen.append(start_step) or gw_)
    del seen[:]
    opt.optimize(walk, state, _ActionConstraints())
    assert seen == [0]


def test_spatial_optimisation_makes_two_passes_for_init_error_sum():
    opt, mins = _optimizer("all", objective=lambda s, data: np.array([-2.0, -1.5, 0.25]))
    walk = _Walk([_Step([_Constraint("keyframe_position")], start_frame=0), _Step([_Constraint("keyframe_position")], start_frame=40),
                  _Step([_Constraint("keyframe_2d_direction"), _Constraint("trajectory")], start_frame=70)])
    assert opt.optimize_spatial_parameters_over_graph_walk(walk, 1) is walk
    g = mins["global"]
    x0 = [0.0, 1.0, 0.0, 1.0]
    assert len(g.objective_calls) == 1 and g.objective_calls[0][0] == x0
    first = g.objective_calls[0][1]
    assert first[0] == "graph" and first[1] == walk.steps[1:] and first[2:4] == (0.8, 0.05) and first[4].shape == (40, 7) and first[5] == 1.0
    assert len(g.runs) == 1 and g.runs[0][0] == x0
    assert g.runs[0][1][5] == 3.25 and g.runs[0][1][1] == walk.steps[1:]             # max(|sum|, 1)
    assert [c[0] for c in walk.calls] == ["update_spatial", "convert"]
    np.testing.assert_array_equal(walk.calls[0][1], np.array(x0) + 1.0)
    assert walk.calls[0][2] == 1 and walk.calls[1][1:] == (1, False)
    # |sum| below 1: init_error_sum is 1; start_step 0: no previous frames
    opt, mins = _optimizer("all", objective=lambda s, data: np.array([0.25, -0.5]))
    opt.optimize_spatial_parameters_over_graph_walk(walk, 0)
    assert mins["global"].runs[0][1][5] == 1.0 and mins["global"].runs[0][1][4] is None


def test_spatial_optimisation_without_constraints_left_does_not_call_the_minimiser():
    opt, mins = _optimizer("all")
    walk = _Walk([_Step([_Constraint("trajectory"), _Constraint("keyframe_pose")]), _Step([_Constraint("ca_constraint")])])
    assert opt.optimize_spatial_parameters_over_graph_walk(walk, 0) is walk
    assert not mins["global"].objective_calls and not mins["global"].runs and not walk.calls


def test_time_constraints_builder():
    steps = [_Step([_Constraint("keyframe_position", desired_time=1.0, canonical_keyframe=3)]),
             _Step([_Constraint("keyframe_position", desired_time=2.5, canonical_keyframe=11), _Constraint("keyframe_position", canonical_keyframe=4),
                    _Constraint("keyframe_2d_direction", desired_time=9.0, canonical_keyframe=5)]),
             _Step(None),
             _Step([_Constraint("keyframe_position", desired_time=4.0, canonical_keyframe=7)])]
    walk = _Walk(steps)
    b = gwo.TimeConstraintsBuilder(walk, 1, 2)
    assert (b.start_step, b.end_step) == (1, 3)                              # end_step + 1
    assert b.time_constraint_list == [(0, 11, 2.5)] and b.n_time_constraints == 1      # the step index counts from start_step
    b = gwo.TimeConstraintsBuilder(walk, 1, 9)
    assert b.end_step == 4                                                   # clipped to the walk
    assert b.time_constraint_list == [(0, 11, 2.5), (2, 7, 4.0)]
    assert gwo.TimeConstraintsBuilder(walk, 2, 2).build("graph", walk) is None


def test_time_constraints_builder_builds_hip_time_constraints(monkeypatch):
    made = []
    monkeypatch.setattr(of, "HipTimeConstraints", lambda *a: made.append(a) or "tc")
    walk = _Walk([_Step([_Constraint("keyframe_position", desired_time=1.0, canonical_keyframe=3)]), _Step([])])
    assert gwo.TimeConstraintsBuilder(walk, 0, 0).build("graph", walk) == "tc"
    assert made == [("graph", walk, 0, 1, [(0, 3, 1.0)])]


def test_time_optimisation_walks_the_actions_with_the_references_window(monkeypatch):
    class _TC(object):
        def __init__(self, graph, walk, start_step, end_step, constraint_list):
            self.args = (start_step, end_step, constraint_list)

        def get_initial_guess(self, walk):
            return [10.0 * self.args[0], float(self.args[1])]
    monkeypatch.setattr(of, "HipTimeConstraints", _TC)
    timed = lambda k: [_Constraint("keyframe_position", desired_time=1.0 + k, canonical_keyframe=k)]
    walk = _Walk([_Step(timed(0)), _Step([]), _Step(timed(2)), _Step([]), _Step([]), _Step(timed(5))])
    walk.elementary_action_list = [_Action(0, 1), _Action(2, 3), _Action(4, 4), _Action(5, 5)]
    opt, mins = _optimizer("all", optimized_actions=2)
    assert opt.optimize_time_parameters_over_graph_walk(walk) is walk
    # prev_action_idx = max(idx - 1, 0): windows (0, 1), (0, 3), (2, 4), (4, 5); all but none of them hold a timed constraint
    assert [c[2:] for c in walk.calls] == [(0, 1), (0, 3), (2, 4), (4, 5)]
    assert [c[0] for c in walk.calls] == ["update_time"] * 4
    runs = mins["time"].runs
    assert [r[0] for r in runs] == [[0.0, 2.0], [0.0, 4.0], [20.0, 5.0], [40.0, 6.0]]             # HipTimeConstraints got (start_step, min(end_step + 1, n))
    assert runs[1][1][0] == "graph" and runs[1][1][1] is walk and runs[1][1][3:] == (2.0, 0.3)
    assert runs[1][1][2].args[2] == [(0, 0, 1.0), (2, 2, 3.0)]
    assert walk.calls[1][1] == [1.0, 5.0]                                                          # what the minimiser returned
    # an action without timed constraints in its window is skipped
    walk2 = _Walk([_Step([]), _Step([])])
    walk2.elementary_action_list = [_Action(0, 1)]
    opt.optimize_time_parameters_over_graph_walk(walk2)
    assert not walk2.calls


def test_module_works_on_a_host_walk_without_a_device():
    from morphablegraphs_amd import graph_walk as gw, synthetic
    datas = [synthetic.make_primitive(seed=70 + i, n_components=L, n_frames=F, n_basis=NB, n_dim=11, n_gmm=2, name="w%d" % i)
             for i, (L, F, NB) in enumerate([(5, 12, 7), (3, 20, 6)])]

    class _Node(object):
        def __init__(self, data):
            self.motion_primitive = self
            m = gw._HostModel(data)
            self.s_pca = {"eigen_vectors": np.asarray(data["eigen_vectors_spatial"], dtype=np.float64).T, "mean_vector": np.asarray(data["mean_spatial_vector"]),
                          "n_basis": m.n_basis, "n_dim": m.n_dim, "knots": m.knots}
            self.n_canonical_frames, self.translation_maxima = m.n_canonical_frames, np.asarray(data.get("translation_maxima", (1.0, 1.0, 1.0)))
            self.has_time_parameters = False

        def get_n_spatial_components(self):
            return self.s_pca["eigen_vectors"].shape[1]

        def get_n_time_components(self):
            return 0

    class _Graph(object):
        nodes = {("walk", "w0"): _Node(datas[0]), ("walk", "w1"): _Node(datas[1])}
        skeleton = None
    graph = _Graph()
    walk = gw.HipGraphWalk(graph, host=True)
    rng = np.random.default_rng(3)
    for key in (("walk", "w0"), ("walk", "w1")):
        st = gw.HipGraphWalkStep.from_graph(graph, key, rng.standard_normal(graph.nodes[key].get_n_spatial_components()))
        st.motion_primitive_constraints = _MPConstraints([_Constraint("keyframe_position")])
        walk.steps.append(st)
    walk.convert_graph_walk_to_quaternion_frames()
    before = walk.get_quat_frames().copy()
    new = np.concatenate([st.parameters for st in walk.steps[1:]]) + 0.5
    mins = {"time": _Minimizer(), "global": _Minimizer(lambda s, data: np.array([4.0]), result=new), "collision_avoidance": _Minimizer()}
    opt = gwo.HipGraphWalkOptimizer(graph, _config("all"), minimizers=mins)
    opt.optimize_spatial_parameters_over_graph_walk(walk, 1)
    np.testing.assert_array_equal(walk.steps[1].parameters, new)
    after = walk.get_quat_frames()
    first = walk.steps[1].start_frame
    np.testing.assert_array_equal(after[:first], before[:first])                # the rows before the optimised step are untouched
    assert after.shape == before.shape and not np.array_equal(after[first:], before[first:])
    assert mins["global"].runs[0][1][4].shape == (first, 11) and mins["global"].runs[0][1][5] == 4.0
