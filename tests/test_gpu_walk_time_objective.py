"""A graph walk's time objective in one launch (mg_score_walk_time, HipWalkTimeObjective, obj_time_error_sum_one_launch) against
the step-by-step chain (obj_time_error_sum over HipTimeConstraints: mg_time_function_canonical and mg_gmm_log_prob per step, the
error on the host), bit for bit, and against the reference's own TimeConstraints (tests/golden/time_constraints.npz)."""
import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import objective_functions as of
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraphNode
from oracle import mg_oracle as orc

pytestmark = pytest.mark.gpu

# a: the common case; b: the smallest F the time model takes with its default n_basis_time; c: no time model (t(i) = i);
# d: another mixture width (KKg 10 where a has 4, b and c 2) and more canonical frames than one 64-frame chunk of the kernel
SHAPES = {"a": dict(n_time_components=3, n_frames=60, n_components=12, n_dim=11, n_gmm=5),
          "b": dict(n_time_components=1, n_frames=12, n_components=5, n_basis=7, n_dim=11, n_gmm=3),
          "c": dict(n_time_components=0, n_frames=20, n_components=7, n_dim=11, n_gmm=2),
          "d": dict(n_time_components=3, n_frames=150, n_components=30, n_dim=11, n_gmm=4),
          "e": dict(n_time_components=2, n_frames=16, n_components=6, n_basis=7, n_dim=11, n_gmm=2)}
STEEP = {"e": 25.0}      # harmonics of order 1 instead of a few percent: time latents of 800 overflow the exponential
FRAME_TIME = 0.02


class _Skeleton(object):
    def __init__(self, frame_time):
        self.aligning_root_node, self.aligning_root_dir, self.root, self.frame_time = "Hips", (0.0, 0.0, 1.0), "Hips", frame_time


class _Graph(object):
    def __init__(self, nodes, frame_time=FRAME_TIME):
        self.nodes, self.skeleton, self.hip_skeleton = nodes, _Skeleton(frame_time), None


class _Step(object):
    def __init__(self, key, parameters, n_spatial, n_time, cons=None):
        self.node_key, self.parameters, self.n_spatial_components, self.n_time_components = key, np.asarray(parameters, dtype=np.float64), n_spatial, n_time
        self.motion_primitive_constraints = cons


class _Action(object):
    def __init__(self, start_step, end_step):
        self.start_step, self.end_step = start_step, end_step


class _Walk(object):
    def __init__(self, steps):
        self.steps, self.elementary_action_list = steps, []

    def update_time_parameters(self, parameter_vector, start_step, end_step):
        offset = 0
        for step in self.steps[start_step:end_step]:
            step.parameters[step.n_spatial_components:] = parameter_vector[offset:offset + step.n_time_components]
            offset += step.n_time_components


class _World(object):
    def __init__(self):
        self.nodes, self.keys, self.datas, self.oracles = {}, {}, {}, {}
        for i, (name, kw) in enumerate(sorted(SHAPES.items())):
            data = synthetic.make_primitive(seed=300 + i, name=name, **kw)
            if name in STEEP:
                data["eigen_vectors_time"] = (STEEP[name] * np.asarray(data["eigen_vectors_time"])).tolist()
            node = HipMotionStateGraphNode()
            node.init_from_dict("walk", {"name": name, "mm": data})
            self.nodes[node.node_key], self.keys[name], self.datas[name] = node, node.node_key, data
            op = orc.OraclePrimitive(data)
            if kw["n_time_components"]:
                op.init_time_model(data)
            self.oracles[name] = op
        self.graph = _Graph(self.nodes)
        self.ctx = self.prim("a").ctx

    def prim(self, name):
        return self.nodes[self.keys[name]].motion_primitive._prim

    def walk(self, sequence, seed=0):
        rng = np.random.default_rng(seed)
        steps = []
        for name in sequence:
            L, Lt = SHAPES[name]["n_components"], SHAPES[name]["n_time_components"]
            steps.append(_Step(self.keys[name], 0.5 * rng.standard_normal(L + Lt), L, Lt))
        return _Walk(steps)

    def negative_t0_gamma(self, name):
        """Time latents whose canonical time function starts below 0 (the oracle says so): against the first time basis function's
        harmonics, the only ones that reach canonical frame 0."""
        e0 = np.asarray(self.datas[name]["eigen_vectors_time"], dtype=np.float64)[0]
        gamma = -8.0 * e0 / np.linalg.norm(e0)
        t0 = self.oracles[name].back_transform_gamma_to_canonical_time_function(gamma)[0]
        assert t0 < 0.0 and int(t0) + 1 == 1, t0
        return gamma

    def close(self):
        of.clear_walk_objectives()
        for node in self.nodes.values():
            node.motion_primitive._prim.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _case(world, sequence, start_step, n, seed=1):
    """walk, HipTimeConstraints over every branch of the error, S (n, the window's time latents) with a negative t(0) under a
    keyframe-0 constraint in row 0."""
    walk = world.walk(sequence, seed)
    window = sequence[start_step:]
    m = len(window)
    F = [SHAPES[k]["n_frames"] for k in window]
    timed = next(j for j, k in enumerate(window) if SHAPES[k]["n_time_components"])
    clist = [(0, F[0] - 1, 1.1), (timed, 0, 0.05), (0, -1, 1.3), (m - 1, 3, 2.0), (m - 1, 5, 2.5),        # both ends, from the end, two on one step
             (m + 2, 1, 1.0), (m, 0, 1.0), (0, F[0] + 3, 2.0), (m - 1, F[m - 1], 2.0),                     # beyond the window; at or past F
             (min(1, m - 1), -2, 3.0), (m - 1, -F[m - 1], 0.3)]
    tc = of.HipTimeConstraints(world.graph, walk, start_step, len(sequence), clist)
    rng = np.random.default_rng(100 * seed + n)
    widths = [SHAPES[k]["n_time_components"] for k in window]
    S = 0.5 * rng.standard_normal((n, sum(widths)))
    at = sum(widths[:timed])
    S[0, at:at + widths[timed]] = world.negative_t0_gamma(window[timed])
    return walk, tc, S


def _chain(world, walk, tc, S, error_scale=2.0, quality_scale=0.3):
    return (np.atleast_1d(of.obj_time_error_sum(S, (world.graph, walk, tc, error_scale, quality_scale))),
            np.atleast_1d(tc.evaluate_graph_walk(S, world.graph, walk)), np.atleast_1d(tc.get_average_loglikelihood(S, world.graph, walk)))


WINDOWS = [(("a",), 0), (("c", "a"), 1), (("a", "b"), 0), (("d", "b", "a"), 1), (("b", "c", "a"), 0), (("a", "c", "a", "d"), 1),
           (("a", "b", "c", "d", "a"), 0), (("b", "d", "c", "a", "b", "a"), 1)]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("sequence,start_step", WINDOWS)
def test_one_launch_is_bit_identical_to_the_chain(world, sequence, start_step, n):
    walk, tc, S = _case(world, sequence, start_step, n)
    want_obj, want_err, want_ll = _chain(world, walk, tc, S)
    objective = of.HipWalkTimeObjective(world.graph, walk, tc)
    try:
        obj, err, ll = objective.evaluate(S, 2.0, 0.3, parts=True)
        print("max |objective - chain| %.3e, |error - chain| %.3e, |log-likelihood - chain| %.3e" %
              (np.max(np.abs(obj - want_obj)), np.max(np.abs(err - want_err)), np.max(np.abs(ll - want_ll))))
        assert np.array_equal(ll, want_ll)
        assert np.array_equal(err, want_err)
        assert np.array_equal(obj, want_obj)
        assert np.array_equal(objective.evaluate(S, 2.0, 0.3), want_obj)
    finally:
        objective.close()
    data = (world.graph, walk, tc, 2.0, 0.3)
    assert np.array_equal(of.obj_time_error_sum_one_launch(S, data), want_obj)
    one = of.obj_time_error_sum_one_launch(S[n - 1], data)
    assert isinstance(one, float) and one == want_obj[n - 1]


def test_golden_cases_of_the_references_own_class():
    from conftest import golden_model, load_golden
    data, gm = golden_model("time_model")
    g = load_golden("time_constraints")
    n_s, n_t = int(gm["n_spatial_components"]), int(gm["n_time_components"])
    node = HipMotionStateGraphNode()
    node.init_from_dict("walk", {"name": "tm", "mm": data})
    walk = _Walk([_Step(node.node_key, b, n_s, n_t) for b in g["base"]])
    graph = _Graph({node.node_key: node}, float(g["frame_time"]))
    for ci in range(int(g["n_cases"])):
        clist = [(int(r[0]), int(r[1]), float(r[2])) for r in g["constraint_list_%d" % ci]]
        tc = of.HipTimeConstraints(graph, walk, int(g["start_step_%d" % ci]), int(g["end_step_%d" % ci]), clist)
        S, want_e, want_l = g["S_%d" % ci], g["error_%d" % ci], g["loglikelihood_%d" % ci]
        objective = of.HipWalkTimeObjective(graph, walk, tc)
        obj, err, ll = objective.evaluate(S, 2.0, 0.3, parts=True)
        np.testing.assert_allclose(err, want_e, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(ll, want_l, rtol=1e-9, atol=1e-8)
        np.testing.assert_allclose(obj, 2.0 * want_e - 0.3 * want_l, rtol=1e-9, atol=1e-8)
        np.testing.assert_array_equal(objective.evaluate(S, 2.0, 0.3), obj)
        objective.close()
    node.motion_primitive._prim.close()


def test_one_evaluate_is_one_launch_and_the_tables_travel_once(world):
    walk, tc, S = _case(world, ("a", "b", "c", "d"), 0, 17)
    objective = of.HipWalkTimeObjective(world.graph, walk, tc)
    ctx = world.ctx
    ctx.profile_enable(True)
    try:
        objective.evaluate(S, 2.0, 0.3)                      # (the context's table may still hold another window's)
        uploads = objective.table_uploads()
        ctx.profile_reset()
        objective.evaluate(S + 0.01, 2.0, 0.3, parts=True)
        assert ctx.profile_get("walk_time")[1] == 1 and ctx.profile_get(13)[1] == 1
        assert ctx.profile_get("gmm_log_prob")[1] == 0
        assert objective.table_uploads() == uploads and objective.n_launches == 2
        _chain(world, walk, tc, S)                           # the chain, for comparison: a mixture launch per step, none in the new slot
        assert ctx.profile_get("gmm_log_prob")[1] >= 4 and ctx.profile_get("walk_time")[1] == 1
    finally:
        ctx.profile_enable(False)
        objective.close()


def test_host_entry_point_equals_the_device_call(world):
    walk, tc, S = _case(world, ("d", "a", "b"), 0, 17)
    objective = of.HipWalkTimeObjective(world.graph, walk, tc)
    want = objective.evaluate(S, 2.0, 0.3, parts=True)
    got = objective.table.score(S, 2.0, 0.3)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert np.array_equal(objective.table.score(S, 2.0, 0.3, parts=False), want[0])
    objective.close()


def test_refusals_and_bad_arguments(world):
    walk, tc, S = _case(world, ("a", "b"), 0, 5)
    objective = of.HipWalkTimeObjective(world.graph, walk, tc)
    with pytest.raises(_capi.MGError) as e:
        objective.evaluate(S.astype(np.float32), 2.0, 0.3)
    assert e.value.status == _capi.MG_ERR_UNSUPPORTED == -4
    with pytest.raises(_capi.MGError) as e:                  # rows shorter than the window's time latents
        with world.ctx.buffers() as bufs:
            objective.table.score_dev(bufs.upload(S), np.float64, len(S), S.shape[1] - 1, 2.0, 0.3, bufs.malloc(8 * len(S)))
    assert e.value.status == _capi.MG_ERR_INVALID_ARGUMENT
    with pytest.raises(_capi.MGError) as e:
        objective.table.score(S[:, :-1], 2.0, 0.3)
    assert e.value.status == _capi.MG_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        objective.evaluate(S[:, :-1], 2.0, 0.3)
    empty = objective.evaluate(S[:0], 2.0, 0.3)
    assert empty.shape == (0,) and all(a.shape == (0,) for a in objective.evaluate(S[:0], 2.0, 0.3, parts=True))
    assert objective.table.score(S[:0], 2.0, 0.3, parts=False).shape == (0,)
    objective.close()
    # a keyframe below -F: IndexError, as indexing the time function would; the entry point itself answers invalid argument
    F = SHAPES["a"]["n_frames"]
    tc_bad = of.HipTimeConstraints(world.graph, walk, 0, 2, [(0, 3, 1.0), (0, -F - 1, 1.0)])
    with pytest.raises(IndexError):
        of.obj_time_error_sum_one_launch(S, (world.graph, walk, tc_bad, 2.0, 0.3))
    with pytest.raises(IndexError):
        of.obj_time_error_sum(S, (world.graph, walk, tc_bad, 2.0, 0.3))
    table = _capi.WalkTimeTable([(world.prim("a"), 0, walk.steps[0].parameters[:12])], [(0, -F - 1, 1.0)], 0.0, FRAME_TIME)
    with pytest.raises(_capi.MGError) as e:
        table.score(S[:, :3], 2.0, 0.3)
    assert e.value.status == _capi.MG_ERR_INVALID_ARGUMENT
    table.close()


def test_a_static_primitive_falls_back_to_the_chain(world):
    from morphablegraphs_amd.motion_primitive_wrapper import HipMotionPrimitiveModelWrapper, HipStaticMotionPrimitive

    class _StaticNode(HipMotionPrimitiveModelWrapper):
        """A node whose motion is constant (its time function is the identity over ITS canonical frames) beside a mixture."""

        def __init__(self, prim, n_canonical_frames):
            HipMotionPrimitiveModelWrapper.__init__(self)
            self.motion_primitive = HipStaticMotionPrimitive()
            self.motion_primitive.n_canonical_frames = n_canonical_frames
            self._prim = prim
    nodes = dict(world.nodes)
    nodes[("walk", "static")] = _StaticNode(world.prim("c"), 9)       # 9 canonical frames where the mixture's primitive has 20
    graph = _Graph(nodes)
    walk = world.walk(("a", "c", "b"), 3)
    walk.steps[1].node_key = ("walk", "static")
    tc = of.HipTimeConstraints(graph, walk, 0, 3, [(1, 8, 1.5), (1, 9, 1.0), (2, 4, 2.0), (0, -1, 1.0)])
    S = 0.4 * np.random.default_rng(9).standard_normal((7, 4))
    with pytest.raises(NotImplementedError):
        of.HipWalkTimeObjective(graph, walk, tc)
    data = (graph, walk, tc, 2.0, 0.3)
    assert np.array_equal(of.obj_time_error_sum_one_launch(S, data), of.obj_time_error_sum(S, data))


def test_a_non_finite_time_function_is_a_value_error_and_leaves_the_other_rows_alone(world):
    walk, tc, S = _case(world, ("e", "b"), 0, 6)
    S[4] = 800.0                                             # exp overflows: t = inf from some frame on (the oracle says so)
    with np.errstate(over="ignore"):
        assert not np.all(np.isfinite(world.oracles["e"].back_transform_gamma_to_canonical_time_function(S[4, :2])))
    data = (world.graph, walk, tc, 2.0, 0.3)
    with pytest.raises(ValueError, match="candidate 4"):
        of.obj_time_error_sum_one_launch(S, data)
    with pytest.raises(ValueError, match="candidate 0"):
        of.obj_time_error_sum_one_launch(S[4], data)
    objective = of.HipWalkTimeObjective(world.graph, walk, tc)
    obj, err, ll = objective.evaluate(S, 2.0, 0.3, parts=True)
    objective.close()
    assert np.isnan(obj[4]) and np.isnan(err[4])
    keep = np.arange(6) != 4
    want_obj, want_err, want_ll = _chain(world, walk, tc, S[keep])
    assert np.array_equal(obj[keep], want_obj) and np.array_equal(err[keep], want_err) and np.array_equal(ll[keep], want_ll)


def test_the_cache_follows_the_window_and_the_spatial_latents(world):
    walk, tc, S = _case(world, ("a", "b"), 0, 3)
    data = (world.graph, walk, tc, 2.0, 0.3)
    first = of.obj_time_error_sum_one_launch(S, data)
    cached = of._walk_time_objective(world.graph, walk, tc)
    assert of._walk_time_objective(world.graph, walk, tc) is cached and cached.n_launches == 1
    walk.steps[0].parameters[SHAPES["a"]["n_components"]:] += 0.1        # time latents: the optimiser's own variables
    assert of._walk_time_objective(world.graph, walk, tc) is cached
    walk.steps[0].parameters[0] += 0.25                                   # a spatial latent: the mixture's row changes
    second = of.obj_time_error_sum_one_launch(S, data)
    assert of._walk_time_objective(world.graph, walk, tc) is not cached and cached.table is None
    assert np.array_equal(second, of.obj_time_error_sum(S, data)) and not np.array_equal(second, first)
    of.clear_walk_objectives()
    assert not of._WALK_TIME_OBJECTIVES


def test_optimizer_takes_the_same_iterates_on_either_objective(world):
    from morphablegraphs_amd.graph_walk_optimizer import HipGraphWalkOptimizer
    from morphablegraphs_amd.motion_primitive_generator import HipNumericalMinimizer

    class _Constraint(object):
        def __init__(self, keyframe, desired_time):
            self.constraint_type, self.canonical_keyframe, self.desired_time = "keyframe_position", keyframe, desired_time

    class _MPConstraints(object):
        def __init__(self, constraints):
            self.constraints = constraints

    class _Stub(object):
        _objective_function = None
    settings = {"max_steps": 2, "position_weight": 1.0, "orientation_weight": 1.0, "error_scale_factor": 2.0, "quality_scale_factor": 0.3,
                "optimized_actions": 2, "method": "BFGS", "max_iterations": 6, "tolerance": 1e-9, "diff_eps": 1e-7, "verbose": False}
    config = {"global_spatial_optimization_mode": "all", "optimize_collision_avoidance_constraints_extra": False,
              "global_spatial_optimization_settings": settings, "global_time_optimization_settings": settings, "local_optimization_settings": settings}
    results = []
    for minimizers in ({}, {"time": HipNumericalMinimizer(settings, of.obj_time_error_sum)}):
        walk = world.walk(("a", "b", "a"), 11)
        walk.steps[0].motion_primitive_constraints = _MPConstraints([_Constraint(40, 1.4)])
        walk.steps[1].motion_primitive_constraints = _MPConstraints([])
        walk.steps[2].motion_primitive_constraints = _MPConstraints([_Constraint(59, 3.1)])
        walk.elementary_action_list = [_Action(0, 2)]
        before = [st.parameters.copy() for st in walk.steps]
        opt = HipGraphWalkOptimizer(world.graph, config, minimizers=dict(minimizers, **{"global": _Stub(), "collision_avoidance": _Stub()}))
        assert (opt.time_error_minimizer._objective_function is of.obj_time_error_sum_one_launch) == (not minimizers)
        assert opt.optimize_time_parameters_over_graph_walk(walk) is walk
        assert any(not np.array_equal(a, st.parameters) for a, st in zip(before, walk.steps))
        assert opt.time_error_minimizer.n_launches > 2
        results.append([st.parameters.copy() for st in walk.steps])
    for a, b in zip(*results):
        assert np.array_equal(a, b)
