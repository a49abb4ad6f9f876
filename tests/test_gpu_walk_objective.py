"""The objective of a whole graph walk in one launch (mg_score_walk_residuals, HipGraphWalkObjective, the *_one_launch
objectives) and HipGraphWalkOptimizer's global spatial optimisation.

Contract: the residuals are the bits of the step-by-step chain (objective_functions._global_blocks) -- both run
mg_constraint_residual on the same k-ordered chains and hand the exit state on as unrounded float64; no tolerance applies.
error_sum adds on the device one by one where NumPy's row sum is pairwise: rtol = atol = 1e-9, the bound
tests/test_gpu_objectives.py holds the chain to against the oracle, which is also the bound of the oracle comparison here
(1e-8 for the naturalness form)."""
import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import objective_functions as of
from morphablegraphs_amd.candidate_scoring import clear_constraint_cache
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraphNode
from oracle import mg_oracle as orc

pytestmark = pytest.mark.gpu

# (n_components, n_frames, n_basis): the packed matrix's k-steps are 2 (L = 3, 8: the smallest), 4 with an odd tail (9), 10 (40); L = 65 has none
SHAPES = {"a": (3, 12, 7), "b": (8, 20, 6), "c": (9, 17, 5), "d": (40, 33, 8), "e": (65, 25, 7)}
MAIN = ["d", "e", "b"]              # the step without packed matrix between two that have one
START_POSE = {"position": [35.0, 7.0, -12.0], "orientation": [0.0, 40.0, 0.0]}
BATCHES = [1, 15, 16, 17, 63, 64, 65, 257]          # the edges of the 16-candidate tile and the 64-candidate workgroup


class _Skeleton(object):
    def __init__(self, node):
        self.aligning_root_node, self.aligning_root_dir, self.root, self.frame_time = node, (0.0, 0.0, 1.0), "Hips", 1.0 / 30.0


class _Constraints(object):
    def __init__(self, cons, is_local, hip_sk, ref_sk, start_pose=None):
        self.constraints, self.is_local, self.hip_skeleton, self.skeleton = cons, is_local, hip_sk, ref_sk
        self.start_pose, self.min_error, self.evaluations = start_pose, None, 0


class _Step(object):
    def __init__(self, key, parameters, n_spatial, cons):
        self.node_key, self.parameters, self.n_spatial_components, self.n_time_components = key, np.asarray(parameters, dtype=np.float64), n_spatial, 0
        self.motion_primitive_constraints = cons


class _Graph(object):
    def __init__(self, nodes, ref_sk, hip_sk):
        self.nodes, self.skeleton, self.hip_skeleton = nodes, ref_sk, hip_sk


class _World(object):
    """The five primitives, made once for the module."""

    def __init__(self):
        self.joints, self.animated = synthetic.make_skeleton()
        self.hip_sk = _capi.Skeleton(self.joints, self.animated)
        self.nodes, self.ops, self.keys = {}, {}, {}
        for i, (name, (L, F, NB)) in enumerate(sorted(SHAPES.items())):
            data = synthetic.make_primitive(seed=60 + i, n_components=L, n_frames=F, n_basis=NB, n_gmm=2, name=name)
            node = HipMotionStateGraphNode()
            node.init_from_dict("walk", {"name": name, "mm": data})
            self.nodes[node.node_key], self.ops[name], self.keys[name] = node, orc.OraclePrimitive(data), node.node_key

    def constraints(self, name, i, variant=0):
        tl = float(SHAPES[name][1] - 1)
        s = 1.0 + 0.25 * variant
        return [{"type": "position", "t": tl, "weight": 1.0, "target": [30.0 * (i + 1) * s, None, -20.0 * i * s]},
                {"type": "direction", "t": tl / 2.0, "weight": 0.5 * s, "target": [0.3, 1.0]},
                {"type": "joint_position", "joint": "LeftHand", "t": tl, "weight": 2.0, "target": [25.0 * (i + 1), 95.0 * s, -15.0 * i]}]

    def walk(self, sequence, aligning_node="Hips", local=(), start_pose=None, empty=(), variants=None, seed=5):
        ref_sk = _Skeleton(aligning_node)
        rng = np.random.default_rng(seed)
        steps = []
        for i, name in enumerate(sequence):
            L = SHAPES[name][0]
            cons = [] if i in empty else self.constraints(name, i, 0 if variants is None else variants[i])
            steps.append(_Step(self.keys[name], rng.standard_normal(L), L, _Constraints(cons, i in local, self.hip_sk, ref_sk, start_pose if i == 0 else None)))
        return _Graph(self.nodes, ref_sk, self.hip_sk), steps

    def prev_frames(self):
        prev = self.ops["d"].back_project_frames(np.random.default_rng(9).standard_normal(SHAPES["d"][0]))[-3:].copy()
        prev[:, 0] += 120.0
        prev[:, 2] -= 40.0
        return prev

    def close(self):
        of.clear_walk_objectives()
        clear_constraint_cache()
        for node in self.nodes.values():
            node.motion_primitive._prim.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _latents(steps, n, seed=17, dtype=np.float64):
    return (0.7 * np.random.default_rng(seed).standard_normal((n, sum(st.n_spatial_components for st in steps)))).astype(dtype)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same_blocks(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape
        np.testing.assert_array_equal(_bits(g), _bits(w))


FIRST = {"prev_root": ("Hips", True, None), "prev_spine": ("Spine", True, None), "start_pose": ("Hips", False, START_POSE), "none": ("Hips", False, None)}


@pytest.mark.parametrize("exit_from", ["frames", "coeffs"])
@pytest.mark.parametrize("local_step", [None, 1])
@pytest.mark.parametrize("first", sorted(FIRST))
def test_one_launch_gives_the_bits_of_the_chain(world, first, local_step, exit_from):
    node, with_prev, start_pose = FIRST[first]
    graph, steps = world.walk(MAIN, node, () if local_step is None else (local_step,), start_pose)
    prev = world.prev_frames() if with_prev else None
    obj = of.HipGraphWalkObjective(graph, steps, prev, exit_from)
    for n in BATCHES:
        for dtype in (np.float64, np.float32):
            S = _latents(steps, n, seed=n, dtype=dtype)
            _assert_same_blocks(obj.blocks(S), of._global_blocks(S, graph, steps, prev, exit_from)[2])
    # the objectives on top of it, against their namesakes
    S = _latents(steps, 17)
    init = 3.5
    if exit_from == "frames":
        data = (graph, steps, 1.0, 0.1, prev)
        np.testing.assert_allclose(of.obj_global_error_sum_one_launch(S, data), of.obj_global_error_sum(S, data), rtol=1e-9, atol=1e-9)
        assert isinstance(of.obj_global_error_sum_one_launch(S[2], data), float)
        a, b = of.obj_global_residual_vector_one_launch(S, data + (init,)), of.obj_global_residual_vector(S, data + (init,))
    else:
        data = (graph, steps, 0.8, 0.05, prev, init)
        a, b = of.obj_global_residual_vector_and_naturalness_one_launch(S, data), of.obj_global_residual_vector_and_naturalness(S, data)
        one = of.obj_global_residual_vector_and_naturalness_one_launch(S[2], data)
        np.testing.assert_array_equal(_bits(one), _bits(b[2]))
    assert a.shape == b.shape == (17, sum(SHAPES[k][0] for k in MAIN))
    np.testing.assert_array_equal(_bits(a), _bits(b))
    before = [st.motion_primitive_constraints.evaluations for st in steps]
    obj.blocks(S)
    assert [st.motion_primitive_constraints.evaluations for st in steps] == [v + 17 for v in before]
    obj.close()


@pytest.mark.parametrize("aligning_node,local_step,with_prev", [("Hips", None, True), ("Spine", 1, True), ("Hips", None, False)])
def test_one_launch_against_the_oracle(world, aligning_node, local_step, with_prev):
    graph, steps = world.walk(MAIN, aligning_node, () if local_step is None else (local_step,))
    prev = world.prev_frames() if with_prev else None
    Ls = [st.n_spatial_components for st in steps]
    ops = [world.ops[k] for k in MAIN]
    cons = [st.motion_primitive_constraints.constraints for st in steps]
    S = _latents(steps, 4)

    def chain(row, exit_from):
        alphas = np.split(row, np.cumsum(Ls)[:-1])
        return orc.graph_walk_residual_blocks(ops, alphas, cons, None if prev is None else prev[-1], world.joints, world.animated, aligning_node,
                                              exit_from=exit_from, local_steps=() if local_step is None else (local_step,))
    init, error_scale, quality_scale = 3.5, 0.8, 0.05
    total = of.obj_global_error_sum_one_launch(S, (graph, steps, 1.0, 0.1, prev))
    rv = of.obj_global_residual_vector_one_launch(S, (graph, steps, 1.0, 0.1, prev, init))
    rn = of.obj_global_residual_vector_and_naturalness_one_launch(S, (graph, steps, error_scale, quality_scale, prev, init))
    for b, row in enumerate(S):
        blocks = chain(row, "frames")
        assert abs(total[b] - sum(blk.sum() for blk in blocks)) <= 1e-9 * max(1.0, abs(total[b]))
        cols = [np.concatenate([blk, np.zeros(L - len(blk))]) for blk, L in zip(blocks, Ls)]
        np.testing.assert_allclose(rv[b], np.concatenate(cols) / init, rtol=1e-9, atol=1e-9)
        cols, off = [], 0
        for blk, L, op in zip(chain(row, "coeffs"), Ls, ops):
            nll = -op.score_samples(row[off:off + L][None, :])[0] * quality_scale
            off += L
            cols.append(np.concatenate([blk * error_scale + nll, np.zeros(L - len(blk))]))
        np.testing.assert_allclose(rn[b], np.concatenate(cols) / init, rtol=1e-8, atol=1e-8)


def test_the_chain_is_real(world):
    """Step 0's latents reach the last step's columns through the state -- and do not where every later step is local."""
    Ls = [SHAPES[k][0] for k in MAIN]
    for local, moves in (((), True), ((1, 2), False)):
        graph, steps = world.walk(MAIN, "Hips", local)
        obj = of.HipGraphWalkObjective(graph, steps, world.prev_frames(), "frames")
        S = _latents(steps, 9)
        S2 = S.copy()
        S2[:, :Ls[0]] += 0.3
        a, b = obj.blocks(S), obj.blocks(S2)
        assert not np.array_equal(a[0], b[0])
        assert np.array_equal(_bits(a[2]), _bits(b[2])) == (not moves)
        assert np.array_equal(obj.exit_state(S), obj.exit_state(S2)) is False      # the exits themselves are always aligned
        obj.close()


def test_a_row_does_not_depend_on_its_batch(world):
    graph, steps = world.walk(MAIN, "Spine", (1,))
    obj = of.HipGraphWalkObjective(graph, steps, world.prev_frames(), "frames")
    S = _latents(steps, 257)
    row = S[200].copy()
    alone = np.hstack(obj.blocks(row[None, :]))
    S[0] = row
    full = np.hstack(obj.blocks(S))
    np.testing.assert_array_equal(_bits(full[0]), _bits(alone[0]))
    np.testing.assert_array_equal(_bits(full[200]), _bits(alone[0]))
    np.testing.assert_array_equal(_bits(np.hstack(obj.blocks(S))), _bits(full))      # two calls in a row repeat
    np.testing.assert_array_equal(_bits(obj.error_sum(S)[[0, 200]]), _bits(np.repeat(obj.error_sum(row[None, :]), 2)))
    obj.close()


def _chain_exit_state(monkeypatch, S, graph, steps, prev, exit_from):
    """The exit columns the chain's last step returns: the last residual matrix a primitive hands back, its last four columns."""
    seen = []
    for name in ("score_constraint_residuals", "score_constraint_residuals_chained"):
        real = getattr(_capi.Primitive, name)
        monkeypatch.setattr(_capi.Primitive, name, (lambda real: lambda self, *a: seen.append(real(self, *a)) or seen[-1])(real))
    blocks = of._global_blocks(S, graph, steps, prev, exit_from)[2]
    monkeypatch.undo()
    return blocks, seen[-1][:, -4:]


@pytest.mark.parametrize("sequence,kw", [(["c"], {}), (["a", "d"], {}), ((["a", "c", "b"] * 22)[:_capi.MG_WALK_MAX_STEPS], {}),
                                         (["b", "c", "b"], {"variants": [0, 0, 1]}),            # one primitive twice, other values in the same structure
                                         (["d", "a", "c"], {"empty": (1,)}),                   # a step with no constraints of its own: exits only
                                         (["d", "a", "c"], {"empty": (1,), "local": (1,)})])
def test_shapes_of_the_walk(world, monkeypatch, sequence, kw):
    graph, steps = world.walk(sequence, "Hips", **kw)
    prev = world.prev_frames()
    S = _latents(steps, 19)
    want, want_exit = _chain_exit_state(monkeypatch, S, graph, steps, prev, "frames")
    obj = of.HipGraphWalkObjective(graph, steps, prev, "frames")
    _assert_same_blocks(obj.blocks(S), want)
    np.testing.assert_array_equal(_bits(obj.exit_state(S)), _bits(want_exit))
    np.testing.assert_allclose(obj.error_sum(S), sum(b.sum(axis=1) for b in want), rtol=1e-9, atol=1e-9)
    obj.close()


def _sets(world, name, i, aligned=True, exits=True):
    """(primitive, scored set) as HipGraphWalkObjective builds them for a later, non-local step."""
    prim = of._prim_of(world.nodes[world.keys[name]])
    al = {"joint": 0, "position": (0.0, 0.0, 0.0), "heading": (0.0, 1.0), "ref_dir": (0.0, 0.0, 1.0)} if aligned else None
    clist = world.constraints(name, i) + (of._exit_constraints(float(prim.n_canonical_frames), 0, (0.0, 0.0, 1.0)) if exits else [])
    return prim, _capi.ConstraintSet(prim, clist, world.hip_sk, al)


def test_refusals_name_their_cause(world):
    pa, sa = _sets(world, "a", 0)
    pb, sb = _sets(world, "b", 1)
    pc, sc_unaligned = _sets(world, "c", 1, aligned=False)
    La, Lb, Lc = SHAPES["a"][0], SHAPES["b"][0], SHAPES["c"][0]
    S = np.zeros((5, La + Lb + Lc))

    def refused(records, needle, ld_res=6, S=S):
        with pytest.raises(_capi.MGError) as e:
            _capi.WalkScoreTable(records).score(S, ld_res)
        assert e.value.status == _capi.MG_ERR_INVALID_ARGUMENT and needle in str(e.value), str(e.value)
    good = [(pa, sa, None, 0, 3, 0), (pb, sb, None, La, 3, 3)]
    res, err, ex = _capi.WalkScoreTable(good).score(S, 6)
    assert np.isfinite(res).all() and np.isfinite(err).all() and np.isfinite(ex).all()
    refused([(pa, sa, None, 0, 3, 0)] * 65, "65 steps")
    refused([(pa, sa, None, 0, 3, 0), (pb, sa, None, La, 3, 3)], "another primitive")
    refused([(pa, sa, None, 0, 3, 0), (pb, sb, None, La, 3, 2)], "overlap")
    refused([(pa, sa, None, 0, 3, 0), (pb, sb, None, La, 3, 4)], "residual columns")                       # passes ld_res
    refused([(pa, sa, None, 0, 3, 0), (pc, sc_unaligned, None, La, 3, 3)], "previous-frame alignment")
    refused([(pa, sa, None, 0, 3, 0), (pb, sb, None, La + Lc + 1, 3, 3)], "latent columns")
    refused([(pa, sa, None, 0, 2, 0), (pb, sb, None, La, 3, 3)], "n_own")
    for cs in (sa, sb, sc_unaligned):
        cs.close()


def test_more_steps_than_one_launch_takes_fall_back_to_the_chain(world):
    graph, steps = world.walk((["a", "b"] * 33)[:65], "Hips")
    S = _latents(steps, 3)
    with pytest.raises(ValueError):
        of.HipGraphWalkObjective(graph, steps, None, "frames")
    data = (graph, steps, 1.0, 0.1, None, 2.0)
    np.testing.assert_array_equal(_bits(of.obj_global_residual_vector_one_launch(S, data)), _bits(of.obj_global_residual_vector(S, data)))
    np.testing.assert_array_equal(_bits(of.obj_global_error_sum_one_launch(S, data[:5])), _bits(of.obj_global_error_sum(S, data[:5])))


def test_through_the_minimiser(world):
    """HipLeastSquares on the one-launch objective walks the chain's path: the same vector, the same evaluation count."""
    from morphablegraphs_amd.motion_primitive_generator import HipLeastSquares
    graph, steps = world.walk(["a", "c", "b"], "Hips")
    prev = world.prev_frames()
    x0 = np.concatenate([st.parameters for st in steps])
    settings = {"max_iterations": 3 * (len(x0) + 2), "verbose": False}       # about three Jacobians of len(x0) evaluations each
    data = (graph, steps, 0.8, 0.05, prev, 2.0)
    out = []
    for objective in (of.obj_global_residual_vector_and_naturalness_one_launch, of.obj_global_residual_vector_and_naturalness):
        m = HipLeastSquares(settings, objective)
        m.set_objective_function_parameters(data)
        out.append((m.run(x0), m.n_equivalent_evaluations))
    assert out[0][1] == out[1][1] and out[0][1] > 2 * len(x0)
    np.testing.assert_array_equal(_bits(out[0][0]), _bits(out[1][0]))
    assert not np.array_equal(out[0][0], x0)


class _C(dict):
    """A device-form constraint that also answers the attributes the optimiser's filter and weights read."""

    def __init__(self, constraint_type, **kw):
        dict.__init__(self, **kw)
        self.constraint_type, self.semantic_annotation, self.weight_factor = constraint_type, {}, 1.0


@pytest.mark.parametrize("start_step", [0, 1])
def test_optimizer_end_to_end(world, start_step):
    from morphablegraphs_amd import graph_walk as gw
    from morphablegraphs_amd.graph_walk_optimizer import HipGraphWalkOptimizer
    sequence = ["a", "c", "b"]
    graph, _ = world.walk(sequence, "Hips")
    rng = np.random.default_rng(23)

    def make_walk(parameters):
        walk = gw.HipGraphWalk(graph)
        for i, (name, p) in enumerate(zip(sequence, parameters)):
            st = gw.HipGraphWalkStep.from_graph(graph, world.keys[name], p)
            kinds = ["keyframe_position", "keyframe_2d_direction", "keyframe_relative_position"]
            cons = [_C(k, **c) for k, c in zip(kinds, world.constraints(name, i))] + [_C("trajectory", type="trajectory")]      # (filtered out)
            st.motion_primitive_constraints = _Constraints(cons, False, world.hip_sk, graph.skeleton)
            walk.steps.append(st)
        walk.convert_graph_walk_to_quaternion_frames()
        return walk
    start = [0.7 * rng.standard_normal(SHAPES[k][0]) for k in sequence]
    walk = make_walk(start)
    before = walk.get_quat_frames().copy()
    row0 = walk.steps[start_step].start_frame
    settings = {"max_steps": 2, "position_weight": 1.0, "orientation_weight": 1.0, "error_scale_factor": 0.8, "quality_scale_factor": 0.05,
                "max_iterations": 70, "verbose": False, "method": "leastsq"}
    config = {"global_spatial_optimization_mode": "all", "optimize_collision_avoidance_constraints_extra": False,
              "global_spatial_optimization_settings": settings, "local_optimization_settings": dict(settings),
              "global_time_optimization_settings": dict(settings, optimized_actions=2, method="BFGS")}
    opt = HipGraphWalkOptimizer(graph, config)
    assert opt.optimize_spatial_parameters_over_graph_walk(walk, start_step) is walk
    assert all(len(st.motion_primitive_constraints.constraints) == 3 for st in walk.steps[start_step:])
    new = [st.parameters.copy() for st in walk.steps]
    for i, (a, b) in enumerate(zip(start, new)):
        assert np.array_equal(a, b) == (i < start_step)
    prev = None if start_step == 0 else before[:row0]
    data = (graph, walk.steps[start_step:], 0.8, 0.05, prev, 1.0)
    f0 = of.obj_global_residual_vector_and_naturalness(np.concatenate(start[start_step:]), data)
    f1 = of.obj_global_residual_vector_and_naturalness(np.concatenate(new[start_step:]), data)
    assert np.dot(f1, f1) <= np.dot(f0, f0)
    after = walk.get_quat_frames()
    np.testing.assert_array_equal(_bits(after[:row0]), _bits(before[:row0]))
    fresh = make_walk(start)                 # the same rows before row0, then the new parameters converted afresh
    for st, p in zip(fresh.steps, new):
        st.parameters = p.copy()
    fresh.convert_graph_walk_to_quaternion_frames(start_step)
    np.testing.assert_array_equal(_bits(after[row0:]), _bits(fresh.get_quat_frames()[row0:]))
    assert not np.array_equal(after[row0:], before[row0:])
    assert walk.get_num_of_frames() == fresh.get_num_of_frames()
    walk.close()
    fresh.close()
