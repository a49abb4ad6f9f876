"""Root trajectory constraints inside the chained graph-walk objectives (obj_global_error_sum, obj_global_residual_vector,
obj_global_residual_vector_and_naturalness, their *_one_launch forms and HipGraphWalkObjective), and the per-step exit values of
mg_score_walk_residuals_steps.

A three-step walk over two root-only primitives, n in {1, 17, 64}; trajectories on steps 2 and 3 (on step 1 too in one case),
a keyframe position constraint in every step, one case with an is_local step.

THE REFERENCE of the chain's values is made candidate by candidate from the single-record pieces: per candidate and step, the
exit values the keyframe route carries (the walk without its trajectories) become an ordinary alignment record, and the
step's constraints are scored with it as the per-primitive objectives do (score_constraint_residuals on a set aligned by that
record, score_trajectory with that record).  The first step and local steps share one record (or none): the same bits.  On a
chained step the single-record path divides the heading by its length on the host, the chained path uses the four values as
they are; where that division leaves a candidate's heading unchanged the comparison is exact, elsewhere the bound is

    TOL = weight * (2^-49 * R_STEP + 32 * 2^-53 * R_WORLD)

-- the heading's two components each move by at most 4 * 2^-53 relative (the square root, the division, and |h| - 1 of the device's
own normalisation), so the cosine and sine of the aligning rotation move by at most 2^-50 each and a root position at most
R_STEP = 64 from its step's first moves by at most 2^-49 * R_STEP; a distance to the target spline moves by no more than its
point does.  From there on every operation of the search rounds differently: about 32 operations on coordinates below
R_WORLD = 512, half an ulp each.  Both magnitudes are asserted on the walk's own paths.  (Measured maxima are in DESIGN 4.20.)

The one-launch forms are held to the chain bit for bit (error_sum to rtol = atol = 1e-9: the device adds one by one, NumPy
pairwise, as tests/test_gpu_walk_objective.py states)."""
import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import objective_functions as of
from morphablegraphs_amd.candidate_scoring import (alignment_from_prev_frames, cached_trajectory, clear_constraint_cache, group_residuals,
                                                   split_trajectories)

pytestmark = pytest.mark.gpu

SHAPES = {"a": (5, 20, 7), "b": (8, 18, 6)}      # n_components, n_frames, n_basis; root only: 3 + 4 channels
SEQUENCE = ["a", "b", "a"]
BATCHES = [1, 17, 64]
R_STEP, R_WORLD = 64.0, 512.0
REF_DIR = (0.0, 0.0, 1.0)
WORST = {"exact": 0, "bounded": 0, "diff": 0.0}


def _tol(weight):
    return weight * (2.0 ** -49 * R_STEP + 32.0 * 2.0 ** -53 * R_WORLD)


class _Skeleton(object):
    aligning_root_node, aligning_root_dir, root, frame_time = "root", REF_DIR, "root", 1.0 / 30.0


class _Constraints(object):
    def __init__(self, cons, is_local):
        self.constraints, self.is_local, self.hip_skeleton, self.skeleton = cons, is_local, None, _Skeleton()
        self.start_pose, self.min_error, self.evaluations = None, None, 0


class _Step(object):
    def __init__(self, key, parameters, cons):
        self.node_key, self.parameters, self.n_spatial_components, self.n_time_components = key, np.asarray(parameters, dtype=np.float64), len(parameters), 0
        self.motion_primitive_constraints = cons


class _Graph(object):
    def __init__(self, nodes):
        self.nodes, self.skeleton, self.hip_skeleton = nodes, _Skeleton(), None


def _model(name):
    """A root-only primitive: the root walks about 40 units forward along z with a gentle bend, varied by the latents."""
    L, F, NB = SHAPES[name]
    data = synthetic.make_primitive(seed=70 + L, name=name, n_components=L, n_frames=F, n_basis=NB, n_dim=7, n_gmm=2)
    mean = np.array(data["mean_spatial_vector"]).reshape(NB, 7)
    eig = np.array(data["eigen_vectors_spatial"]).reshape(L, NB, 7)
    t = np.linspace(0.0, 1.0, NB)
    mean[:, :3] = np.stack([6.0 * np.sin(2.0 * t), 90.0 + 0.0 * t, 40.0 * t], axis=-1)
    eig[:, :, :3] *= 0.03
    data["mean_spatial_vector"] = mean.reshape(-1).tolist()
    data["eigen_vectors_spatial"] = eig.reshape(L, -1).tolist()
    return data


def _path(k, wiggle):
    """A target path ahead of the walk's start (PREV): about 40 units per step along the previous heading."""
    t = np.linspace(0.0, 1.0, 7)
    return np.stack([20.0 + 150.0 * t * 0.6 + wiggle * np.sin(5.0 * t + k), 90.0 + 0.0 * t, -10.0 + 150.0 * t * 0.8 + wiggle * np.cos(3.0 * t + k)], axis=-1).tolist()


def _trajectory(k, weight=1.0, min_u=0.0, spline_type=0):
    c = {"type": "trajectory", "control_points": _path(k, 3.0 + k), "min_u": min_u, "weight": weight, "granularity": 1000}
    if spline_type:
        c["spline_type"] = spline_type
    return c


def _position(i, weight=1.0):
    return {"type": "position", "t": 10.0 + i, "weight": weight, "target": [40.0 + 20.0 * i, None, 20.0 + 30.0 * i]}


PREV = np.array([[18.0, 90.0, -14.0, 0.95, 0.0, 0.31, 0.0], [20.0, 90.0, -10.0, 0.94, 0.0, 0.34, 0.0]])
CASES = {
    # step -> constraint list; local steps
    "later_steps": ([[_position(0)], [_position(1, 0.5), _trajectory(1, 1.5)], [_trajectory(2, 1.0, 0.1), _position(2)]], ()),
    "first_step_too": ([[_position(0), _trajectory(0, 2.0)], [_trajectory(1, 1.5), _position(1), _trajectory(3, 0.5, 0.0, 1)], [_position(2), _trajectory(2, 1.0, 0.0, 2)]], ()),
    "local_step": ([[_position(0)], [_position(1), _trajectory(1, 1.5)], [_position(2), _trajectory(2)]], (1,)),
}


class _World(object):
    def __init__(self):
        self.ctx = _capi.Context(0)
        self.prims = {name: _capi.Primitive(self.ctx, _model(name)) for name in SHAPES}

    def walk(self, case, strip=False):
        lists, local = CASES[case]
        rng = np.random.default_rng(5)
        steps = []
        for i, name in enumerate(SEQUENCE):
            cons = [c for c in lists[i] if not (strip and c["type"] == "trajectory")]
            steps.append(_Step(name, rng.standard_normal(SHAPES[name][0]), _Constraints(cons, i in local)))
        return _Graph(self.prims), steps

    def close(self):
        of.clear_walk_objectives()
        clear_constraint_cache()
        for p in self.prims.values():
            p.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _latents(n, dtype=np.float64):
    return (0.7 * np.random.default_rng(100 + n).standard_normal((n, sum(SHAPES[k][0] for k in SEQUENCE)))).astype(dtype)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_blocks(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape
        np.testing.assert_array_equal(_bits(g), _bits(w))


def _survives(h):
    """The host's normalisation (mg_traj_fill_args: h / sqrt(h[0] * h[0] + h[1] * h[1])) leaves this heading as it is."""
    hn = np.sqrt(h[0] * h[0] + h[1] * h[1])
    return h[0] / hn == h[0] and h[1] / hn == h[1]


def _reference(world, case, S, exit_from):
    """Per step (blocks (n, columns), errors (n,), exact (n,) bool) from single-record launches, candidate by candidate."""
    graph, steps = world.walk(case)
    states = []
    of._global_blocks(S, *world.walk(case, strip=True), PREV, exit_from, states=states)      # the keyframe route's exit values
    al0 = alignment_from_prev_frames(PREV, type("_C", (), {"is_local": False, "skeleton": _Skeleton(), "start_pose": None})(), None)
    out, offset = [], 0
    for i, step in enumerate(steps):
        prim = graph.nodes[step.node_key]
        Li = step.n_spatial_components
        keyframes, trajectories = split_trajectories(step.motion_primitive_constraints.constraints)
        local = step.motion_primitive_constraints.is_local
        blocks, errors, exact = [], [], []
        for b in range(len(S)):
            alpha = np.ascontiguousarray(S[b:b + 1, offset:offset + Li])
            if local:
                record, same = None, True
            elif i == 0:
                record, same = al0, True
            else:
                hx, hz, px, pz = states[i - 1][b]
                record, same = {"joint": 0, "position": (px, 0.0, pz), "heading": (hx, hz), "ref_dir": REF_DIR}, _survives((hx, hz))
            cs = _capi.ConstraintSet(prim, keyframes, None, record)
            block = [group_residuals(keyframes, prim.score_constraint_residuals(cs, alpha))]
            cs.close()
            err = block[0].sum(axis=1)
            for c in trajectories:
                e, r = prim.score_trajectory(cached_trajectory(prim, c), alpha, c["min_u"], c["weight"], record, residuals=True)
                block.append(r)
                err = err + e
            blocks.append(np.hstack(block))
            errors.append(err)
            exact.append(same)
        out.append((np.vstack(blocks), np.concatenate(errors), np.array(exact)))
        offset += Li
    return out


def _column_weights(lists_i):
    keyframes, trajectories = split_trajectories(lists_i)
    return [c["weight"] for c in keyframes], [c["weight"] for c in trajectories]


def _column_bounds(kw, tw, T):
    return np.concatenate([[_tol(w) for w in kw]] + [np.full(T, _tol(w)) for w in tw])


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_chained_objectives_against_single_record_launches(world, case, n):
    graph, steps = world.walk(case)
    S = _latents(n)
    # the magnitudes the bound is derived from, on this walk's own candidates
    for name, prim in world.prims.items():
        root = prim.back_project_frames_f64(S[:, :SHAPES[name][0]] if name == "a" else S[:, SHAPES["a"][0]:SHAPES["a"][0] + SHAPES["b"][0]])[:, :, :3]
        assert np.abs(root - root[:, :1]).max() < R_STEP
    states = []
    _, _, blocks, errors = of._global_blocks(S, graph, steps, PREV, "frames", states=states)
    assert all(np.abs(st[:, 2:]).max() < R_WORLD - R_STEP for st in states)
    ref = _reference(world, case, S, "frames")
    total = np.zeros(n)
    for i, ((want_b, want_e, exact), got_b, got_e) in enumerate(zip(ref, blocks, errors)):
        assert got_b.shape == want_b.shape and got_e.shape == (n,)
        kw, tw = _column_weights(CASES[case][0][i])
        T = world.prims[SEQUENCE[i]]._grid_size(None)
        assert got_b.shape[1] == len(kw) + T * len(tw)
        col_tol = _column_bounds(kw, tw, T)
        same = exact
        np.testing.assert_array_equal(_bits(got_b[same]), _bits(want_b[same]), err_msg="step %d" % i)
        np.testing.assert_array_equal(_bits(got_e[same]), _bits(want_e[same]), err_msg="step %d" % i)
        diff = np.abs(got_b[~same] - want_b[~same])
        WORST["exact"] += int(same.sum())
        WORST["bounded"] += int((~same).sum())
        if diff.size:
            WORST["diff"] = max(WORST["diff"], float(diff.max()))
            print("step %d: %d candidates exact, %d bounded, max |difference| %.3e (bound %.3e)" % (i, same.sum(), (~same).sum(), diff.max(), col_tol.min()))
            assert (diff <= col_tol[None, :]).all(), (case, n, i, float(diff.max()))
            assert (np.abs(got_e[~same] - want_e[~same]) <= sum(_tol(w) for w in kw + tw)).all()
        # the error is the keyframe columns' sum and the trajectories' weighted AVERAGE distance, not the sum of their T columns
        want_sum = got_b[:, :len(kw)].sum(axis=1)
        for k in range(len(tw)):
            want_sum = want_sum + got_b[:, len(kw) + k * T:len(kw) + (k + 1) * T].mean(axis=1)
        np.testing.assert_allclose(got_e, want_sum, rtol=1e-12, atol=1e-12)
        total = total + got_e
    if case != "local_step":
        assert any(not e.all() for _, _, e in ref[1:]) or n == 1      # real chains' headings are generally not fixed points of the division
    # the three objectives on top of it
    init = 3.5
    np.testing.assert_array_equal(_bits(of.obj_global_error_sum(S, (graph, steps, 1.0, 0.1, PREV))), _bits(total))
    assert isinstance(of.obj_global_error_sum(S[0], (graph, steps, 1.0, 0.1, PREV)), float)
    rv = of.obj_global_residual_vector(S, (graph, steps, 1.0, 0.1, PREV, init))
    want = np.hstack([of._pad(b, st.n_spatial_components) for b, st in zip(blocks, steps)]) / init
    np.testing.assert_array_equal(_bits(rv), _bits(want))
    rn = of.obj_global_residual_vector_and_naturalness(S, (graph, steps, 0.8, 0.05, PREV, init))
    assert rn.shape == want.shape and np.isfinite(rn).all()
    # ... whose chain hands the last CONTROL POINT on: its own reference
    ref_c = _reference(world, case, S[:min(n, 4)], "coeffs")
    blocks_c = of._global_blocks(S[:min(n, 4)], graph, steps, PREV, "coeffs")[2]
    for i, ((want_b, _, exact), got_b) in enumerate(zip(ref_c, blocks_c)):
        kw, tw = _column_weights(CASES[case][0][i])
        assert (np.abs(got_b - want_b) <= _column_bounds(kw, tw, world.prims[SEQUENCE[i]]._grid_size(None))[None, :]).all()
        np.testing.assert_array_equal(_bits(got_b[exact]), _bits(want_b[exact]))


@pytest.mark.parametrize("case", sorted(CASES))
def test_one_launch_gives_the_bits_of_the_chain(world, case):
    graph, steps = world.walk(case)
    n_traj = sum(c["type"] == "trajectory" for lst in CASES[case][0] for c in lst)
    init = 3.5
    for exit_from in ("frames", "coeffs"):
        obj = of.HipGraphWalkObjective(graph, steps, PREV, exit_from)
        for n in BATCHES:
            for dtype in (np.float64, np.float32):
                S = _latents(n, dtype)
                before = obj.n_launches
                got = obj.blocks(S)
                assert obj.n_launches - before == 1 + n_traj
                _, _, want, errors = of._global_blocks(S, graph, steps, PREV, exit_from)
                _same_blocks(got, want)
                np.testing.assert_allclose(obj.error_sum(S), sum(errors), rtol=1e-9, atol=1e-9)
        assert obj.blocks(np.zeros((0, obj.n_latents)))[1].shape[0] == 0
        obj.close()
    S = _latents(17)
    data = (graph, steps, 1.0, 0.1, PREV)
    np.testing.assert_allclose(of.obj_global_error_sum_one_launch(S, data), of.obj_global_error_sum(S, data), rtol=1e-9, atol=1e-9)
    assert isinstance(of.obj_global_error_sum_one_launch(S[2], data), float)
    a, b = of.obj_global_residual_vector_one_launch(S, data + (init,)), of.obj_global_residual_vector(S, data + (init,))
    np.testing.assert_array_equal(_bits(a), _bits(b))
    data = (graph, steps, 0.8, 0.05, PREV, init)
    a, b = of.obj_global_residual_vector_and_naturalness_one_launch(S, data), of.obj_global_residual_vector_and_naturalness(S, data)
    np.testing.assert_array_equal(_bits(a), _bits(b))
    np.testing.assert_array_equal(_bits(of.obj_global_residual_vector_and_naturalness_one_launch(S[2], data)), _bits(b[2]))
    of.clear_walk_objectives()


@pytest.mark.parametrize("search,lanes", [(1, 0), (1, 1)])
def test_one_launch_under_the_other_search(world, search, lanes):
    """The monotone walk, eight lanes per candidate and one: the chained launch takes the route of the unchained one."""
    world.ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
    world.ctx.set_option(_capi.MG_OPT_TRAJECTORY_LANES, lanes)
    try:
        graph, steps = world.walk("first_step_too")
        obj = of.HipGraphWalkObjective(graph, steps, PREV, "frames")
        S = _latents(64)
        _same_blocks(obj.blocks(S), of._global_blocks(S, graph, steps, PREV, "frames")[2])
        obj.close()
    finally:
        world.ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
        world.ctx.set_option(_capi.MG_OPT_TRAJECTORY_LANES, 0)


@pytest.mark.parametrize("case", ["later_steps", "local_step"])
def test_the_exit_values_of_every_step(world, case):
    """mg_score_walk_residuals_steps: row [:, i] is the state the chain carries after step i, the last row is exit_state; without
    step_exits the call is mg_score_walk_residuals and gives the same bits."""
    graph, steps = world.walk(case)
    obj = of.HipGraphWalkObjective(graph, steps, PREV, "frames")
    for n in (1, 17, 64, 65):
        for dtype in (np.float64, np.float32):
            S = _latents(n, dtype)
            states = []
            of._global_blocks(S, graph, steps, PREV, "frames", states=states)
            res, err, ex, st = obj.table.score(S, obj.n_columns, step_exits=True)
            res0, err0, ex0 = obj.table.score(S, obj.n_columns)
            for a, b in ((res, res0), (err, err0), (ex, ex0)):
                np.testing.assert_array_equal(_bits(a), _bits(b))
            assert st.shape == (n, len(steps), 4)
            np.testing.assert_array_equal(_bits(st[:, -1, :]), _bits(ex0))
            for i, state in enumerate(states):
                np.testing.assert_array_equal(_bits(st[:, i, :]), _bits(state), err_msg="step %d" % i)
    # only the exit values asked for
    only = obj.table.score(_latents(17), obj.n_columns, residuals=False, errors=False, exit_state=False, step_exits=True)
    assert only[:3] == (None, None, None)
    np.testing.assert_array_equal(_bits(only[3]), _bits(obj.table.score(_latents(17), obj.n_columns, step_exits=True)[3]))
    obj.close()


def test_report():
    print("chained steps: %d candidates exact, %d within the bound, largest |difference| %.3e" % (WORST["exact"], WORST["bounded"], WORST["diff"]))
