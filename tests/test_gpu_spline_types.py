"""B-spline and fitted-B-spline trajectories (the reference's SPLINE_TYPE_BSPLINE = 1, SPLINE_TYPE_FITTED_BSPLINE = 2) on the device:
mg_trajectory_create_typed builds the tables, every kernel that takes a mg_trajectory reads them as it reads a Catmull-Rom spline's.

What is compared with what, and at which bound:
  * the device's tables against the host statement (spline_types.trajectory_polynomials_host / arc_length_table_host): both are host
    float64 arithmetic in the same order -- expected equal bit for bit, allowed one rounding;
  * the device's points and arc-length look-ups against the reference's own (tests/golden/trajectory_spline_types.npz) at the CPU
    test's BOUND (tests/test_spline_types_host.py: 16 x the measured conversion difference) plus one rounding of the largest
    coordinate per axis for the device's evaluation;
  * the closest-point search against the reference's find_closest_point_fast values at test_spline_types_host.closest_point_bounds:
    twice what the Catmull-Rom test tolerates relative to the path length (|du| <= 4e-6, |dd| <= 8.02e-6 of the path length); a case
    is left out only where the parameters differ by more than one cell of the granularity-1000 grid (another basin), at most 5 %;
  * every kernel route against a NumPy evaluation on the statement's polynomials: the oracle's one-variable L-BFGS-B at the sweep's
    tolerance for that pairing (tests/test_gpu_trajectory_shapes.py: 1e-6 max(1, d)), the monotone walk restated below (held to
    oracle.mg_oracle.closest_point_walk on a Catmull-Rom table by a CPU test) at 1e-9.
The tests print what they measure."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd.spline_types import arc_length_table_host, polynomial_point, trajectory_polynomials_host
from oracle import mg_oracle as orc
from test_spline_types_host import BOUND, CURVES, POINTS, closest_point_bounds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MG_ERR_INVALID_ARGUMENT = -1
D_TOL, WALK_TOL = 1.0e-6, 1.0e-9          # tests/test_gpu_trajectory_shapes.py
WEIGHT = 1.5
BATCHES = (1, 17, 65)


# ---- NumPy evaluations on the statement's table --------------------------------------------------------------------------------------
def _d2(poly, u, q):
    v = polynomial_point(poly, u) - q
    return float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def _derivatives(poly, u):
    """mg_traj_d2_derivs' dP/du and d2P/du2 (zero past the last piece)"""
    n_seg = (len(poly) - 3) // 12
    scaled = n_seg * float(u)
    index = int(math.floor(scaled))
    if index >= n_seg:
        return np.zeros(3), np.zeros(3)
    t = scaled - index
    A = poly[index * 12:index * 12 + 12].reshape(4, 3)
    return n_seg * ((3.0 * A[0] * t + 2.0 * A[1]) * t + A[2]), n_seg * n_seg * (6.0 * A[0] * t + 2.0 * A[1])


def lbfgsb_on_poly(poly, q, min_u):
    """find_closest_point_fast as the device runs it (oracle.mg_oracle.closest_point_lbfgsb) on a table of any type"""
    u = orc.lbfgsb_1d(lambda x: math.sqrt(_d2(poly, x, q)), float(min_u), float(min_u), 1.0, formk_rule=True)
    return u, math.sqrt(_d2(poly, u, q))


def walk_on_poly(poly, q, min_u, G=1000):
    """oracle.mg_oracle.closest_point_walk (MG_OPT_TRAJECTORY_SEARCH 1) restated on a table of any type"""
    k = min(G, int(math.ceil(min_u * G - 1e-12)))
    dk = _d2(poly, k / G, q)
    d_start = _d2(poly, min_u, q)
    while k < G:
        dn = _d2(poly, (k + 1) / G, q)
        if dn >= dk:
            break
        k, dk = k + 1, dn
    u = k / G
    if 0 < k < G:
        a, c = _d2(poly, (k - 1) / G, q), _d2(poly, (k + 1) / G, q)
        den = a - 2.0 * dk + c
        if den > 0.0:
            u = (k + 0.5 * (a - c) / den) / G
    lo, hi = max(float(min_u), (k - 1) / G), min(1.0, (k + 1) / G)
    u = min(hi, max(lo, u))
    for _ in range(4):
        v = polynomial_point(poly, u) - q
        p1, p2 = _derivatives(poly, u)
        f1, f2 = 2.0 * float(v @ p1), 2.0 * float(p1 @ p1 + v @ p2)
        if not f2 > 0.0:
            break
        un = min(hi, max(lo, u - f1 / f2))
        if _d2(poly, un, q) > _d2(poly, u, q):
            break
        u = un
    u = min(1.0, max(float(min_u), u))
    if d_start <= _d2(poly, u, q):
        u = float(min_u)
    return u, math.sqrt(_d2(poly, u, q))


def chain_on_poly(poly, path, min_u, search):
    ds = []
    for q in path:
        min_u, d = (walk_on_poly if search == 1 else lbfgsb_on_poly)(poly, q, min_u)
        ds.append(d)
    return np.array(ds)


def test_the_restated_walk_is_the_oracles_walk():
    """walk_on_poly on a Catmull-Rom table against oracle.mg_oracle.closest_point_walk, chained over a path: the restatement the walk
    routes below are held to is the pinned one.  At WALK_TOL, the bound the device's walk is held to against the same function: the
    two evaluate the same cubic in different forms (Horner on the table, a matrix product on the control points), and the parameter of
    a minimum is only determined to about the square root of the distance's rounding."""
    rng = np.random.default_rng(8)
    cps = np.cumsum(np.column_stack([rng.uniform(20, 60, 6), rng.uniform(-3, 3, 6), rng.uniform(-40, 40, 6)]), axis=0)
    poly = trajectory_polynomials_host(cps, 0)
    s = np.linspace(0.0, 1.1, 30)
    path = cps[0] + s[:, None] * (cps[-1] - cps[0]) + rng.normal(0.0, 3.0, (30, 3))
    mu_a = mu_b = 0.1
    for q in path:
        _, mu_a = orc.closest_point_walk(cps, q, mu_a)
        mu_b, _ = walk_on_poly(poly, q, mu_b)
        assert abs(mu_a - mu_b) <= WALK_TOL, (mu_a, mu_b)


# ---- the device ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trajectory_spline_types.npz"))


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiny(ctx):
    """the existing tiny model: L = 3, D = 7, F = 12"""
    data = synthetic.make_tiny_primitive()
    p = _capi.Primitive(ctx, data)
    yield p
    p.close()


@pytest.fixture(autouse=True)
def _default_options(request):
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        if c.handle:
            c.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
            c.set_option(_capi.MG_OPT_TRAJECTORY_LANES, 0)


def _set(ctx, search, opt):
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_LANES, opt)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _frame_constraint(prim, desc, track):
    """mg_score_frame_constraint for one candidate on a given track (T, J, 3): the residual vector"""
    ctx, lib = prim.ctx, prim.lib
    track = np.ascontiguousarray(track, dtype=np.float64)
    T, J = track.shape[:2]
    m = lib.mg_frame_constraint_width(C.byref(desc), T)
    d_t, d_e, d_r = ctx.upload(track[None]), ctx.malloc(8), ctx.malloc(max(m, 1) * 8)
    try:
        _capi._check(lib.mg_score_frame_constraint(prim.handle, C.byref(desc), d_t.ptr, 1, T, J, d_e.ptr, 0, d_r.ptr))
        return ctx.download(d_r, (m,), np.float64)
    finally:
        for b in (d_t, d_e, d_r):
            b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("spline_type,n_points", CURVES + [(0, 5)])
def test_device_tables_are_the_host_statement(tiny, golden, spline_type, n_points):
    """poly, the arc-length table and the full arc length as the kernels read them against the NumPy statement: one rounding at most
    (measured: the number of differing words is printed, 0 expected)."""
    cps = golden["control_points_%d_%d" % (spline_type, n_points)] if spline_type else np.load(os.path.join(GOLDEN, "trajectory_spline.npz"))["control_points_1"]
    traj = _capi.Trajectory(tiny, cps, 1000, spline_type)
    try:
        assert tiny.lib.mg_trajectory_spline_type(traj.handle) == spline_type
        poly, arc, full = traj.tables()
    finally:
        traj.close()
    want = trajectory_polynomials_host(cps, spline_type)
    want_arc, want_full = arc_length_table_host(want, 1000)
    print("type %d, %d points: differing words: poly %d of %d, arc table %d of %d, full arc length %d" % (
        spline_type, n_points, int((_bits(poly) != _bits(want)).sum()), len(want), int((_bits(arc) != _bits(want_arc)).sum()), len(arc), int(full != want_full)))
    assert poly.shape == want.shape and (np.abs(poly - want) <= np.spacing(np.abs(want))).all()
    assert (np.abs(arc - want_arc) <= np.spacing(1.0)).all() and abs(full - want_full) <= np.spacing(want_full)


@pytest.mark.gpu
@pytest.mark.parametrize("spline_type,n_points", CURVES)
def test_device_points_and_arc_lengths_against_the_reference(tiny, golden, spline_type, n_points):
    """Points by parameter: mg_trajectory_closest_points with the reference's point as the target and its parameter as the bound --
    the search starts at the bound, where the projected gradient is zero, and returns the distance from the device's point at that
    parameter to the reference's.  Points by arc length: the local-trajectory kind of mg_score_frame_constraints (x and z: its
    residual is the squared xz distance to the target looked up at start_t) and the trajectory-set kind (the mean of all three
    components) on a one-frame track that stands on the reference's point."""
    key = "%d_%d" % (spline_type, n_points)
    cps = golden["control_points_" + key]
    one_rounding = math.sqrt(3.0) * float(np.spacing(np.abs(cps).max()))
    bound = BOUND + one_rounding
    poly = trajectory_polynomials_host(cps, spline_type)
    traj = _capi.Trajectory(tiny, cps, 1000, spline_type)
    worst_p = worst_s = worst_xz = worst_mean = 0.0
    try:
        for u_ref, pt in zip(golden["parameters_" + key], golden["points_" + key]):
            u, d = tiny.trajectory_closest_points(traj, pt[None, None, :], float(u_ref))
            assert u[0, 0] == u_ref, (u_ref, u[0, 0])
            worst_p = max(worst_p, float(d[0, 0]))
            worst_s = max(worst_s, abs(float(d[0, 0]) - float(np.linalg.norm(polynomial_point(poly, u_ref) - pt))))
        full = float(golden["full_arc_length_" + key])
        for arc, pt in zip(golden["arc_lengths_" + key], golden["points_by_arc_" + key]):
            desc = _capi.FrameConstraintDesc()
            desc.type, desc.weight, desc.n_joints, desc.n_frames, desc.start_arc = _capi.MG_FRAME_LOCAL_TRAJECTORY, 1.0, 1, 1, float(arc)
            desc.trajectories[0] = traj.handle.value
            worst_xz = max(worst_xz, math.sqrt(float(_frame_constraint(tiny, desc, pt[None, None, :])[0])))
            desc = _capi.FrameConstraintDesc()
            desc.type, desc.weight, desc.n_joints, desc.n_frames = _capi.MG_FRAME_TRAJECTORY_SET, 1.0, 1, 1
            desc.trajectories[0], desc.arc0[0], desc.has_range[0] = traj.handle.value, float(arc), 1
            desc.range_start[0], desc.range_end[0] = -1.0, 2.0 * full
            worst_mean = max(worst_mean, float(_frame_constraint(tiny, desc, pt[None, None, :])[0]))
    finally:
        traj.close()
    print("type %d, %d points: device against the reference: points %.3e, by arc length xz %.3e, mean of components %.3e (bound %.3e); "
          "device against the statement's distance %.3e (one rounding %.3e)" % (spline_type, n_points, worst_p, worst_xz, worst_mean, bound, worst_s, one_rounding))
    assert worst_p <= bound and worst_xz <= bound and worst_mean <= bound and worst_s <= one_rounding


@pytest.mark.gpu
@pytest.mark.parametrize("spline_type,n_points", CURVES)
def test_closest_points_against_the_references_search(tiny, golden, spline_type, n_points):
    """mg_trajectory_closest_points on the fixture's targets against the reference's own find_closest_point_fast"""
    key = "%d_%d" % (spline_type, n_points)
    u_tol, d_tol = closest_point_bounds(float(golden["full_arc_length_" + key]))
    targets, min_us, u_ref, d_ref = (golden[n + key] for n in ("cp_targets_", "cp_min_u_", "cp_u_", "cp_distance_"))
    traj = _capi.Trajectory(tiny, golden["control_points_" + key], 1000, spline_type)
    u, d = np.empty(len(u_ref)), np.empty(len(u_ref))
    try:
        for m in (0.0, 0.3):
            sel = min_us == m
            uu, dd = tiny.trajectory_closest_points(traj, targets[sel][:, None, :], m)
            u[sel], d[sel] = uu[:, 0], dd[:, 0]
    finally:
        traj.close()
    same = np.abs(u - u_ref) <= 1.0e-3
    du, dd = np.abs(u - u_ref)[same].max(), np.abs(d - d_ref)[same].max()
    print("type %d, %d points: |du| %.3e (bound %.1e), |dd| %.3e (bound %.3e = %.3e of the path length), left out (another basin) %d of %d" % (
        spline_type, n_points, du, u_tol, dd, d_tol, d_tol / float(golden["full_arc_length_" + key]), int((~same).sum()), len(same)))
    assert (~same).sum() <= 0.05 * len(same) and du <= u_tol and dd <= d_tol


def _tiny_cps(n, shift=0.0):
    """a target curve beside the tiny model's root paths (tests/test_gpu_trajectory_shapes.py's tiny row runs from (-80, 0, -60) to (90, 5, 70))"""
    s = np.linspace(0.0, 1.0, n)
    return np.column_stack([-80.0 + 170.0 * s + shift, 5.0 * s + 2.0 * np.sin(5.0 * s), -60.0 + 130.0 * s + 12.0 * np.sin(4.0 * s + shift)])


ROUTES = [(0, 0, "stream"), (1, 1, "stream"), (1, 8, "coop8"), (1, 4, "coop4")]             # (search, lanes option, kernel) on the root rows
ROUTES_MULTI = [(0, 0, "stream_multi"), (1, 1, "stream_multi"), (1, 8, "coop8_multi"), (1, 4, "coop4_multi")]
LONG = {1: 1689, 2: 1687}      # control points whose pieces (1686) no longer fit LDS on the points route: the polynomials stay in global memory


@pytest.mark.gpu
@pytest.mark.parametrize("spline_type", [1, 2])
def test_every_kernel_route_on_typed_trajectories(ctx, tiny, spline_type):
    """mg_score_trajectory on the tiny primitive with a typed trajectory through the routes mg_trajectory_plan names for its root
    rows (stream, coop8, coop4), mg_score_trajectories for the side-by-side forms, mg_score_trajectory_points for the staged
    kernels (polynomials in LDS; in global memory for a spline of 1686 pieces): 1, 17 and 65 candidates.  Every route of a search gives
    the same bits; every candidate is held to the NumPy evaluation on the statement's polynomials."""
    L, rows, T = 3, 3 * 7 + 4, tiny.n_canonical_frames
    S = np.random.default_rng(40 + spline_type).standard_normal((max(BATCHES), L))
    P = tiny.back_project_frames_f64(S)[:, :, :3].copy()            # the candidates' root paths
    cps = _tiny_cps(9)
    poly = trajectory_polynomials_host(cps, spline_type)
    n_seg = (len(poly) - 3) // 12
    traj = _capi.Trajectory(tiny, cps, 1000, spline_type)
    other = _capi.Trajectory(tiny, _tiny_cps(7, 3.0), 1000, 3 - spline_type)     # the second scorer of the side-by-side launches: the other type
    long_cps = _tiny_cps(LONG[spline_type])
    long_traj = _capi.Trajectory(tiny, long_cps, 1000, spline_type)
    seen = set()
    try:
        want = {s: np.stack([chain_on_poly(poly, P[b], 0.25, s) for b in range(max(BATCHES))]) for s in (0, 1)}
        worst = {0: 0.0, 1: 0.0}
        base = {}
        for search, opt, kernel in ROUTES:
            _set(ctx, search, opt)
            for B in BATCHES[::-1]:         # (the largest batch first: the smaller ones are held to its rows)
                assert ctx.trajectory_plan(L, rows, n_seg, B)["kernel"] == kernel, (search, opt, B)
                err, res = tiny.score_trajectory(traj, S[:B], min_u=0.25, weight=WEIGHT, residuals=True)
                base.setdefault(search, res)
                np.testing.assert_array_equal(_bits(res), _bits(base[search][:B]), err_msg=str((search, opt, B)))
                np.testing.assert_allclose(err, res.mean(axis=1), rtol=1e-13, atol=1e-13)
                dd = np.abs(res / WEIGHT - want[search][:B]) / np.maximum(1.0, want[search][:B])
                worst[search] = max(worst[search], float(dd.max()))
                assert dd.max() <= (WALK_TOL if search == 1 else D_TOL), (search, opt, B, float(dd.max()))
            seen.add(kernel)
        # side by side: two scorers (this type and the other one) in one launch, the bits of the single launches
        for search, opt, kernel in ROUTES_MULTI:
            _set(ctx, search, opt)
            for B in BATCHES:
                assert ctx.trajectory_plan(L, rows, n_seg, B, 2 * B)["kernel"] == kernel, (search, opt, B)
                singles = [tiny.score_trajectory(t, S[:B], min_u=m, weight=WEIGHT) for t, m in ((traj, 0.25), (other, 0.0))]
                d_S, d_e = ctx.upload(S[:B]), [ctx.malloc(B * 8) for _ in range(2)]
                try:
                    _capi.Primitive.score_trajectories_dev([tiny, tiny], [traj, other], [d_S, d_S], S.dtype, B, [L, L], d_e, [0.25, 0.0], [WEIGHT] * 2)
                    got = [ctx.download(e, (B,), np.float64) for e in d_e]
                finally:
                    for b in [d_S] + d_e:
                        b.free()
                for k in range(2):
                    np.testing.assert_array_equal(_bits(got[k]), _bits(singles[k]), err_msg=str((search, opt, B, k)))
            seen.add(kernel)
        # the staged kernels: given points (the same root paths: the bits of the root route), polynomials in LDS and in global memory
        for search in (0, 1):
            _set(ctx, search, 1)
            for B in BATCHES:
                assert ctx.trajectory_plan(L, rows, n_seg, B, points=True)["kernel"] == "staged_lds"
                err, res = tiny.score_trajectory_points(traj, P[:B], 0.25, weight=WEIGHT, residuals=True)
                np.testing.assert_array_equal(_bits(res), _bits(base[search][:B]), err_msg=str(("points", search, B)))
            seen.add("staged_lds")
        long_poly = trajectory_polynomials_host(long_cps, spline_type)
        assert (len(long_poly) - 3) // 12 == 1686
        for search in (0, 1):
            _set(ctx, search, 1)
            long_base = None
            for B in BATCHES[::-1]:
                assert ctx.trajectory_plan(L, rows, 1686, B, points=True)["kernel"] == "staged_global"
                err, res = tiny.score_trajectory_points(long_traj, P[:B], 0.0, weight=WEIGHT, residuals=True)
                long_base = res if long_base is None else long_base
                np.testing.assert_array_equal(_bits(res), _bits(long_base[:B]), err_msg=str(("long", search, B)))
            for b in (0, 16, 64):
                w = chain_on_poly(long_poly, P[b], 0.0, search)
                dd = np.abs(long_base[b] / WEIGHT - w) / np.maximum(1.0, w)
                worst[search] = max(worst[search], float(dd.max()))
                assert dd.max() <= (WALK_TOL if search == 1 else D_TOL), ("long", search, b, float(dd.max()))
            seen.add("staged_global")
    finally:
        for t in (traj, other, long_traj):
            t.close()
    assert seen == set(_capi.MG_TRAJ_KERNELS), sorted(set(_capi.MG_TRAJ_KERNELS) ^ seen)
    print("type %d: worst |dd| / max(1, d) against the NumPy evaluation: reference search %.3e (tolerance %.1e), walk %.3e (%.1e)" % (
        spline_type, worst[0], D_TOL, worst[1], WALK_TOL))


@pytest.mark.gpu
def test_planner_step_with_b_spline_trajectories_equals_option_by_option():
    """One planner step whose two options each carry a type-1 trajectory: the winners of the options scored one by one, bit for bit,
    the two trajectories in ONE side-by-side launch, and the device objects the step made are B-splines."""
    from morphablegraphs_amd import candidate_scoring as cs
    from morphablegraphs_amd.candidate_scoring import sample_and_evaluate_on_device
    from morphablegraphs_amd.motion_state_graph import HipPrimitiveSet
    prims = synthetic.make_graph_primitives(2)
    names = [p["name"] for p in prims]
    sk = _capi.Skeleton(*synthetic.make_skeleton())
    pset = HipPrimitiveSet(prims)

    wrapped = {}
    for i, (nm, p) in enumerate(zip(names, prims)):
        traj = {"type": "trajectory", "control_points": [[0.0, 0.0, 0.0], [5.0 + i, 0.0, 2.0], [9.0, 0.5, 6.0], [12.0, 0.0, 3.0 + i], [20.0, 0.0, -2.0]],
                "min_u": 0.0, "weight": 0.5, "granularity": 1000, "spline_type": 1}
        cl = [{"type": "position", "t": float(p["n_canonical_frames"] - 1), "weight": 1.0, "target": [10.0, None, 5.0]}, traj]
        wrapped[nm] = type("Cons", (), {"constraints": cl, "hip_skeleton": sk, "is_local": True})()
    np.random.seed(17)
    pset.ctx.profile_reset(); pset.ctx.profile_enable(1)
    best, res = pset.evaluate_options_on_device(names, wrapped, n_samples=777, seed=40)
    launches = pset.ctx.profile_get("trajectory")[1]
    pset.ctx.profile_enable(0)
    assert launches == 1, launches
    # the step's own device trajectories are B-splines: one per option in the cache, keyed by the type
    for nm in names:
        cps = wrapped[nm].constraints[1]["control_points"]
        mine = [t for k, t in cs._TRAJ_CACHE if len(k) == 5 and k[2] == cs._freeze(cps) and k[4] == 1 and t.handle]
        assert len(mine) == 1 and mine[0].prim.lib.mg_trajectory_spline_type(mine[0].handle) == 1, nm
        assert not [k for k, _ in cs._TRAJ_CACHE if len(k) == 4 and k[2] == cs._freeze(cps)], nm
    np.random.seed(17)
    for k, nm in enumerate(names):
        lat, err = sample_and_evaluate_on_device(pset.nodes[nm], wrapped[nm], 777, seed=40 + k)
        np.testing.assert_array_equal(res[nm][0], lat, err_msg=nm)
        assert res[nm][1] == err, (nm, res[nm][1], err)
    assert best == names[int(np.argmin([res[nm][1] for nm in names]))]


@pytest.mark.gpu
def test_type_0_through_the_typed_entry_point_is_mg_trajectory_create(tiny):
    """mg_trajectory_create_typed(..., MG_SPLINE_CATMULL_ROM, ...) forwards: the same tables and the same scores, bit for bit"""
    cps = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "trajectory_spline.npz"))["control_points_2"])
    plain = _capi.Trajectory(tiny, cps, 1000)
    h = C.c_void_p()
    _capi._check(tiny.lib.mg_trajectory_create_typed(tiny.handle, cps.ctypes.data_as(C.c_void_p), len(cps), 1000, 0, C.byref(h)))
    typed = _capi.Trajectory.__new__(_capi.Trajectory)
    typed.prim, typed.handle, typed.spline_type = tiny, h, 0
    try:
        assert tiny.lib.mg_trajectory_spline_type(h) == 0
        for a, b in zip(plain.tables(), typed.tables()):
            np.testing.assert_array_equal(_bits(a), _bits(b))
        np.testing.assert_array_equal(_bits(plain.tables()[0]), _bits(trajectory_polynomials_host(cps, 0)))
        S = np.random.default_rng(2).standard_normal((65, 3))
        for a, b in zip(tiny.score_trajectory(plain, S, min_u=0.1, residuals=True), tiny.score_trajectory(typed, S, min_u=0.1, residuals=True)):
            np.testing.assert_array_equal(_bits(a), _bits(b))
    finally:
        plain.close()
        typed.close()


@pytest.mark.gpu
def test_refusals_report_and_launch_nothing(ctx, tiny):
    """three control points for types 1 and 2, an unknown type, a non-finite coordinate: MG_ERR_INVALID_ARGUMENT with a message in
    the library's style, no object, no launch"""
    ctx.profile_reset(); ctx.profile_enable(1)
    try:
        for spline_type, what in ((1, "B-spline"), (2, "fitted B-spline")):
            with pytest.raises(_capi.MGError) as e:
                _capi.Trajectory(tiny, POINTS[:3], 1000, spline_type)
            assert e.value.status == MG_ERR_INVALID_ARGUMENT and ">= 4 control points (x, y, z) for a %s" % what in str(e.value)
            bad = np.array(POINTS)
            bad[2, 1] = np.inf
            with pytest.raises(_capi.MGError) as e:
                _capi.Trajectory(tiny, bad, 1000, spline_type)
            assert e.value.status == MG_ERR_INVALID_ARGUMENT and "control point 2 is not finite" in str(e.value)
        for unknown in (3, -1):
            with pytest.raises(_capi.MGError) as e:
                _capi.Trajectory(tiny, POINTS, 1000, unknown)
            assert e.value.status == MG_ERR_INVALID_ARGUMENT and "unknown spline type %d" % unknown in str(e.value)
        assert ctx.profile_get("trajectory")[1] == 0 and ctx.profile_get("frame_constraints")[1] == 0
    finally:
        ctx.profile_enable(0)
    assert tiny.lib.mg_trajectory_spline_type(None) == -1
