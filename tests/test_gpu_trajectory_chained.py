"""mg_score_trajectory_chained: the trajectory scorer with every candidate aligned to its own previous motion.

The reference for every case is the single-record scorer, mg_score_trajectory: align_cand is dealt from K = 4 records in a
pattern that makes neighbouring lanes (and neighbouring lane groups of the cooperative kernels) differ; per record the whole
batch is scored with that record as `alignment`, and the rows that carry the record are taken.  The chained call reads a
candidate's four values as they are where the single-record call divides its heading by sqrt(hx * hx + hz * hz) on the host:
the records' headings are axis aligned, that division leaves them as they are (asserted below with the library's expression),
so errors and residuals must be the SAME BITS -- no tolerance applies.

Every one of the five single-launch kernels is reached (by the search, the lane option and the length of the target spline,
as tests/test_gpu_trajectory_shapes.py steers them); the plan is read from mg_trajectory_plan for the shape that ran, and
test_every_single_launch_kernel_ran fails when one of them stops being reached."""
import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd.candidate_scoring import alignment_from_start_pose

pytestmark = pytest.mark.gpu

L, F, NB, D = 6, 20, 7, 7
ROWS = 3 * NB + 4
BATCHES = (1, 63, 64, 65, 130)        # MG_TRAJ_BLOCK is 64; a wave holds 8 or 16 candidates of the cooperative kernels
WEIGHT = 1.5
SENTINEL = 0x7FF8000000C0FFEE
REF_DIR = (0.0, 0.0, 1.0)
# K = 4 previous-frame records: unit heading (x, z), root position (x, z)
RECORDS = [((0.0, 1.0), (30.0, -15.0)), ((1.0, 0.0), (-12.5, 40.0)), ((0.0, -1.0), (0.0, 0.0)), ((-1.0, 0.0), (7.25, 3.5))]
LEDGER = set()
SINGLE_LAUNCH_KERNELS = {"staged_lds", "staged_global", "stream", "coop8", "coop4"}
# route -> (search, MG_OPT_TRAJECTORY_LANES, control points of the target spline, the kernel the plan must name)
ROUTES = {
    "stream_reference_search": (0, 0, 7, "stream"),
    "stream_walk": (1, 1, 7, "stream"),
    "coop8": (1, 8, 7, "coop8"),
    "coop4": (1, 4, 7, "coop4"),
    "staged_lds": (0, 0, 700, "staged_lds"),          # 699 segments: the polynomials pass the streaming kernel's 60 KB
    "staged_lds_walk": (1, 8, 700, "staged_lds"),     # ... and the cooperative kernels'
    "staged_global": (1, 0, 1600, "staged_global"),   # 1599 segments: rows and polynomials pass 158 KB, the table stays in global memory
}
# (latent dtype, accumulate onto a pre-filled buffer, residuals, grid)
COMBOS = [(np.float64, False, True, None), (np.float32, True, True, "short"), (np.float64, True, False, None), (np.float32, False, False, "short")]


def _curve(t):
    t = np.asarray(t, dtype=np.float64)
    return np.stack([160.0 * t, 90.0 + 2.0 * np.sin(6.0 * t), 40.0 * np.sin(2.0 * t)], axis=-1)


def _control_points(n):
    t = np.linspace(0.0, 1.0, n)
    cps = _curve(t)
    cps[:, 0] += 6.0 * t
    cps[:, 2] -= 4.0 * t
    return cps


def _model():
    """A root-only primitive whose root path follows _curve, varied by a few units by the latents."""
    data = synthetic.make_primitive(seed=9100, name="chained", n_components=L, n_frames=F, n_basis=NB, n_dim=D, n_gmm=1)
    mean = np.array(data["mean_spatial_vector"]).reshape(NB, D)
    eig = np.array(data["eigen_vectors_spatial"]).reshape(L, NB, D)
    mean[:, :3] = _curve(np.linspace(0.0, 1.0, NB))
    eig[:, :, :3] *= 0.03
    data["mean_spatial_vector"] = mean.reshape(-1).tolist()
    data["eigen_vectors_spatial"] = eig.reshape(L, -1).tolist()
    return data


def _record(k):
    (hx, hz), (px, pz) = RECORDS[k]
    return {"joint": 0, "position": (px, 0.0, pz), "heading": (hx, hz), "ref_dir": REF_DIR}


TEMPLATE = {"joint": 0, "position": (0.0, 0.0, 0.0), "heading": (0.0, 1.0), "ref_dir": REF_DIR}


def _deal(B):
    """The record of every candidate: neighbours differ, and so do the neighbours of every fourth and eighth candidate."""
    b = np.arange(B)
    return (b + b // 4 + b // 8) % len(RECORDS)


def _align_cand(B):
    return np.array([RECORDS[k][0] + RECORDS[k][1] for k in _deal(B)], dtype=np.float64).reshape(B, 4)


def test_the_records_headings_survive_the_hosts_normalisation():
    """mg_traj_fill_args: hn = sqrt(h[0] * h[0] + h[1] * h[1]); al[0] = h[0] / hn; al[1] = h[1] / hn -- in float64, as here."""
    for (hx, hz), _ in RECORDS:
        hx, hz = np.float64(hx), np.float64(hz)
        hn = np.sqrt(hx * hx + hz * hz)
        assert (hx / hn).tobytes() == hx.tobytes() and (hz / hn).tobytes() == hz.tobytes() and hn == 1.0
    assert len({r[0] for r in RECORDS}) == len(RECORDS) and len({r[1] for r in RECORDS}) == len(RECORDS)
    for B in BATCHES[1:]:
        deal = _deal(B)
        assert (np.diff(deal) != 0).all() and set(deal) == set(range(len(RECORDS)))
        assert (deal[8:] != deal[:-8]).any() and (deal[4:] != deal[:-4]).any()


@pytest.fixture(scope="module")
def world():
    ctx = _capi.Context(0)
    prim = _capi.Primitive(ctx, _model())
    w = {"ctx": ctx, "prim": prim, "traj": {}, "grid": prim.time_grid(np.array([0.0, 3.5, 7.25, 11.0, 12.5, F - 1.0]))}
    for n in (7, 700, 1600):
        w["traj"][n] = _capi.Trajectory(prim, _control_points(n), granularity=1000)
    w["traj"]["bspline"] = _capi.Trajectory(prim, _control_points(9), 1000, _capi.MG_SPLINE_BSPLINE)
    w["traj"]["fitted"] = _capi.Trajectory(prim, _control_points(9), 1000, _capi.MG_SPLINE_FITTED_BSPLINE)
    w["S"] = np.random.default_rng(77).standard_normal((max(BATCHES), L))
    yield w
    for t in w["traj"].values():
        t.close()
    w["grid"].close()
    prim.close()
    ctx.close()


@pytest.fixture(autouse=True)
def _default_options(request):
    yield
    if "world" in request.fixturenames:
        c = request.getfixturevalue("world")["ctx"]
        if c.handle:
            c.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
            c.set_option(_capi.MG_OPT_TRAJECTORY_LANES, 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _score(w, traj, S, grid, min_u, prefill, residuals, alignment=None, align_cand=None):
    """One launch on device buffers -> (errors (B,), residuals (B, T) or None).  align_cand: the chained entry point with
    `alignment` as its template.  The residual buffer starts as a sentinel pattern."""
    ctx, prim = w["ctx"], w["prim"]
    B, T = len(S), prim._grid_size(grid)
    start = prefill if prefill is not None else np.full(B, SENTINEL, dtype=np.uint64).view(np.float64)
    bufs = [ctx.upload(S), ctx.upload(start), ctx.upload(np.full(B * T, SENTINEL, dtype=np.uint64))]
    if align_cand is not None:
        bufs.append(ctx.upload(align_cand))
    try:
        d_S, d_e, d_r = bufs[:3]
        if align_cand is not None:
            prim.score_trajectory_chained_dev(traj, d_S, S.dtype, B, S.shape[1], bufs[3], alignment, d_e, min_u, WEIGHT, prefill is not None,
                                              d_r if residuals else None, grid)
        else:
            prim.score_trajectory_dev(traj, d_S, S.dtype, B, S.shape[1], d_e, min_u, WEIGHT, alignment, prefill is not None,
                                      d_r if residuals else None, grid)
        err = ctx.download(d_e, (B,), np.float64)
        res = ctx.download(d_r, (B, T), np.uint64)
        if residuals:
            assert not (res == SENTINEL).any(), "residuals the kernel never wrote"
            return err, res.view(np.float64)
        assert (res == SENTINEL).all(), "residuals written where none were asked for"
        return err, None
    finally:
        for b in bufs:
            b.free()


def _compare(w, traj, S, grid, min_u, prefill, residuals, tag):
    """The chained launch against the rows of K single-record launches over the same batch."""
    B = len(S)
    deal = _deal(B)
    err, res = _score(w, traj, S, grid, min_u, prefill, residuals, TEMPLATE, _align_cand(B))
    want_e = np.empty(B)
    want_r = np.empty((B, w["prim"]._grid_size(grid))) if residuals else None
    for k in range(len(RECORDS)):
        rows = deal == k
        if not rows.any():
            continue
        e, r = _score(w, traj, S, grid, min_u, prefill, residuals, _record(k))
        want_e[rows] = e[rows]
        if residuals:
            want_r[rows] = r[rows]
    np.testing.assert_array_equal(_bits(err), _bits(want_e), err_msg=str(tag))
    if residuals:
        np.testing.assert_array_equal(_bits(res), _bits(want_r), err_msg=str(tag))
    return err


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_chained_equals_the_single_record_rows_bit_for_bit(world, route):
    search, lanes, n_cp, kernel = ROUTES[route]
    ctx = world["ctx"]
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_LANES, lanes)
    traj = world["traj"][n_cp]
    rng = np.random.default_rng(3)
    moved = False
    for B in BATCHES:
        plan = ctx.trajectory_plan(L, ROWS, n_cp - 1, B)
        assert plan["kernel"] == kernel, (route, B, plan)
        for ci, (dtype, accumulate, residuals, gname) in enumerate(COMBOS):
            S = world["S"][:B].astype(dtype)
            grid = world["grid"] if gname == "short" else None
            assert grid is None or grid.size < F
            prefill = rng.standard_normal(B) if accumulate else None
            min_u = 0.0 if ci % 2 == 0 else 0.2
            err = _compare(world, traj, S, grid, min_u, prefill, residuals, (route, B, ci))
            if B >= 4 and not accumulate:
                moved = moved or len(set(np.round(err[:4], 6))) == 4     # the four records give four different answers: the alignment is read
        LEDGER.add(plan["kernel"])
    assert moved


@pytest.mark.parametrize("spline", ["bspline", "fitted"])
def test_the_other_spline_types(world, spline):
    ctx = world["ctx"]
    for search, lanes in ((0, 0), (1, 8)):
        ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
        ctx.set_option(_capi.MG_OPT_TRAJECTORY_LANES, lanes)
        for B in (65, 130):
            _compare(world, world["traj"][spline], world["S"][:B], None, 0.1, None, True, (spline, search, B))


def test_the_host_array_form(world):
    """Primitive.score_trajectory_chained (upload, launch, download) gives the device form's numbers."""
    B = 65
    S = world["S"][:B]
    err, res = world["prim"].score_trajectory_chained(world["traj"][7], S, _align_cand(B), TEMPLATE, 0.1, WEIGHT, residuals=True)
    e2, r2 = _score(world, world["traj"][7], S, None, 0.1, None, True, TEMPLATE, _align_cand(B))
    np.testing.assert_array_equal(_bits(err), _bits(e2))
    np.testing.assert_array_equal(_bits(res), _bits(r2))
    only = world["prim"].score_trajectory_chained(world["traj"][7], S, _align_cand(B), TEMPLATE, 0.1, WEIGHT)
    np.testing.assert_array_equal(_bits(only), _bits(err))
    assert world["prim"].score_trajectory_chained(world["traj"][7], S[:0], np.zeros((0, 4)), TEMPLATE).shape == (0,)


def test_argument_errors_launch_nothing(world):
    ctx, prim, traj = world["ctx"], world["prim"], world["traj"][7]
    B = 16
    S = world["S"][:B]
    d_S, d_A = ctx.upload(S), ctx.upload(_align_cand(B))
    d_e = ctx.upload(np.full(B, SENTINEL, dtype=np.uint64))
    start_pose = alignment_from_start_pose({"position": [3.0, 2.0, 1.0], "orientation": [0.0, 25.0, 0.0]})
    try:
        for template, align_cand, status in ((start_pose, d_A, _capi.MG_ERR_INVALID_ARGUMENT),
                                             (dict(TEMPLATE, joint=2), d_A, _capi.MG_ERR_UNSUPPORTED),
                                             (None, d_A, _capi.MG_ERR_INVALID_ARGUMENT),
                                             (TEMPLATE, None, _capi.MG_ERR_INVALID_ARGUMENT)):
            with pytest.raises(_capi.MGError) as e:
                prim.score_trajectory_chained_dev(traj, d_S, S.dtype, B, L, align_cand, template, d_e)
            assert e.value.status == status, (template, e.value)
            ctx.synchronize()
            assert (ctx.download(d_e, (B,), np.uint64) == SENTINEL).all()
        # no candidates: nothing to do, whatever the pointers
        prim.score_trajectory_chained_dev(traj, d_S, S.dtype, 0, L, None, TEMPLATE, d_e)
        assert (ctx.download(d_e, (B,), np.uint64) == SENTINEL).all()
    finally:
        for b in (d_S, d_A, d_e):
            b.free()


def test_every_single_launch_kernel_ran():
    """Runs last: each of the five single-launch kernels scored a chained batch above and matched."""
    missing = SINGLE_LAUNCH_KERNELS - LEDGER
    assert not missing, sorted(missing)
