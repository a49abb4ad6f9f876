"""The device DTW (mg_dtw_distance_grids, mg_dtw_paths, mg_warp_motions and morphablegraphs_amd.dtw) against the reference's
construction/dtw.py as recorded in tests/golden/dtw.npz.  From given grids everything is bit-exact; the grids follow the
parity rule of tests/test_dtw_host.py."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dtw_host import GOLDEN, GRIDS, MOTIONS, POINT, all_grid_cases, check_grid, end_to_end, grid_bound, grid_case, point_case, same_bits  # noqa: E402

from morphablegraphs_amd import _capi, dtw  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from morphablegraphs_amd.motion_primitive import get_context
    return get_context(0)


def point_set(s):
    cases = [point_case(s, k) for k in range(int(GOLDEN["p%d_n" % s]))]
    return cases, (None if s == 0 else cases[0]["weights"])


def check_paths(result, c):
    assert same_bits(result["D"], c["D"]), c["name"]
    assert same_bits(result["total"], c["D"][-1, -1]), c["name"]
    assert np.array_equal(result["path"], c["path"]) and result["path"].dtype == np.int32, c["name"]
    assert np.array_equal(result["warping_function"], c["warp"]), c["name"]


def test_paths_from_golden_grids_are_the_reference_bit_for_bit(ctx):
    """Every golden grid, ties included; batched by the reference motion's length, alone, and twice."""
    cases = all_grid_cases()
    by_rows = collections.OrderedDict()
    for c in cases:
        by_rows.setdefault(c["S"].shape[0], []).append(c)
    assert any(len(v) > 1 for v in by_rows.values())
    for group in by_rows.values():
        batch = dtw.paths_from_grids([c["S"] for c in group], ctx=ctx)
        again = dtw.paths_from_grids([c["S"] for c in group], ctx=ctx)
        for c, r, r2 in zip(group, batch, again):
            check_paths(r, c)
            alone = dtw.paths_from_grids([c["S"]], ctx=ctx)[0]
            for other in (r2, alone):
                assert same_bits(other["D"], r["D"]) and np.array_equal(other["path"], r["path"]) and other["total"] == r["total"]
                assert np.array_equal(other["warping_function"], r["warping_function"])
            skipped = dtw.paths_from_grids([c["S"]], accumulated=False, ctx=ctx)[0]
            assert skipped["D"] is None and np.array_equal(skipped["path"], c["path"]) and same_bits(skipped["total"], c["D"][-1, -1])


@pytest.mark.parametrize("s", range(int(GOLDEN["n_point_sets"])))
def test_distance_grids_against_the_restatement(ctx, s):
    """|ours - golden| <= 10 * max(spread, 1e-13 * max|S|) per motion; a motion alone gives the bits of the batch."""
    cases, weights = point_set(s)
    grids = dtw.distance_grids(cases[0]["ref"], [c["cloud"] for c in cases], weights, ctx=ctx)
    again = dtw.distance_grids(cases[0]["ref"], [c["cloud"] for c in cases], weights, ctx=ctx)
    worst = 0.0
    for c, S, S2 in zip(cases, grids, again):
        worst = max(worst, check_grid(c["name"], S, c))
        assert same_bits(S, S2)
        assert same_bits(dtw.distance_grids(c["ref"], [c["cloud"]], weights, ctx=ctx)[0], S)
        host = dtw.distance_grid_host(c["ref"], c["cloud"], weights)
        print("%s: max |device - host restatement| %.3g" % (c["name"], float(np.max(np.abs(S - host)))))
    print("set %d: worst error / bound %.3g" % (s, worst))


@pytest.mark.parametrize("s", range(int(GOLDEN["n_point_sets"])))
def test_no_nearby_angle_fits_better(ctx, s):
    """The property the restatement itself is tested by: at sampled cells the device's distance is that of a rotation no
    nearby angle improves on.  For a rotation theta' the best translation moves the weighted centroids onto each other, so
    the weighted squared residual is a function of theta' alone; it is scanned around the optimum (closed form, from the
    clouds) and the mean distance at the scan's best angle must reproduce the device's cell within the grid's bound."""
    cases, weights = point_set(s)
    rng = np.random.default_rng(11 + s)
    grids = dtw.distance_grids(cases[0]["ref"], [c["cloud"] for c in cases], weights, ctx=ctx)
    for c, S in zip(cases, grids):
        w = np.ones(c["ref"].shape[1]) if weights is None else weights
        for _ in range(6):
            i, j = int(rng.integers(S.shape[0])), int(rng.integers(S.shape[1]))
            a, b = c["ref"][i], c["cloud"][j]
            ca, cb = (w[:, None] * a).sum(0) / w.sum(), (w[:, None] * b).sum(0) / w.sum()
            pa, pb = a - ca, b - cb
            theta0 = np.arctan2((w * (pa[:, 0] * pb[:, 2] - pb[:, 0] * pa[:, 2])).sum(), (w * (pa[:, 0] * pb[:, 0] + pa[:, 2] * pb[:, 2])).sum())

            def fitted(theta):
                out = pb.copy()
                out[:, 0] = pb[:, 0] * np.cos(theta) + pb[:, 2] * np.sin(theta)
                out[:, 2] = -pb[:, 0] * np.sin(theta) + pb[:, 2] * np.cos(theta)
                return out

            def residual(theta):
                d = pa - fitted(theta)
                return float((w * (d[:, 0] ** 2 + d[:, 2] ** 2)).sum())
            scan = theta0 + np.linspace(-0.05, 0.05, 2001)
            best = scan[int(np.argmin([residual(t) for t in scan]))]
            assert abs(best - theta0) <= 1e-4 and residual(theta0) <= residual(best) * (1 + 1e-12) + 1e-300
            d = pa - fitted(theta0)
            d[:, 1] = a[:, 1] - b[:, 1]
            mean_distance = float(np.sqrt((d ** 2).sum(1)).sum() / len(a))
            assert abs(S[i, j] - mean_distance) <= max(grid_bound(c), 1e-12 * max(1.0, float(np.max(np.abs(a))), float(np.max(np.abs(b))))), (c["name"], i, j)


@pytest.mark.parametrize("s", range(int(GOLDEN["n_point_sets"])))
def test_end_to_end_from_clouds(ctx, s):
    """Paths equal the golden paths on every kept case (what the generator's gap condition buys); the total cost lies
    within (Fr + F) times the bound of the grid."""
    cases, weights = point_set(s)
    results = dtw.dtw_batch(cases[0]["ref"], [c["cloud"] for c in cases], weights, accumulated=True, ctx=ctx)
    for c, r in zip(cases, results):
        assert np.array_equal(r["path"], c["path"]), c["name"]
        assert np.array_equal(r["warping_function"], c["warp"]), c["name"]
        err, bound = abs(r["total"] - c["D"][-1, -1]), sum(c["S"].shape) * grid_bound(c)
        print("%s: |total - golden| %.3g, bound %.3g" % (c["name"], err, bound))
        assert err <= bound, c["name"]
    if s == 0:
        c = cases[0]
        path, D = dtw.run_dtw(c["ref"], c["cloud"], ctx=ctx)
        assert path == [tuple(int(v) for v in p) for p in c["path"]] and same_bits(D, results[0]["D"])
        clouds = collections.OrderedDict([("ref", c["ref"])] + [("m%d" % k, x["cloud"]) for k, x in enumerate(cases)])
        paths = dtw.find_optimal_dtw(clouds, "ref", ctx=ctx)
        assert list(paths.keys()) == list(clouds.keys()) and paths["ref"] == [(i, i) for i in range(len(c["ref"]))]
        for k, x in enumerate(cases):
            assert paths["m%d" % k] == [tuple(int(v) for v in p) for p in x["path"]]
        with pytest.raises(KeyError):
            dtw.find_optimal_dtw(clouds, None, ctx=ctx)


def brute_force_dp(S):
    D = np.zeros_like(S)
    for i in range(S.shape[0]):
        for j in range(S.shape[1]):
            prev = [D[a, b] for a, b in ((i - 1, j - 1), (i - 1, j), (i, j - 1)) if a >= 0 and b >= 0]
            D[i, j] = (min(prev) if prev else 0.0) + S[i, j]
    return D


def test_optimality_on_random_grids(ctx):
    """Independent of any restatement: the device's total is a brute-force NumPy recurrence's, the path's cells add up to
    it, and no random monotone path is cheaper."""
    rng = np.random.default_rng(3)
    fr = 37
    grids = [rng.uniform(0.0, 1.0, (fr, f)) ** 3 for f in (5, 37, 64, 90)]
    for S, r in zip(grids, dtw.paths_from_grids(grids, ctx=ctx)):
        D = brute_force_dp(S)
        assert same_bits(r["D"], D) and r["total"] == D[-1, -1]
        path = r["path"]
        assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (fr - 1, S.shape[1] - 1)
        steps = np.diff(path, axis=0)
        assert np.all((steps >= 0) & (steps <= 1)) and np.all(steps.sum(1) >= 1)
        assert abs(S[path[:, 0], path[:, 1]].sum() - r["total"]) <= 1e-12 * r["total"]
        for _ in range(100):
            i = j = 0
            cost = S[0, 0]
            while (i, j) != (fr - 1, S.shape[1] - 1):
                moves = [(a, b) for a, b in ((i + 1, j + 1), (i + 1, j), (i, j + 1)) if a < fr and b < S.shape[1]]
                i, j = moves[int(rng.integers(len(moves)))]
                cost += S[i, j]
            assert r["total"] <= cost


def test_large_grids_keep_their_back_steps_in_device_memory(ctx):
    """1024 x 1000: the back-step codes no longer fit the LDS; same recurrence, same rule."""
    rng = np.random.default_rng(5)
    grids = [np.floor(rng.uniform(0.0, 4.0, (1024, f))) for f in (1000, 333)]
    for S, r in zip(grids, dtw.paths_from_grids(grids, ctx=ctx)):
        D, path, warp = dtw.dtw_paths_host(S)
        assert same_bits(r["D"], D) and [tuple(int(v) for v in p) for p in r["path"]] == path and r["warping_function"].tolist() == warp


def skeleton_and_motions():
    joints, animated, keys, motions = end_to_end()
    return _capi.Skeleton(joints, animated), [j[0] for j in joints], keys, motions


class _OneGaussian(object):
    """A stand-in trainer (six motions are too few for the AIC sweep): one component with a diagonal covariance."""

    def fit(self, data):
        self.data = np.array(data)

    def convert_model_to_json(self):
        return {'gmm_weights': [1.0], 'gmm_means': [self.data.mean(axis=0).tolist()], 'gmm_covars': [np.diag(self.data.var(axis=0) + 1e-6).tolist()]}


def test_align_frames_temporally(ctx):
    from morphablegraphs_amd import fpca
    from morphablegraphs_amd.motion_primitive import HipMotionPrimitive
    sk, names, keys, motions = skeleton_and_motions()
    warped, warps = dtw.align_frames_temporally(sk, names, motions, ctx=ctx)
    assert isinstance(warped, collections.OrderedDict) and isinstance(warps, collections.OrderedDict)
    assert list(warped.keys()) == keys and list(warps.keys()) == keys
    fr = len(motions[str(GOLDEN["e_mean_key"])])
    for i in MOTIONS:
        k = keys[i]
        assert warped[k].shape == (fr, motions[k].shape[1]) and len(warps[k]) == fr
        assert warps[k] == GOLDEN["e_m%d_warp" % i].tolist(), k
        assert same_bits(warped[k], GOLDEN["e_m%d_warped" % i]), k
    explicit = dtw.align_frames_temporally(sk, names, motions, mean_key=str(GOLDEN["e_mean_key"]), ctx=ctx)
    assert all(same_bits(explicit[0][k], warped[k]) and explicit[1][k] == warps[k] for k in keys)
    config = {"n_spatial_basis_factor": 0.25, "n_components": None, "fraction": 0.95, "n_basis_functions_temporal": 8, "npc_temporal": None,
              "precision_temporal": 0.99}
    data = fpca.construct_motion_primitive_model(warped, warps, config, animated_joints=[str(a) for a in GOLDEN["e_animated_joints"]], name="walk",
                                                 version=1, frame_time=1.0 / 30, gmm_trainer=_OneGaussian(), ctx=ctx)
    prim = HipMotionPrimitive(context=ctx)
    prim._initialize_from_json(data)
    assert data["n_canonical_frames"] == fr and prim.get_n_spatial_components() == len(data["eigen_vectors_spatial"])


def test_align_frames_temporally_in_sections(ctx):
    sk, names, keys, motions = skeleton_and_motions()
    sections = {k: [{"start_idx": 0, "end_idx": len(m) // 2}, {"start_idx": len(m) // 2, "end_idx": len(m)}] for k, m in motions.items()}
    mean_key = dtw.get_average_time_line(motions)
    warped, warps = dtw.align_frames_temporally(sk, names, motions, sections=sections, ctx=ctx)
    parts = []
    for s in range(2):
        part = collections.OrderedDict((k, m[sections[k][s]["start_idx"]:sections[k][s]["end_idx"]]) for k, m in motions.items())
        parts.append(dtw.align_frames_temporally(sk, names, part, mean_key=mean_key, ctx=ctx))
    assert list(warped.keys()) == keys
    for k in keys:
        assert same_bits(warped[k], np.concatenate([p[0][k] for p in parts]))
        assert warps[k] == parts[0][1][k] + parts[1][1][k] and len(warps[k]) == len(motions[mean_key])


def status_of(call):
    with pytest.raises(_capi.MGError) as ei:
        call()
    return ei.value.status


def test_limits_and_misuse(ctx):
    """The documented status, before any DTW kernel is launched; nothing here can fault."""
    J = 3
    off = lambda *lengths: np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)      # noqa: E731
    big = ctx.upload(np.zeros((1030, 65, 3)))
    out = ctx.malloc(8 * 1030 * 1030)
    ints = ctx.malloc(8 * 4200)
    try:
        grids = lambda fr, o, j=J: _capi.dtw_distance_grids(ctx, big, fr, big, o, j, None, out)      # noqa: E731
        paths = lambda fr, o: _capi.dtw_paths(ctx, big, fr, o, None, out, ints, ints, ints)      # noqa: E731
        warp = lambda fr, o: _capi.warp_motions(ctx, big, o, 3, ints, fr, out)      # noqa: E731
        for call in (grids, paths, warp):
            assert status_of(lambda: call(1025, off(4))) == _capi.MG_ERR_UNSUPPORTED
            assert status_of(lambda: call(4, off(4, 1025))) == _capi.MG_ERR_UNSUPPORTED
            assert status_of(lambda: call(4, np.array([1, 5], dtype=np.int64))) == _capi.MG_ERR_INVALID_ARGUMENT
            assert status_of(lambda: call(4, np.array([0, 5, 5], dtype=np.int64))) == _capi.MG_ERR_INVALID_ARGUMENT
            assert status_of(lambda: call(4, np.array([0, 5, 3], dtype=np.int64))) == _capi.MG_ERR_INVALID_ARGUMENT
            assert status_of(lambda: call(0, off(4))) == _capi.MG_ERR_INVALID_ARGUMENT
            call(4, off())        # no motions: MG_OK, nothing to do
        assert status_of(lambda: grids(4, off(4), 65)) == _capi.MG_ERR_UNSUPPORTED
        assert status_of(lambda: grids(4, off(4), 0)) == _capi.MG_ERR_INVALID_ARGUMENT
        assert status_of(lambda: _capi.dtw_distance_grids(ctx, big, 4, big, off(4), J, [1.0, -1.0, 1.0], out)) == _capi.MG_ERR_INVALID_ARGUMENT
        with pytest.raises(ValueError):
            _capi.dtw_distance_grids(ctx, big, 4, big, off(4), J, [1.0, 1.0], out)
        grids(1024, off(1024, 1), 64)       # the limits themselves are supported (their values: test_gpu_construction_shapes.py)
        # a NaN in the clouds, an infinity in a grid
        bad = np.zeros((9, J, 3))
        bad[7, 1, 2] = np.nan
        b_dev = ctx.upload(bad)
        try:
            assert status_of(lambda: _capi.dtw_distance_grids(ctx, big, 4, b_dev, off(4, 5), J, None, out)) == _capi.MG_ERR_INVALID_ARGUMENT
            assert status_of(lambda: _capi.dtw_distance_grids(ctx, b_dev, 9, big, off(4), J, None, out)) == _capi.MG_ERR_INVALID_ARGUMENT
        finally:
            b_dev.free()
        g = np.ones((4, 6))
        g[3, 5] = np.inf
        g_dev = ctx.upload(g)
        try:
            assert status_of(lambda: _capi.dtw_paths(ctx, g_dev, 4, off(6), None, out, ints, ints, ints)) == _capi.MG_ERR_INVALID_ARGUMENT
        finally:
            g_dev.free()
        # a warping function that points outside its motion: refused, nothing read for it
        w_dev = ctx.upload(np.array([0, 1, 4, 2], dtype=np.int32))
        try:
            assert status_of(lambda: _capi.warp_motions(ctx, big, off(4), 3, w_dev, 4, out)) == _capi.MG_ERR_INVALID_ARGUMENT
        finally:
            w_dev.free()
    finally:
        for b in (big, out, ints):
            b.free()
    with pytest.raises(ValueError):
        dtw.paths_from_grids([np.ones((4, 1025))], ctx=ctx)
    with pytest.raises(ValueError):
        dtw.distance_grids(np.zeros((4, 65, 3)), [np.zeros((4, 65, 3))], ctx=ctx)
    assert dtw.paths_from_grids([], ctx=ctx) == [] and dtw.distance_grids(np.zeros((4, 2, 3)), [], ctx=ctx) == []
