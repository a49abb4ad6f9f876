"""The all-pairs DTW costs on the device (mg_dtw_pair_costs, dtw.all_pairs_costs, dtw.select_reference_motion and
align_frames_temporally's reference_selection).  The pin is the project's own pairwise path: costs[r][n] has the bits of
dtw.dtw_batch(clouds[r], clouds)[n]["total"] (mg_dtw_distance_grids + mg_dtw_paths), which tests/test_gpu_dtw.py pins to the
reference."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dtw_host import GOLDEN, MARGIN, FLOOR, end_to_end, same_bits  # noqa: E402
from test_dtw_pairs_host import point_table  # noqa: E402

from morphablegraphs_amd import _capi, dtw  # noqa: E402

pytestmark = pytest.mark.gpu

# the kernel's own shape constants (csrc/mg_dtw_pairs.hip)
STRIP = 64           # PAIRS_STRIP: columns of a strip, the lanes of the recurrence's wave (= the wave size)
SUB = 16             # PAIRS_SUB: rows of the reference motion staged at a time
WAVES = 8            # PAIRS_WAVES: a 16-row step gives each wave rows w and w + 8
PASS_ROWS = (64, 32)   # rows of a pass: PAIRS_PASS_ROWS at J = 1 and 19, halved at J = 64 (the LDS limit)
ISSUE_LENGTHS = [1, 2, 15, 16, 17, 33, 63, 64, 65, 130]
BOUNDARY_LENGTHS = [WAVES - 1, WAVES, WAVES + 1, PASS_ROWS[1] - 1, PASS_ROWS[1], 2 * STRIP - 1, 2 * STRIP, 2 * STRIP + 1]
SWEEP_LENGTHS = ISSUE_LENGTHS + BOUNDARY_LENGTHS      # SUB +- 1, PASS_ROWS[1] + 1, STRIP +- 1 and PASS_ROWS[0] +- 1 are in the issue's list


@pytest.fixture(scope="module")
def ctx():
    from morphablegraphs_amd.motion_primitive import get_context
    return get_context(0)


def pairwise(ctx, table, weights, references=None):
    """The matrix as the parent commit can produce it: one dtw_batch per reference motion, reading `total`."""
    refs = range(len(table)) if references is None else references
    return np.array([[r["total"] for r in dtw.dtw_batch(table[m], table, weights, ctx=ctx)] for m in refs])


def synthetic_clouds(J, lengths, seed):
    """Seeded clouds: one random pose, drifting, turning about y and jittering over the frames."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((J, 3)) * np.array([30.0, 60.0, 30.0])
    out = []
    for F in lengths:
        t = np.linspace(0.0, 1.0, F)[:, None, None]
        ang = (rng.uniform(-1.5, 1.5) * t[:, :, 0] + rng.uniform(-3.0, 3.0))
        cloud = base[None] + 8.0 * rng.standard_normal((F, J, 3)) + t * rng.standard_normal((1, 1, 3)) * 50.0
        x, z = cloud[:, :, 0].copy(), cloud[:, :, 2].copy()
        cloud[:, :, 0], cloud[:, :, 2] = x * np.cos(ang) + z * np.sin(ang), -x * np.sin(ang) + z * np.cos(ang)
        out.append(np.ascontiguousarray(cloud))
    return out


def test_the_sweep_straddles_the_kernels_boundaries():
    for edge in (SUB, WAVES, STRIP, 2 * STRIP) + PASS_ROWS:
        assert {edge - 1, edge, edge + 1} <= set(SWEEP_LENGTHS), edge
    assert len(SWEEP_LENGTHS) == len(set(SWEEP_LENGTHS))


@pytest.mark.parametrize("s", range(int(GOLDEN["n_point_sets"])))
def test_golden_point_sets_in_bits(ctx, s):
    """The device matrix is the pairwise path's in bits, row by row; twice; a choice of rows; every pair alone."""
    _, table, weights = point_table(s)
    costs = dtw.all_pairs_costs(table, weights, ctx=ctx)
    assert costs.shape == (len(table), len(table)) and costs.dtype == np.float64
    assert same_bits(costs, pairwise(ctx, table, weights))
    assert costs.tobytes() == dtw.all_pairs_costs(table, weights, ctx=ctx).tobytes()
    assert same_bits(dtw.all_pairs_costs(table, weights, references=[2, 0], ctx=ctx), costs[[2, 0]])
    for r in range(len(table)):
        for n in range(len(table)):
            alone = dtw.all_pairs_costs([table[r], table[n]], weights, references=[0], ctx=ctx)
            assert same_bits(alone[0, 1], costs[r, n]), (r, n)
    host = dtw.all_pairs_costs_host(table, weights)
    print("set %d: max |device - all_pairs_costs_host| %.3g (largest cost %.3g)" % (s, float(np.max(np.abs(costs - host))), float(costs.max())))


@pytest.mark.parametrize("J", [1, 19, 64])
def test_shape_sweep_in_bits(ctx, J):
    """Motions of every length around the strip (64, 128), the 16-row step, the waves' row pairs (8) and the pass (64 rows; 32 at
    J = 64) in one table, every one a reference motion and a motion; non-uniform weights at J = 19.  At J = 19 also against the
    host restatement: |device - host| <= (Fr + F) x 10 max(spread, 1e-13 max|S|), the grid rule of tests/test_dtw_host.py
    scaled by the number of cells a path can add up; spread (the restatement's own change over 3 joint permutations) is
    computed for a motion against itself, whose grid's diagonal is all rounding, and taken as 0 elsewhere (a smaller bound)."""
    table = synthetic_clouds(J, SWEEP_LENGTHS, 100 + J)
    weights = np.random.default_rng(7).uniform(0.2, 2.0, J) if J == 19 else None
    costs = dtw.all_pairs_costs(table, weights, ctx=ctx)
    assert same_bits(costs, pairwise(ctx, table, weights))
    picked = [len(table) - 1, 0, 9]
    assert same_bits(dtw.all_pairs_costs(table, weights, references=picked, ctx=ctx), costs[picked])
    if J != 19:
        return
    host = dtw.all_pairs_costs_host(table, weights)
    rng = np.random.default_rng(8)
    worst = 0.0
    for r, a in enumerate(table):
        for n, b in enumerate(table):
            S = dtw.distance_grid_host(a, b, weights)
            spread = 0.0
            if r == n:
                for _ in range(3):
                    perm = rng.permutation(J)
                    spread = max(spread, float(np.max(np.abs(dtw.distance_grid_host(a[:, perm], b[:, perm], weights[perm]) - S))))
            bound = (len(a) + len(b)) * MARGIN * max(spread, FLOOR * float(np.max(np.abs(S))))
            err = abs(costs[r, n] - host[r, n])
            worst = max(worst, err / bound)
            assert err <= bound, (r, n, err, bound)
    print("J = 19: worst |device - host| / bound %.3g, max |device - host| %.3g" % (worst, float(np.max(np.abs(costs - host)))))


def test_the_limits_in_bits(ctx):
    """1024 and 1000 frames at J = 64: the 32-row pass, the largest LDS request, 16 strips; all four pairs."""
    table = synthetic_clouds(64, [1024, 1000], 5)
    costs = dtw.all_pairs_costs(table, ctx=ctx)
    assert same_bits(costs, pairwise(ctx, table, None))
    assert np.all(np.isfinite(costs)) and costs[0, 1] > 0.0


def test_ties_follow_pythons_min(ctx):
    """J = 1 with x = z = 0 and small integer y: num = den = 0, the fit is the identity, S[i][j] = |a_i - b_j| exactly, and the
    grids are full of ties; the totals are dtw_paths_host's.  One-frame motions make the first-row-only (1 x F) and
    first-column-only (F x 1) optima."""
    rng = np.random.default_rng(21)
    ys = [np.floor(rng.uniform(0.0, 4.0, F)) for F in (1, 1, 5, STRIP, STRIP + 6, 2 * STRIP + 2)]
    ys[1][0] = ys[0][0] + 2.0
    table = [np.stack([np.zeros(len(y)), y, np.zeros(len(y))], axis=1)[:, None, :] for y in ys]
    costs = dtw.all_pairs_costs(table, ctx=ctx)
    want = np.array([[dtw.dtw_paths_host(np.abs(a[:, None] - b[None, :]))[0][-1, -1] for b in ys] for a in ys])
    assert same_bits(costs, want)
    assert costs[0, 5] == float(np.abs(ys[0][0] - ys[5]).sum()) and costs[5, 0] == costs[0, 5]     # 1 x F and F x 1
    assert same_bits(costs, pairwise(ctx, table, None))


def status_of(call):
    with pytest.raises(_capi.MGError) as ei:
        call()
    return ei.value.status


def test_limits_and_misuse_are_refused_on_the_host(ctx):
    """The documented status for everything the host can see, before any launch; a NaN through the check kernel.  Nothing
    here can fault, and a good call on the same context succeeds after each refusal."""
    J = 3
    off = lambda *lengths: np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)      # noqa: E731
    good = synthetic_clouds(J, [4, 6], 3)
    want = pairwise(ctx, good, None)
    g_dev, big, out = ctx.upload(np.concatenate(good)), ctx.upload(np.zeros((1030, 65, 3))), ctx.malloc(8 * 16)
    bad = np.zeros((9, J, 3))
    bad[7, 1, 2] = np.nan
    b_dev = ctx.upload(bad)
    try:
        def good_call():
            ctx.upload_into(out, np.zeros(16))
            assert _capi.dtw_pair_costs(ctx, g_dev, off(4, 6), J, None, None, out) == 2
            assert same_bits(ctx.download(out, (2, 2), np.float64), want)

        good_call()
        refusals = [
            (lambda: _capi.dtw_pair_costs(ctx, big, off(4, 5), 65, None, None, out), _capi.MG_ERR_UNSUPPORTED),
            (lambda: _capi.dtw_pair_costs(ctx, big, off(4, 1025), J, None, None, out), _capi.MG_ERR_UNSUPPORTED),
            (lambda: _capi.dtw_pair_costs(ctx, big, off(4, 5), J, None, [0, 2], out), _capi.MG_ERR_INVALID_ARGUMENT),
            (lambda: _capi.dtw_pair_costs(ctx, big, off(4, 5), J, None, [-1], out), _capi.MG_ERR_INVALID_ARGUMENT),
            (lambda: _capi.dtw_pair_costs(ctx, b_dev, off(4, 5), J, None, None, out), _capi.MG_ERR_INVALID_ARGUMENT),
            (lambda: _capi.dtw_pair_costs(ctx, big, np.array([0, 5, 5], dtype=np.int64), J, None, None, out), _capi.MG_ERR_INVALID_ARGUMENT),
            (lambda: _capi.dtw_pair_costs(ctx, big, np.array([1, 5], dtype=np.int64), J, None, None, out), _capi.MG_ERR_INVALID_ARGUMENT),
            (lambda: _capi.dtw_pair_costs(ctx, big, off(4, 5), 0, None, None, out), _capi.MG_ERR_INVALID_ARGUMENT),
            (lambda: _capi.dtw_pair_costs(ctx, big, off(4, 5), J, [1.0, -1.0, 1.0], None, out), _capi.MG_ERR_INVALID_ARGUMENT),
        ]
        for call, status in refusals:
            assert status_of(call) == status
            good_call()
        # no motions, no reference motions: MG_OK, nothing written
        marks = np.arange(16.0)
        ctx.upload_into(out, marks)
        assert _capi.dtw_pair_costs(ctx, big, off(), J, None, None, out) == 0
        assert _capi.dtw_pair_costs(ctx, big, off(4, 5), J, None, [], out) == 0
        assert np.array_equal(ctx.download(out, (16,), np.float64), marks)
        good_call()
    finally:
        for b in (g_dev, big, out, b_dev):
            b.free()
    assert dtw.all_pairs_costs([], ctx=ctx).shape == (0, 0)
    assert dtw.all_pairs_costs(good, references=[], ctx=ctx).shape == (0, 2)
    with pytest.raises(ValueError):
        dtw.all_pairs_costs(good, references=[2], ctx=ctx)
    with pytest.raises(ValueError):
        dtw.all_pairs_costs([np.zeros((1025, J, 3))], ctx=ctx)


def test_reference_selection_end_to_end(ctx):
    """The golden quaternion motions (6 of 30 .. 44 frames, a 7-joint skeleton)."""
    joints, animated, keys, motions = end_to_end()
    sk, names = _capi.Skeleton(joints, animated), [j[0] for j in joints]
    clouds = [ctx.joint_positions(sk, names, motions[k]) for k in keys]
    costs = dtw.all_pairs_costs(clouds, ctx=ctx)
    want_key, want_means = dtw.reference_from_costs(costs, keys)
    key, means = dtw.select_reference_motion(sk, names, motions, ctx=ctx)
    assert key == want_key and isinstance(means, collections.OrderedDict) and list(means.keys()) == keys
    assert same_bits(list(means.values()), want_means)
    print("mean costs %s -> %r (get_average_time_line: %r)" % (["%.4g" % v for v in means.values()], key, dtw.get_average_time_line(motions)))
    # restricted to two candidates: the better of the two, from the same rows
    two = [keys[4], keys[1]]
    key2, means2 = dtw.select_reference_motion(sk, names, motions, candidates=two, ctx=ctx)
    assert list(means2.keys()) == two and same_bits(list(means2.values()), want_means[[4, 1]])
    assert key2 == (two[0] if want_means[4] <= want_means[1] else two[1])
    with pytest.raises(KeyError):
        dtw.select_reference_motion(sk, names, motions, candidates=["no such motion"], ctx=ctx)
    # align_frames_temporally: the new selection is the call with that key, whole and in sections; the default is unchanged
    sections = {k: [{"start_idx": 0, "end_idx": len(m) // 2}, {"start_idx": len(m) // 2, "end_idx": len(m)}] for k, m in motions.items()}
    for sec in (None, sections):
        selected = dtw.align_frames_temporally(sk, names, motions, sections=sec, reference_selection="least_mean_cost", ctx=ctx)
        explicit = dtw.align_frames_temporally(sk, names, motions, mean_key=want_key, sections=sec, ctx=ctx)
        default = dtw.align_frames_temporally(sk, names, motions, sections=sec, ctx=ctx)
        average = dtw.align_frames_temporally(sk, names, motions, mean_key=dtw.get_average_time_line(motions), sections=sec, ctx=ctx)
        for got, want in ((selected, explicit), (default, average)):
            assert list(got[0].keys()) == keys and list(got[1].keys()) == keys
            assert all(same_bits(got[0][k], want[0][k]) and got[1][k] == want[1][k] for k in keys)
    # an explicit mean_key wins over the selection; an unknown selection is refused
    forced = dtw.align_frames_temporally(sk, names, motions, mean_key=keys[0], reference_selection="least_mean_cost", ctx=ctx)
    assert len(forced[1][keys[1]]) == len(motions[keys[0]])
    with pytest.raises(ValueError):
        dtw.align_frames_temporally(sk, names, motions, reference_selection="shortest", ctx=ctx)
