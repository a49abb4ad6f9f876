"""The device segmentation (mg_keyframe_distances, mg_segment_search and morphablegraphs_amd.segmentation) against the
reference's construction/keyframe_detection.py and segmentation.py as recorded in tests/golden/segmentation.npz.  From given
distances everything is exact; the distances follow the parity rule of tests/test_dtw_host.py and are, in bits, cells of the
DTW grids."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dtw_host import same_bits  # noqa: E402
from test_segmentation_host import GOLDEN, all_search_cases, check_distances, end_to_end, point_case, weights_of  # noqa: E402

from morphablegraphs_amd import _capi, dtw  # noqa: E402
from morphablegraphs_amd import segmentation as seg  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from morphablegraphs_amd.motion_primitive import get_context
    return get_context(0)


def point_set(s):
    cases = [point_case(s, k) for k in range(int(GOLDEN["p%d_n" % s]))]
    return cases, weights_of(s, cases[0]), np.stack([cases[0]["start"], cases[0]["end"]])


def same_pairs(ours, golden):
    golden = golden.reshape(-1, 2)
    return ours.dtype == np.int32 and ours.shape == golden.shape and np.array_equal(ours, golden)


def test_search_on_golden_distances_is_the_reference(ctx):
    """Every golden case, ties included, both modes and every setting; batched per setting, alone, and twice."""
    cases = all_search_cases()
    by_setting = collections.OrderedDict()
    for c in cases:
        for j, setting in enumerate(c["settings"]):
            by_setting.setdefault(setting, []).append((c, j))
    assert any(len(v) > 1 for v in by_setting.values())
    singles = seg.segment_search([c["S"] for c in cases], [c["E"] for c in cases], seg.SINGLE, ctx=ctx)
    for c, r in zip(cases, singles):
        assert same_pairs(r, c["single"]), c["name"]
        assert np.array_equal(seg.segment_search([c["S"]], [c["E"]], seg.SINGLE, ctx=ctx)[0], r)
    for (threshold, min_size), group in by_setting.items():
        args = ([c["S"] for c, _ in group], [c["E"] for c, _ in group], seg.MULTI, threshold, min_size)
        batch, again = seg.segment_search(*args, ctx=ctx), seg.segment_search(*args, ctx=ctx)
        for (c, j), r, r2 in zip(group, batch, again):
            assert same_pairs(r, c["multi"][j]), (c["name"], threshold, min_size)
            alone = seg.segment_search([c["S"]], [c["E"]], seg.MULTI, threshold, min_size, ctx=ctx)[0]
            assert r2.tobytes() == r.tobytes() and alone.tobytes() == r.tobytes()
            assert [tuple(int(v) for v in p) for p in r] == seg.segment_search_host(c["S"], c["E"], seg.MULTI, threshold, min_size)


def test_search_on_long_tied_distances(ctx):
    """Captures far beyond 1024 frames with many instances (more than one compaction step, more than one wave's share),
    against the host restatement."""
    rng = np.random.default_rng(17)
    starts = [np.floor(rng.uniform(0.0, 6.0, f)) for f in (5000, 257, 256, 12345, 64, 65)]
    ends = [np.floor(rng.uniform(0.0, 50.0, len(s))) for s in starts]
    for threshold, min_size in ((0.0, 0), (0.0, 3), (1.0, 1), (5.0, 0), (0.5, 7)):
        results = seg.segment_search(starts, ends, seg.MULTI, threshold, min_size, ctx=ctx)
        for s, e, r in zip(starts, ends, results):
            assert [tuple(int(v) for v in p) for p in r] == seg.segment_search_host(s, e, seg.MULTI, threshold, min_size)
    for s, e, r in zip(starts, ends, seg.segment_search(starts, ends, seg.SINGLE, ctx=ctx)):
        assert r.tolist() == [[int(np.argmin(s)), int(np.argmin(e))]]


@pytest.mark.parametrize("s", range(int(GOLDEN["n_point_sets"])))
def test_keyframe_distances_against_the_restatement(ctx, s):
    """|ours - golden| <= 10 * max(spread, 1e-13 * max|S|) per capture and keyframe; a capture alone and a second call give
    the bits of the batch; K keyframes in one call give the bits of K calls of one keyframe."""
    cases, weights, keys = point_set(s)
    clouds = [c["cloud"] for c in cases]
    dist = seg.keyframe_distances(clouds, keys, weights, ctx=ctx)
    again = seg.keyframe_distances(clouds, keys, weights, ctx=ctx)
    one_by_one = [seg.keyframe_distances(clouds, keys[k:k + 1], weights, ctx=ctx) for k in range(len(keys))]
    many = np.concatenate([keys, keys[::-1], keys, keys])       # 8 keyframes in one call
    eight = seg.keyframe_distances(clouds, many, weights, ctx=ctx)
    worst = 0.0
    for n, (c, d, d2) in enumerate(zip(cases, dist, again)):
        assert d.shape == (2, len(c["cloud"]))
        worst = max(worst, check_distances(c["name"], d, c))
        assert same_bits(d, d2)
        assert same_bits(seg.keyframe_distances([c["cloud"]], keys, weights, ctx=ctx)[0], d)
        for k in range(len(keys)):
            assert same_bits(one_by_one[k][n][0], d[k])
        assert same_bits(eight[n], np.concatenate([d, d[::-1], d, d]))
        host = seg.keyframe_distances_host([c["cloud"]], keys, weights)[0]
        print("%s: max |device - host restatement| %.3g" % (c["name"], float(np.max(np.abs(d - host)))))
    print("set %d: worst error / bound %.3g" % (s, worst))


@pytest.mark.parametrize("s", range(int(GOLDEN["n_point_sets"])))
def test_keyframe_distances_are_cells_of_the_dtw_grids(ctx, s):
    """For the captures the DTW kernel takes (at most 1024 frames): bit-identical to column 0 of the grid of (reference motion
    = the capture, one motion = the one-frame keyframe)."""
    cases, weights, keys = point_set(s)
    short = [c for c in cases if len(c["cloud"]) <= dtw.MAX_FRAMES]
    assert short
    dist = seg.keyframe_distances([c["cloud"] for c in short], keys, weights, ctx=ctx)
    for c, d in zip(short, dist):
        for k in range(len(keys)):
            grid = dtw.distance_grids(c["cloud"], [keys[k][None]], weights, ctx=ctx)[0]
            assert grid.shape == (len(c["cloud"]), 1) and same_bits(d[k], grid[:, 0]), (c["name"], k)


@pytest.mark.parametrize("s", range(int(GOLDEN["n_point_sets"])))
def test_end_to_end_from_clouds(ctx, s):
    """Every segment list equals the golden one (what the generator's margin condition buys), all captures in one call."""
    cases, weights, keys = point_set(s)
    clouds = [c["cloud"] for c in cases]
    for j, (threshold, min_size) in enumerate(cases[0]["settings"]):
        sg = seg.Segmentation(None, None, min_size, ctx=ctx, weights=weights)
        triples = sg.segment_indices(clouds, keys[0], keys[1], threshold)
        assert triples == [(n, int(a), int(b)) for n, c in enumerate(cases) for a, b in c["multi"][j]]
        slices = sg.extract_segments(clouds, keys[0], keys[1], threshold)
        assert len(slices) == len(triples)
        for (n, a, b), view in zip(triples, slices):
            assert np.shares_memory(view, clouds[n]) and same_bits(view, clouds[n][a:b])
    sg = seg.Segmentation(None, ctx=ctx, weights=weights)
    assert sg.segment_indices(clouds, keys[0], keys[1], single=True) == [(n, int(c["single"][0]), int(c["single"][1])) for n, c in enumerate(cases)]
    for c, view in zip(cases, sg.extract_single_segments(clouds, keys[0], keys[1])):
        assert len(view) == max(0, int(c["single"][1]) - int(c["single"][0]))
    det = seg.KeyframeDetector(None, ctx=ctx, weights=weights)
    c = cases[0]
    assert det.find_instance(c["cloud"], keys[0]) == int(c["single"][0]) and det.find_instance(c["cloud"], keys[1]) == int(c["single"][1])
    threshold = c["settings"][0][0]
    assert det.find_instances(c["cloud"], keys[0], threshold) == seg.argmin_multi(c["S"].tolist(), threshold)
    d = det.calculate_distances(clouds, keys[1])
    assert all(same_bits(x, y[1]) for x, y in zip(d, seg.keyframe_distances(clouds, keys, weights, ctx=ctx)))


def skeleton_and_motions():
    joints, animated, motions = end_to_end()
    return _capi.Skeleton(joints, animated), [j[0] for j in joints], motions


def test_extract_segments_from_quaternion_motions(ctx):
    """Case (c): the golden slices bit for bit, through the forward kinematics on the device."""
    sk, names, motions = skeleton_and_motions()
    sg = seg.Segmentation(sk, names, int(GOLDEN["e_min_segment_size"]), ctx=ctx)
    start, end, threshold = GOLDEN["e_start"], GOLDEN["e_end"], float(GOLDEN["e_threshold"])
    triples = sg.segment_indices(motions, start, end, threshold)
    assert triples == [tuple(int(v) for v in t) for t in GOLDEN["e_segments"]]
    slices = sg.extract_segments(motions, start, end, threshold)
    assert all(np.shares_memory(v, motions[m]) for (m, _, _), v in zip(triples, slices))
    assert same_bits(np.concatenate(slices), GOLDEN["e_slices"])
    assert sg.segment_indices(motions, start, end, single=True) == [tuple(int(v) for v in t) for t in GOLDEN["e_single"]]
    singles = sg.extract_single_segments(motions, start, end)
    assert [len(v) for v in singles] == [max(0, int(b) - int(a)) for _, a, b in GOLDEN["e_single"]]
    det = seg.KeyframeDetector(sk, names, ctx=ctx)
    assert det.find_instance(motions[0], start) == int(GOLDEN["e_single"][0][1])
    with pytest.raises(ValueError):
        sg.extract_segments(motions, start[:5], end[:5], threshold)
    with pytest.raises(ValueError):
        seg.Segmentation(None, ctx=ctx).extract_segments(motions, start, end, threshold)


def test_segments_run_through_align_frames_temporally(ctx):
    sk, names, motions = skeleton_and_motions()
    sg = seg.Segmentation(sk, names, int(GOLDEN["e_min_segment_size"]), ctx=ctx)
    slices = sg.extract_segments(motions, GOLDEN["e_start"], GOLDEN["e_end"], float(GOLDEN["e_threshold"]))
    clips = collections.OrderedDict(("clip_%02d" % i, v) for i, v in enumerate(slices))
    warped, warps = dtw.align_frames_temporally(sk, names, clips, ctx=ctx)
    fr = len(clips[dtw.get_average_time_line(clips)])
    assert list(warped.keys()) == list(clips.keys())
    for k, clip in clips.items():
        assert warped[k].shape == (fr, clip.shape[1]) and len(warps[k]) == fr
        assert warps[k][-1] == len(clip) - 1 and same_bits(warped[k], clip[warps[k]])


def status_of(call):
    with pytest.raises(_capi.MGError) as ei:
        call()
    return ei.value.status


def test_limits_and_misuse(ctx):
    """The documented status, before any kernel of the two calls is launched; nothing here can fault."""
    J = 3
    off = lambda *lengths: np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)      # noqa: E731
    big = ctx.upload(np.zeros((40, 65, 3)))
    out = ctx.malloc(8 * 16 * 40)
    ints = ctx.malloc(8 * 200)
    cnt = ctx.malloc(4 * 16)
    invalid = _capi.MG_ERR_INVALID_ARGUMENT
    try:
        kd = lambda o, j=J, k=2, w=None: _capi.keyframe_distances(ctx, big, o, j, big, k, w, out)      # noqa: E731
        assert status_of(lambda: kd(off(4), 65)) == invalid
        assert status_of(lambda: kd(off(4), 0)) == invalid
        assert status_of(lambda: kd(off(4), J, 9)) == invalid
        assert status_of(lambda: kd(off(4), J, 0)) == invalid
        assert status_of(lambda: kd(np.array([0, 5, 5], dtype=np.int64))) == invalid       # an empty motion
        assert status_of(lambda: kd(np.array([0, 5, 3], dtype=np.int64))) == invalid
        assert status_of(lambda: kd(np.array([1, 5], dtype=np.int64))) == invalid
        assert status_of(lambda: kd(off(4), J, 2, [1.0, -1.0, 1.0])) == invalid
        assert status_of(lambda: kd(off(4), J, 2, [0.0, 0.0, 0.0])) == invalid
        with pytest.raises(ValueError):
            kd(off(4), J, 2, [1.0, 1.0])
        kd(off())                 # no motions: MG_OK, nothing to do
        kd(off(30, 10), 64, 8)    # the limits themselves are supported (their values: test_gpu_construction_shapes.py)
        search = lambda o, so, mode=seg.MULTI, t=1.0, m=1: _capi.segment_search(ctx, big, big, o, mode, t, m, so, ints, cnt)      # noqa: E731
        assert status_of(lambda: search(off(10), off(6), 2)) == invalid
        assert status_of(lambda: search(off(10), off(6), seg.MULTI, np.nan)) == invalid
        assert status_of(lambda: search(off(10), off(6), seg.MULTI, 1.0, -1)) == invalid
        assert status_of(lambda: search(off(10), off(5))) == invalid                       # room for 5 pairs, 10 / 2 + 1 needed
        assert status_of(lambda: search(off(10, 10), off(6, 0), seg.SINGLE)) == invalid
        assert status_of(lambda: search(np.array([0, 5, 5], dtype=np.int64), off(6, 6))) == invalid
        assert status_of(lambda: search(np.array([2, 5], dtype=np.int64), off(6))) == invalid
        with pytest.raises(ValueError):
            search(off(10), off(6, 6))
        search(off(), off())
        search(off(10), off(6))
        search(off(10, 10), off(1, 1), seg.SINGLE)
        # a NaN in the clouds or the keyframes, an infinity in the distances
        bad = np.zeros((9, J, 3))
        bad[7, 1, 2] = np.nan
        b_dev = ctx.upload(bad)
        d = np.ones(10)
        d[9] = np.inf
        d_dev = ctx.upload(d)
        try:
            assert status_of(lambda: _capi.keyframe_distances(ctx, b_dev, off(4, 5), J, big, 2, None, out)) == invalid
            assert status_of(lambda: _capi.keyframe_distances(ctx, big, off(4, 5), J, b_dev, 8, None, out)) == invalid     # the NaN lies in keyframe 7
            assert status_of(lambda: _capi.segment_search(ctx, d_dev, big, off(10), seg.MULTI, 1.0, 1, off(6), ints, cnt)) == invalid
            assert status_of(lambda: _capi.segment_search(ctx, big, d_dev, off(10), seg.SINGLE, 1.0, 1, off(1), ints, cnt)) == invalid
        finally:
            b_dev.free()
            d_dev.free()
    finally:
        for b in (big, out, ints, cnt):
            b.free()
    with pytest.raises(ValueError):
        seg.keyframe_distances([np.zeros((4, 65, 3))], np.zeros((1, 65, 3)), ctx=ctx)
    with pytest.raises(ValueError):
        seg.keyframe_distances([np.zeros((4, 3, 3))], np.zeros((9, 3, 3)), ctx=ctx)
    with pytest.raises(ValueError):
        seg.segment_search([np.ones(4)], [np.ones(5)], seg.MULTI, ctx=ctx)
    assert seg.keyframe_distances([], np.zeros((2, 3, 3)), ctx=ctx) == [] and seg.segment_search([], [], seg.MULTI, ctx=ctx) == []
    assert seg.Segmentation(None, ctx=ctx).extract_segments([], np.zeros((3, 3)), np.zeros((3, 3))) == []
