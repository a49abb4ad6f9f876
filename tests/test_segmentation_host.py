"""The host restatements of morphablegraphs_amd.segmentation against tests/golden/segmentation.npz (tools/
gen_segmentation_golden.py: the reference's construction/keyframe_detection.py and segmentation.py imported unmodified, the
distance from oracle.mg_oracle's 2-D fit).

From given distances, the segments of both modes are the reference's exactly.  The distances themselves follow the project's
parity rule, the one of tests/test_dtw_host.py: |ours - golden| <= 10 * max(spread, 1e-13 * max|S|), spread being the
reference-side restatement's own largest change over 3 reruns with the joints permuted (recorded by the generator)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dtw_host import check_grid, same_bits  # noqa: E402

from morphablegraphs_amd import segmentation as seg  # noqa: E402

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmentation.npz"))
POINT = [(s, k) for s in range(int(GOLDEN["n_point_sets"])) for k in range(int(GOLDEN["p%d_n" % s]))]
CASES = list(range(int(GOLDEN["n_distance_cases"])))
P_SETTINGS = [(float(t), int(m)) for t, m in GOLDEN["p_settings"]]


def point_case(s, k):
    p, q = "p%d_" % s, "p%d_c%d_" % (s, k)
    c = {name: GOLDEN[q + name] for name in ("cloud", "S", "E", "spread", "single", "margin", "redraws")}
    c.update({"weights": GOLDEN[p + "weights"], "start": GOLDEN[p + "start"], "end": GOLDEN[p + "end"], "settings": P_SETTINGS,
              "multi": [GOLDEN[q + "t%d_multi" % j] for j in range(len(P_SETTINGS))], "name": "%s capture %d" % (str(GOLDEN[p + "name"]), k)})
    return c


def distance_case(i):
    q = "g%d_" % i
    settings = [(float(t), int(m)) for t, m in GOLDEN[q + "settings"]]
    return {"S": GOLDEN[q + "S"], "E": GOLDEN[q + "E"], "single": GOLDEN[q + "single"], "settings": settings,
            "multi": [GOLDEN[q + "t%d_multi" % j] for j in range(len(settings))], "name": str(GOLDEN[q + "name"])}


def all_search_cases():
    return [point_case(s, k) for s, k in POINT] + [distance_case(i) for i in CASES]


def weights_of(s, c):
    return None if s == 0 else c["weights"]


def check_distances(what, ours, c):
    """The parity rule on the (2, F) distances to the start and the end keyframe; returns the larger error / bound."""
    return max(check_grid("%s, %s keyframe" % (what, name), ours[i], {"S": c[key], "spread": c["spread"]})
               for i, (name, key) in enumerate((("start", "S"), ("end", "E"))))


def end_to_end():
    joints = [(str(n), str(p) if str(p) else None, tuple(o)) for n, p, o in zip(GOLDEN["e_joint_names"], GOLDEN["e_joint_parents"], GOLDEN["e_joint_offsets"])]
    motions = [GOLDEN["e_m%d_frames" % m] for m in range(int(GOLDEN["e_n"]))]
    return joints, [str(a) for a in GOLDEN["e_animated_joints"]], motions


def test_the_golden_file_keeps_the_generators_conditions():
    assert 4 * int(GOLDEN["redraws"]) <= int(GOLDEN["draws"])
    for s, k in POINT:
        assert float(point_case(s, k)["margin"]) >= 1e-6
    assert float(GOLDEN["e_margin"]) >= 1e-6
    lengths = [len(point_case(0, k)["S"]) for k in range(int(GOLDEN["p0_n"]))]
    assert any(f < 1024 for f in lengths) and any(f > 1024 for f in lengths) and max(lengths) >= 3000
    assert len(set(np.round(GOLDEN["p1_weights"], 6))) > 1 and len(set(np.round(GOLDEN["p0_weights"], 6))) == 1
    for s, k in POINT:
        assert all(2 <= len(m) <= 5 for m in point_case(s, k)["multi"][:1])
    names = [distance_case(i)["name"] for i in CASES]
    assert len(distance_case(names.index("one_frame"))["S"]) == 1
    assert all(len(m) == 0 for i in CASES if distance_case(i)["name"] in ("adjacent_instances_every_window_dropped", "no_kept_segment")
               for m in distance_case(i)["multi"])
    assert any(t == 0.0 for i in CASES for t, _ in distance_case(i)["settings"]) and any(m == 0 for i in CASES for _, m in distance_case(i)["settings"])


@pytest.mark.parametrize("c", all_search_cases(), ids=lambda c: str(c["name"]).replace(" ", "_"))
def test_segment_search_host_is_the_reference(c):
    single = seg.segment_search_host(c["S"], c["E"], seg.SINGLE)
    assert single == [tuple(int(v) for v in c["single"])]
    for (threshold, min_size), pairs in zip(c["settings"], c["multi"]):
        ours = seg.segment_search_host(c["S"], c["E"], seg.MULTI, threshold, min_size)
        assert ours == [tuple(int(v) for v in p) for p in pairs], (c["name"], threshold, min_size)
        assert all(e - s > min_size for s, e in ours) and all(a[1] <= b[0] for a, b in zip(ours, ours[1:]))
        assert len(ours) <= len(c["S"]) // (min_size + 1) + 1
    assert seg.argmin(c["S"].tolist()) == int(c["single"][0]) == int(np.argmin(c["S"]))
    assert seg.argmin_multi(c["S"].tolist(), 0.0) == np.flatnonzero(c["S"] == c["S"].min()).tolist()


@pytest.mark.parametrize("s,k", POINT)
def test_keyframe_distances_host_against_the_restatement(s, k):
    c = point_case(s, k)
    ours = seg.keyframe_distances_host([c["cloud"]], np.stack([c["start"], c["end"]]), weights_of(s, c))[0]
    assert ours.shape == (2, len(c["cloud"]))
    check_distances(c["name"], ours, c)
    # a frame's distance is the cell (frame, keyframe) of the DTW grid, in bits
    from morphablegraphs_amd import dtw
    assert same_bits(ours[1], dtw.distance_grid_host(c["cloud"], c["end"][None], weights_of(s, c))[:, 0])


def test_first_index_wins_ties():
    assert seg.argmin([3.0, 1.0, 1.0, 2.0]) == 1 and seg.argmin([]) == 0 and seg.argmin([0.0, -0.0]) == 0
    assert seg.argmin_multi([3.0, 1.0, 1.5, 2.0, 1.0], 0.5) == [1, 2, 4]
    flat = np.zeros(40)
    # every frame is an instance: all windows but the last are one frame long; the last runs from 39 to 39
    assert seg.segment_search_host(flat, flat, seg.MULTI, 0.0, 0) == []
    assert seg.segment_search_host(flat, flat, seg.SINGLE) == [(0, 0)]
    # one instance at 0: the window is [0, 39), the arg-min of equal end distances its first frame: nothing is kept
    start = np.ones(40)
    start[0] = 0.0
    assert seg.segment_search_host(start, flat, seg.MULTI, 0.5, 0) == []
    end = np.ones(40)
    end[[20, 30]] = 0.25
    assert seg.segment_search_host(start, end, seg.MULTI, 0.5, 19) == [(0, 20)]
    assert seg.segment_search_host(start, end, seg.MULTI, 0.5, 20) == []


def test_limits_and_argument_errors_raise():
    d = np.ones(12)
    bad = d.copy()
    bad[3] = np.nan
    for call in (lambda: seg.segment_search_host(bad, d, seg.SINGLE), lambda: seg.segment_search_host(d, bad, seg.MULTI),
                 lambda: seg.segment_search_host(d, d[:5], seg.MULTI), lambda: seg.segment_search_host([], [], seg.SINGLE),
                 lambda: seg.segment_search_host(d, d, 2), lambda: seg.segment_search_host(d, d, seg.MULTI, 1.0, -1),
                 lambda: seg.segment_search_host(d, d, seg.MULTI, np.nan, 1)):
        with pytest.raises(ValueError):
            call()
    cloud, keys = np.zeros((5, 3, 3)), np.zeros((2, 3, 3))
    assert seg.keyframe_distances_host([cloud], keys)[0].shape == (2, 5) and seg.keyframe_distances_host([], keys) == []
    nan_cloud = cloud.copy()
    nan_cloud[2, 1, 0] = np.inf
    for call in (lambda: seg.keyframe_distances_host([np.zeros((5, 65, 3))], np.zeros((1, 65, 3))),
                 lambda: seg.keyframe_distances_host([cloud], np.zeros((9, 3, 3))), lambda: seg.keyframe_distances_host([cloud], np.zeros((0, 3, 3))),
                 lambda: seg.keyframe_distances_host([cloud, np.zeros((0, 3, 3))], keys), lambda: seg.keyframe_distances_host([nan_cloud], keys),
                 lambda: seg.keyframe_distances_host([np.zeros((5, 4, 3))], keys), lambda: seg.keyframe_distances_host([cloud], np.zeros((3, 3)))):
        with pytest.raises(ValueError):
            call()


def test_device_functions_have_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        return      # with a device the GPU tests say what the functions do
    from morphablegraphs_amd import _capi
    c = point_case(0, 0)
    with pytest.raises(_capi.MGError):
        seg.Segmentation(None).extract_segments([c["cloud"]], c["start"], c["end"], 0.01)
