"""The host restatements of morphablegraphs_amd.dtw against tests/golden/dtw.npz (tools/gen_dtw_golden.py: the reference's
construction/dtw.py imported unmodified, the cell distance from oracle.mg_oracle's 2-D fit).

From a given grid S, the accumulated cost D, the path and the warping function are the reference's bit for bit.  The grids
themselves follow the project's parity rule: |ours - golden| <= 10 * max(spread, 1e-13 * max|S|), spread being the
reference-side restatement's own largest change over 3 reruns with the joints permuted (recorded by the generator)."""
import collections
import os

import numpy as np
import pytest

from morphablegraphs_amd import dtw

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dtw.npz"))
POINT = [(s, k) for s in range(int(GOLDEN["n_point_sets"])) for k in range(int(GOLDEN["p%d_n" % s]))]
GRIDS = list(range(int(GOLDEN["n_grids"])))
MOTIONS = list(range(len(GOLDEN["e_keys"])))
MARGIN, FLOOR = 10.0, 1e-13


def point_case(s, k):
    p, q = "p%d_" % s, "p%d_m%d_" % (s, k)
    c = {name: GOLDEN[q + name] for name in ("cloud", "S", "D", "path", "warp", "spread", "gap", "redraws")}
    c.update({"ref": GOLDEN[p + "ref"], "weights": GOLDEN[p + "weights"], "name": "%s motion %d" % (str(GOLDEN[p + "name"]), k)})
    return c


def grid_case(i):
    return {name: GOLDEN["g%d_%s" % (i, name)] for name in ("S", "D", "path", "warp", "name")}


def all_grid_cases():
    return [point_case(s, k) for s, k in POINT] + [grid_case(i) for i in GRIDS]


def grid_bound(c):
    return MARGIN * max(float(c["spread"]), FLOOR * float(np.max(np.abs(c["S"]))))


def check_grid(what, ours, c):
    """The parity rule; prints the figure before it asserts.  Returns error / bound."""
    err, bound = float(np.max(np.abs(ours - c["S"]))), grid_bound(c)
    print("%s: max |S - golden| %.3g, bound %.3g, ratio %.3g" % (what, err, bound, err / bound))
    assert ours.shape == c["S"].shape and err <= bound, (what, err, bound)
    return err / bound


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def end_to_end():
    joints = [(str(n), str(p) if str(p) else None, tuple(o)) for n, p, o in zip(GOLDEN["e_joint_names"], GOLDEN["e_joint_parents"], GOLDEN["e_joint_offsets"])]
    keys = [str(k) for k in GOLDEN["e_keys"]]
    motions = collections.OrderedDict((k, GOLDEN["e_m%d_frames" % i]) for i, k in enumerate(keys))
    return joints, [str(a) for a in GOLDEN["e_animated_joints"]], keys, motions


def test_the_golden_file_keeps_the_generators_conditions():
    assert 4 * int(GOLDEN["redraws"]) <= int(GOLDEN["draws"])
    for s, k in POINT:
        assert float(point_case(s, k)["gap"]) >= 1e-6
    assert float(GOLDEN["e_gap"]) >= 1e-6
    shapes = [point_case(0, k)["S"].shape for k in range(int(GOLDEN["p0_n"]))]
    fr = shapes[0][0]
    assert any(f > fr for _, f in shapes) and any(1 < f < fr for _, f in shapes) and any(f == 1 for _, f in shapes) and any(f == fr for _, f in shapes)
    assert len(set(np.round(GOLDEN["p1_weights"], 6))) > 1


@pytest.mark.parametrize("c", all_grid_cases(), ids=lambda c: str(c["name"]).replace(" ", "_"))
def test_paths_host_is_the_reference_bit_for_bit(c):
    D, path, warp = dtw.dtw_paths_host(c["S"])
    assert same_bits(D, c["D"])
    assert path == [tuple(int(v) for v in p) for p in c["path"]]
    assert warp == c["warp"].tolist()
    assert dtw.get_warping_function(path) == c["warp"].tolist()
    assert dtw.get_warping_function(c["path"]) == c["warp"].tolist()


@pytest.mark.parametrize("s,k", POINT)
def test_distance_grid_host_against_the_restatement(s, k):
    c = point_case(s, k)
    weights = None if s == 0 else c["weights"]
    check_grid(c["name"], dtw.distance_grid_host(c["ref"], c["cloud"], weights), c)


def test_the_reference_motion_against_itself_walks_the_diagonal():
    c = next(point_case(0, k) for k in range(int(GOLDEN["p0_n"])) if np.array_equal(point_case(0, k)["cloud"], GOLDEN["p0_ref"]))
    S = dtw.distance_grid_host(c["ref"], c["cloud"])
    _, path, warp = dtw.dtw_paths_host(S)
    n = len(c["ref"])
    assert path == [(i, i) for i in range(n)] and warp == list(range(n))
    assert np.max(np.diag(S)) <= grid_bound(c)


def test_first_minimum_wins_ties():
    """find_path's rule on a grid of equal cells: always the diagonal, then (i-1, j) once the first column is reached."""
    _, path, warp = dtw.dtw_paths_host(np.ones((3, 5)))
    assert path == [(0, 0), (0, 1), (0, 2), (1, 3), (2, 4)] and warp == [2, 3, 4]
    _, path, _ = dtw.dtw_paths_host(np.ones((4, 2)))
    assert path == [(0, 0), (1, 0), (2, 0), (3, 1)]


def test_warp_motion_and_average_time_line_against_the_reference():
    _, _, keys, motions = end_to_end()
    assert dtw.get_average_time_line(motions) == str(GOLDEN["e_mean_key"])
    for i, k in enumerate(keys):
        warped = np.array(dtw.warp_motion(motions[k], GOLDEN["e_m%d_warp" % i].tolist()))
        assert same_bits(warped, GOLDEN["e_m%d_warped" % i])
        assert dtw.get_warping_function(GOLDEN["e_m%d_path" % i]) == GOLDEN["e_m%d_warp" % i].tolist()
    # the first of equally distant motions is kept
    assert dtw.get_average_time_line(collections.OrderedDict([("a", [0] * 4), ("b", [0] * 6), ("c", [0] * 5), ("d", [0] * 5)])) == "c"


def test_device_functions_have_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from morphablegraphs_amd import _capi
    c = point_case(0, 0)
    with pytest.raises(_capi.MGError):
        dtw.run_dtw(c["ref"], c["cloud"])
