"""The host side of the all-pairs DTW search (morphablegraphs_amd.dtw: all_pairs_costs_host, reference_from_costs): the selection the
reference's find_optimal_dtw means (construction/dtw.py:125-146) and the cost matrix against tests/golden/dtw.npz."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dtw_host import GOLDEN, grid_bound, point_case, same_bits  # noqa: E402

from morphablegraphs_amd import dtw  # noqa: E402


def point_table(s):
    """The table of point set s: [the reference motion] + its motions; the set's weights (None for set 0)."""
    cases = [point_case(s, k) for k in range(int(GOLDEN["p%d_n" % s]))]
    return cases, [cases[0]["ref"]] + [c["cloud"] for c in cases], (None if s == 0 else cases[0]["weights"])


def test_the_least_mean_wins_not_the_last_key():
    """The reference's loop never updates best_d, so its last key wins; here the least mean does."""
    costs = np.array([[0.0, 4.0, 5.0], [1.0, 0.0, 1.0], [3.0, 2.5, 0.0]])
    key, means = dtw.reference_from_costs(costs, ["a", "b", "c"])
    assert key == "b" and means.tolist() == [3.0, 2.0 / 3.0, 5.5 / 3.0]


def test_the_first_of_equal_least_means_is_kept():
    costs = np.array([[0.0, 9.0], [3.0, 1.0], [1.0, 3.0], [2.0, 2.0]])
    key, means = dtw.reference_from_costs(costs, [10, 11, 12, 13])
    assert means.tolist() == [4.5, 2.0, 2.0, 2.0] and key == 11


def test_a_row_is_added_in_column_order():
    """avg_distances[i] += path_cost, one motion after the other: ((1e16 + 1) - 1e16) + 1 = 1, not 2 and not 0."""
    row = [1e16, 1.0, -1e16, 1.0]
    long_row = [1e16] + [1.0] * 7 + [-1e16] + [1.0] * 7     # pairwise or blocked sums give another value
    in_order = 0.0
    for v in long_row:
        in_order += v
    assert in_order == 7.0 and float(np.sum(long_row)) != in_order
    key, means = dtw.reference_from_costs(np.array([row, [0.5, 0.5, 0.5, 0.5]]), ["x", "y"])
    assert means.tolist() == [0.25, 0.5] and key == "x"
    key, means = dtw.reference_from_costs(np.array([long_row, [0.5] * 16]), ["x", "y"])
    assert means.tolist() == [7.0 / 16, 0.5] and key == "x"


def test_non_finite_costs_and_bad_shapes_are_refused():
    costs = np.ones((2, 3))
    for bad in (np.nan, np.inf):
        c = costs.copy()
        c[1, 2] = bad
        with pytest.raises(ValueError):
            dtw.reference_from_costs(c, ["a", "b"])
    with pytest.raises(ValueError):
        dtw.reference_from_costs(costs, ["a", "b", "c"])
    with pytest.raises(ValueError):
        dtw.reference_from_costs(np.zeros((0, 0)), [])


@pytest.mark.parametrize("s", range(int(GOLDEN["n_point_sets"])))
def test_all_pairs_costs_host_on_the_golden_point_sets(s):
    """Row 0 (the set's reference motion) against the golden D[-1, -1] within (Fr + F) x the grid's bound; a motion against
    itself costs the sum of its grid's diagonal; `references` picks rows."""
    cases, table, weights = point_table(s)
    costs = dtw.all_pairs_costs_host(table, weights)
    assert costs.shape == (len(table), len(table)) and np.all(np.isfinite(costs))
    for k, c in enumerate(cases):
        err, bound = abs(costs[0, k + 1] - c["D"][-1, -1]), sum(c["S"].shape) * grid_bound(c)
        print("%s: |total - golden| %.3g, bound %.3g" % (c["name"], err, bound))
        assert err <= bound, c["name"]
    for n, cloud in enumerate(table):
        diagonal = np.diag(dtw.distance_grid_host(cloud, cloud, weights))
        in_order = 0.0
        for v in diagonal.tolist():
            in_order += v
        assert costs[n, n] == in_order, n
    picked = dtw.all_pairs_costs_host(table, weights, references=[2, 0])
    assert same_bits(picked, costs[[2, 0]])
    with pytest.raises(ValueError):
        dtw.all_pairs_costs_host(table, weights, references=[len(table)])


def test_the_public_names():
    import morphablegraphs_amd
    for name in ("all_pairs_costs", "reference_from_costs", "select_reference_motion", "align_frames_temporally"):
        assert getattr(morphablegraphs_amd, name) is getattr(dtw, name)
