"""The NumPy statements of the arc-length queries (morphablegraphs_amd/spline_types.py: arc_length_of_point_host,
tangent_at_arc_length_host, angle_at_arc_length_2d_host, sample_parameters_host) against vectors the reference's own, unmodified
ParameterizedSpline produced (tests/golden/trajectory_arc_queries.npz, tools/gen_trajectory_arc_golden.py).  No GPU.

Tolerances.  Arc lengths and points: those tests/test_oracle_golden.py holds the pinned arc-length tables to (rtol 1e-12 on arc
lengths, atol 1e-9 on points looked up by arc length).  Tangents: a unit chord (p2 - p1) / |p2 - p1| whose ends are good to 1e-9 each;
the shortest chord of the fixture is the one past the end of the path (arc length full + 2.55, range widened to 2.6: 0.05 units of
path), so 2e-9 / 0.05 per component, doubled for the normalisation = 8e-8.  Angles: acos of a dot product of unit vectors good to
8e-8 each; |d acos / dx| = 1 / sin(angle), and the fixture's angles stay 5 degrees away from 0 and 180 (asserted), so
1.6e-7 / sin(5 deg) rad = 1.1e-4 degrees; 2e-4."""
import math

import numpy as np
import pytest

from conftest import load_golden
from morphablegraphs_amd import spline_types as st

ARC_RTOL, POINT_ATOL = 1.0e-12, 1.0e-9
TANGENT_ATOL, ANGLE_ATOL = 8.0e-8, 2.0e-4


@pytest.fixture(scope="module")
def golden():
    return load_golden("trajectory_arc_queries")


def _cases(g):
    for t in g["spline_types"]:
        for n in g["n_points"]:
            key = "%d_%d" % (t, n)
            poly = st.trajectory_polynomials_host(g["control_points_" + key], int(t))
            arcs, full = st.arc_length_table_host(poly, 1000)
            yield key, poly, arcs, full


def test_sample_parameters_are_the_references_sums(golden):
    for gran, count, last in zip(golden["uk_granularity"], golden["uk_count"], golden["uk_last"]):
        us = st.sample_parameters_host(int(gran))
        assert len(us) == int(count) and us[-1] == float(last), (gran, len(us), us[-1])
        assert us[0] == 0.0 and np.all(np.diff(us) > 0.0) and us[-1] <= 1.0
    # the sums drift: neither the count nor the values are those of k / granularity
    assert len(st.sample_parameters_host(1000)) == 1000 and len(st.sample_parameters_host(1024)) == 1025
    assert np.any(st.sample_parameters_host(1000) != np.arange(1000) / 1000.0)


def test_points_tangents_and_angles_against_the_reference(golden):
    ref_dir = golden["reference_dir"]
    for key, poly, arcs, full in _cases(golden):
        np.testing.assert_allclose(full, float(golden["full_arc_length_" + key]), rtol=ARC_RTOL)
        want_angles = golden["angles_" + key]
        assert np.all((want_angles > 5.0) & (want_angles < 175.0))
        for a, p, t, ang in zip(golden["arcs_" + key], golden["points_by_arc_" + key], golden["tangents_" + key], want_angles):
            start, tangent, angle = st.angle_at_arc_length_2d_host(poly, arcs, full, a, ref_dir)
            np.testing.assert_allclose(start, p, rtol=0, atol=POINT_ATOL, err_msg=key)
            np.testing.assert_allclose(tangent, t, rtol=0, atol=TANGENT_ATOL, err_msg=key)
            np.testing.assert_allclose(angle, ang, rtol=0, atol=ANGLE_ATOL, err_msg=key)
            start2, tangent2 = st.tangent_at_arc_length_host(poly, arcs, full, a)
            assert np.array_equal(start2, start) and np.array_equal(tangent2, tangent)


def test_arc_length_of_points_against_the_reference(golden):
    us = st.sample_parameters_host(1000)
    total = left_out = 0
    for key, poly, arcs, full in _cases(golden):
        amb = golden["q_ambiguous_" + key]
        for i, (p, m) in enumerate(zip(golden["q_points_" + key], golden["q_min_arc_" + key])):
            arc, point, k = st.arc_length_of_point_host(poly, arcs, full, p, m, us)
            want_arc, want_k = float(golden["q_arc_" + key][i]), int(golden["q_min_index_" + key][i])
            total += 1
            if want_k < 0:
                assert (arc, point, k) == (-1.0, None, -1) and want_arc == -1.0
                continue
            if amb[i]:
                left_out += 1
                continue
            assert k == want_k and us[k] == float(golden["q_min_u_" + key][i]), (key, i, k, want_k)
            np.testing.assert_allclose(arc, want_arc, rtol=ARC_RTOL, err_msg=key)
            np.testing.assert_allclose(point, golden["q_min_point_" + key][i], rtol=0, atol=POINT_ATOL, err_msg=key)
            assert arc > m
    assert left_out <= 0.02 * total, (left_out, total)
    assert any(int(k) < 0 for key, *_ in _cases(golden) for k in golden["q_min_index_" + key])


def test_absolute_arc_length_restates_the_lookup():
    """get_absolute_arc_length's own cases: a parameter on a table entry, between two, the last entry, and the strict > of the scan."""
    arcs = np.array([0.0, 0.1, 0.4, 1.0])
    full = 30.0
    assert st.absolute_arc_length_host(arcs, full, 0.0) == 0.0
    assert st.absolute_arc_length_host(arcs, full, 1.0) == 30.0
    t = 0.5
    i = int(t / (1.0 / 3))
    want = (arcs[i] + ((t - i / 3.0) / ((i + 1) / 3.0 - i / 3.0)) * (arcs[i + 1] - arcs[i])) * full
    assert st.absolute_arc_length_host(arcs, full, t) == want
    # a straight path: a min_arc_length equal to a sample's arc length excludes that sample
    poly = st.trajectory_polynomials_host([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0]], 0)
    arcs, full = st.arc_length_table_host(poly, 8)
    us = st.sample_parameters_host(8)
    a3 = st.absolute_arc_length_host(arcs, full, us[3])
    arc, point, k = st.arc_length_of_point_host(poly, arcs, full, st.polynomial_point(poly, us[3]), a3, us)
    assert k == 4 and arc > a3
    assert st.arc_length_of_point_host(poly, arcs, full, [1.0, 0.0, 0.0], full, us) == (-1.0, None, -1)


TIE_CPS = [[0.0, 0.0, 0.0], [16.0, 0.0, 0.0], [32.0, 0.0, 0.0], [48.0, 0.0, 0.0]]
TIE_GRANULARITY = 64
TIE_K = 30


def tie_point(poly, us):
    """A point at exactly the same distance from samples TIE_K and TIE_K + 1 of the Catmull-Rom path through TIE_CPS: its middle piece
    is x = 16 + 16 t with integer coefficients, the parameters are multiples of 1 / 64, so both samples, their midpoint and the two
    differences are exact."""
    a, b = st.polynomial_point(poly, us[TIE_K]), st.polynomial_point(poly, us[TIE_K + 1])
    assert (a[0], b[0]) == (22.5, 23.25) and not a[1:].any() and not b[1:].any()
    q = np.array([0.5 * (a[0] + b[0]), 3.0, 0.0])
    assert q[0] - a[0] == b[0] - q[0] == 0.375
    return q


def test_the_first_of_two_equal_distances_wins():
    """A straight path with a point on the perpendicular bisector of two samples: the distances are equal by construction."""
    poly = st.trajectory_polynomials_host(TIE_CPS, 0)
    arcs, full = st.arc_length_table_host(poly, TIE_GRANULARITY)
    us = st.sample_parameters_host(TIE_GRANULARITY)
    assert st.arc_length_of_point_host(poly, arcs, full, tie_point(poly, us), 0.0, us)[2] == TIE_K


def test_acos_statement_is_within_an_ulp_of_the_library():
    xs = np.concatenate([np.linspace(-1.0, 1.0, 4001), [0.5, -0.5, np.nextafter(0.5, 0), np.nextafter(-0.5, 0), 1e-300, 0.0]])
    for x in xs:
        got, want = st.acos_host(x), math.acos(x)
        assert abs(got - want) <= 2.0 ** -52 * max(want, 2.0 ** -30), (x, got, want)
    assert math.isnan(st.acos_host(1.0000000000000002)) and math.isnan(st.acos_host(float("nan")))


def test_tangent_widening_and_its_bound():
    """A doubled control point: the chord's ends coincide and eval_range is widened; far past the end the bound is reported."""
    cps = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [40.0, 0.0, 30.0], [80.0, 0.0, 0.0]]
    poly = st.trajectory_polynomials_host(cps, 0)
    arcs, full = st.arc_length_table_host(poly, 1000)
    start, tangent = st.tangent_at_arc_length_host(poly, arcs, full, full + 1.0, 0.5)       # both ends past the end until r > 1
    assert np.array_equal(start, [80.0, 0.0, 0.0]) and abs(np.linalg.norm(tangent) - 1.0) < 1e-15
    with pytest.raises(st.TangentWideningExhausted):
        st.tangent_at_arc_length_host(poly, arcs, full, full + 1000.0)
