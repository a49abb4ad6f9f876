"""The B-spline and fitted-B-spline trajectories (the reference's SPLINE_TYPE_BSPLINE = 1, SPLINE_TYPE_FITTED_BSPLINE = 2) on the host:
morphablegraphs_amd.spline_types.trajectory_polynomials_host -- the statement of the table mg_trajectory_create_typed builds --
against tests/golden/trajectory_spline_types.npz, which the reference's own ParameterizedSpline produced
(tools/gen_spline_type_golden.py), and the Python seam that recognises the reference's spline objects.

BOUND.  The conversion to the power basis rounds differently from de Boor's recurrence and from FITPACK's splev.  Measured over the
whole fixture in float64 (points by parameter, full arc length, points by arc length; coordinates up to 365): the largest absolute
difference is MEASURED = 5.684e-13 (a by-arc-length point of the 9-point fitted spline; points by parameter 1.137e-13, full arc length
4.547e-13).  BOUND = 16 x MEASURED leaves room for another libm or compiler.  MEASURED is 1.6e-15 of the largest coordinate, far
below the 1e-9 at which the conversion would count as wrong.  The tests print what they measure."""
import math
import os

import numpy as np
import pytest

from morphablegraphs_amd import spline_types as st
from morphablegraphs_amd.candidate_scoring import _spline_control_points, cached_trajectory, constraints_to_device_form, trajectory_to_device_form
from morphablegraphs_amd.spline_types import (arc_length_table_host, point_by_arc_length_host, polynomial_point, trajectory_polynomials_host,
                                              trajectory_segment_count)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEASURED = 5.684341886080802e-13
BOUND = 16.0 * MEASURED
CURVES = [(t, n) for t in (1, 2) for n in (4, 5, 9)]
# the closest-point search: see test_the_statements_search_is_the_references_search
U_TOL_CATMULL_ROM, D_TOL_CATMULL_ROM = 2.0e-6, 1.0e-6      # tests/test_gpu_closest_point.py


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trajectory_spline_types.npz"))


def closest_point_bounds(full_arc_length):
    """(|du| bound, |dd| bound) of the typed curves' closest-point search against the reference's find_closest_point_fast: TWICE the
    worst difference the Catmull-Rom test tolerates on tests/golden/trajectory_closest_point.npz, relative to the path length.  That
    test allows |dd| <= 1e-6 max(1, d_ref) per frame; over the fixture's 26 tracks the largest such allowance is 4.011e-6 of its
    spline's arc length (the 2-point spline's 'far' track: 250.9 away from a path 62.5 long).  It allows |du| <= 2e-6 of the
    parameter range, which is relative to the path as it stands."""
    g = np.load(os.path.join(GOLDEN, "trajectory_closest_point.npz"))
    worst = 0.0
    for ci in range(int(g["n_cases"])):
        full = float(g["full_arc_length_%d" % ci])
        for ti in range(len(g["track_names_%d" % ci])):
            worst = max(worst, D_TOL_CATMULL_ROM * max(1.0, float(g["distance_%d_%d" % (ci, ti)].max())) / full)
    assert abs(worst - 4.011e-6) < 1e-9, worst
    return 2.0 * U_TOL_CATMULL_ROM, 2.0 * worst * full_arc_length


@pytest.mark.parametrize("spline_type,n_points", CURVES)
def test_polynomials_reproduce_the_references_points_and_arc_lengths(golden, spline_type, n_points):
    key = "%d_%d" % (spline_type, n_points)
    cps = golden["control_points_" + key]
    poly = trajectory_polynomials_host(cps, spline_type)
    n_seg = trajectory_segment_count(n_points, spline_type)
    assert n_seg == (n_points - 3 if spline_type == 1 else n_points - 1) and poly.shape == (n_seg * 12 + 3,)
    us = golden["parameters_" + key]
    breaks = np.linspace(0.0, 1.0, n_seg + 1)[1:-1]
    assert us[0] == 0.0 and us[1] == 1.0 and all(b in us and np.nextafter(b, 0.0) in us and np.nextafter(b, 1.0) in us for b in breaks)
    pts = np.stack([polynomial_point(poly, u) for u in us])
    e_pts = float(np.abs(pts - golden["points_" + key]).max())
    # the ends are the end control points themselves (b_spline.py:134-137; the fitted spline interpolates)
    np.testing.assert_array_equal(polynomial_point(poly, 1.0), cps[-1])
    assert np.abs(polynomial_point(poly, 0.0) - cps[0]).max() <= BOUND
    arcs, full = arc_length_table_host(poly, 1000)
    e_full = abs(full - float(golden["full_arc_length_" + key]))
    assert arcs[0] == 0.0 and arcs[-1] == 1.0 and (np.diff(arcs) >= 0.0).all()
    by_arc = np.stack([point_by_arc_length_host(poly, arcs, full, a) for a in golden["arc_lengths_" + key]])
    e_arc = float(np.abs(by_arc - golden["points_by_arc_" + key]).max())
    np.testing.assert_array_equal(by_arc[3], cps[-1])                      # 1.25 x the full length: the last control point
    print("type %d, %d points: |points| %.3e  |full arc length| %.3e  |points by arc length| %.3e  (bound %.3e, largest coordinate %.1f)" % (
        spline_type, n_points, e_pts, e_full, e_arc, BOUND, np.abs(cps).max()))
    assert max(e_pts, e_full, e_arc) <= BOUND, (e_pts, e_full, e_arc)
    assert BOUND <= 1.0e-9 * np.abs(cps).max()


def test_the_pieces_the_issue_names():
    """n_points = 4: type 1 is ONE Bezier piece on the four control points, type 2 one cubic on three pieces; type 2's first two
    and last two pieces are the same cubic re-expanded (not-a-knot), its pieces pass through the data."""
    rng = np.random.default_rng(3)
    P = np.cumsum(rng.uniform(-30, 50, (4, 3)), axis=0)
    A = trajectory_polynomials_host(P, 1)[:12].reshape(4, 3)
    bezier = np.array([-P[0] + 3 * P[1] - 3 * P[2] + P[3], 3 * P[0] - 6 * P[1] + 3 * P[2], -3 * P[0] + 3 * P[1], P[0]])
    np.testing.assert_allclose(A, bezier, rtol=0, atol=1e-12)

    def shifted(piece):          # the cubic of `piece` (powers 3..0 of t) re-expanded in t + 1
        a, b, c, d = piece
        return np.array([a, 3 * a + b, 3 * a + 2 * b + c, a + b + c + d])
    for n in (4, 5, 9):
        Q = np.cumsum(rng.uniform(-30, 50, (n, 3)), axis=0)
        pieces = trajectory_polynomials_host(Q, 2)[:-3].reshape(n - 1, 4, 3)
        np.testing.assert_allclose(shifted(pieces[0]), pieces[1], rtol=0, atol=1e-11)
        np.testing.assert_allclose(shifted(pieces[-2]), pieces[-1], rtol=0, atol=1e-11)
        np.testing.assert_array_equal(pieces[:, 3], Q[:-1])
        np.testing.assert_allclose(pieces.sum(axis=1), Q[1:], rtol=0, atol=1e-11)
        if n == 4:
            np.testing.assert_allclose(shifted(pieces[1]), pieces[2], rtol=0, atol=1e-11)
        else:                    # a real knot at the third site: the third derivative jumps there for generic data
            assert np.abs(pieces[1][0] - pieces[2][0]).max() > 1e-6


def test_type_0_is_the_catmull_rom_spline_the_existing_fixture_pins():
    """One statement for all three types: type 0 of trajectory_polynomials_host against tests/golden/trajectory_spline.npz at the bound
    that fixture's own test uses (tests/test_oracle_golden.py: 1e-9), and equal to the oracle's Catmull-Rom point."""
    from oracle import mg_oracle as orc
    g = np.load(os.path.join(GOLDEN, "trajectory_spline.npz"))
    for ci in range(int(g["n_cases"])):
        cps = g["control_points_%d" % ci]
        poly = trajectory_polynomials_host(cps, 0)
        assert poly.shape == ((len(cps) - 1) * 12 + 3,)
        pts = np.stack([polynomial_point(poly, u) for u in g["parameters_%d" % ci]])
        np.testing.assert_allclose(pts, g["points_%d" % ci], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(pts, np.stack([orc.catmull_rom_point(cps, u) for u in g["parameters_%d" % ci]]), rtol=0, atol=1e-11)
        arcs, full = arc_length_table_host(poly, 1000)
        assert abs(full - float(g["full_arc_length_%d" % ci])) <= 1e-9 * full
        by_arc = np.stack([point_by_arc_length_host(poly, arcs, full, a) for a in g["arc_lengths_%d" % ci]])
        np.testing.assert_allclose(by_arc, g["points_by_arc_%d" % ci], rtol=1e-9, atol=1e-9)
    assert np.array_equal(trajectory_polynomials_host(cps), poly)          # the default type is 0


@pytest.mark.parametrize("spline_type,n_points", CURVES)
def test_the_statements_search_is_the_references_search(golden, spline_type, n_points):
    """The oracle's one-variable L-BFGS-B on the statement's polynomials against the reference's own find_closest_point_fast: the
    pairing the GPU test holds the device to.  A case counts as another basin where the parameters differ by more than one cell of
    the granularity-1000 grid; at most 5 % may (the generator chose the targets so that none does)."""
    from oracle import mg_oracle as orc
    key = "%d_%d" % (spline_type, n_points)
    poly = trajectory_polynomials_host(golden["control_points_" + key], spline_type)
    u_tol, d_tol = closest_point_bounds(float(golden["full_arc_length_" + key]))
    worst_u = worst_d = 0.0
    other = 0
    n = len(golden["cp_u_" + key])
    assert n == 48 and set(golden["cp_min_u_" + key]) == {0.0, 0.3}
    for tg, min_u, u_ref, d_ref in zip(golden["cp_targets_" + key], golden["cp_min_u_" + key], golden["cp_u_" + key], golden["cp_distance_" + key]):
        def dist(x):
            v = polynomial_point(poly, x) - tg
            return math.sqrt(float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
        u = orc.lbfgsb_1d(dist, float(min_u), float(min_u), 1.0, formk_rule=True)
        if abs(u - u_ref) > 1.0e-3:
            other += 1
            continue
        worst_u, worst_d = max(worst_u, abs(u - u_ref)), max(worst_d, abs(dist(u) - d_ref))
    print("type %d, %d points: |du| %.3e (bound %.1e)  |dd| %.3e (bound %.3e)  other basin %d of %d" % (spline_type, n_points, worst_u, u_tol, worst_d, d_tol, other, n))
    assert other <= 0.05 * n and worst_u <= u_tol and worst_d <= d_tol


# ---- the seam: reference-shaped objects ----------------------------------------------------------------------------------------------
class _BSpline(object):                   # b_spline.py:46-59
    def __init__(self, points):
        self.points = np.array(points)
        self.degree, self.domain, self.dimensions = 3, (0.0, 1.0), 3
        inner = np.linspace(0.0, 1.0, len(points) - 2).tolist()
        self.knots = inner[:1] * 3 + inner + inner[-1:] * 3


class _FittedBSpline(object):             # fitted_b_spline.py:29-47
    def __init__(self, points):
        self.points = np.array(points)
        self.degree, self.domain, self.dimensions = 1, (0.0, 1.0), 3
        self.spline_def = [None, None, None]


class _CatmullRom(object):                # catmull_rom_spline.py:50-71
    def __init__(self, points):
        self._catmullrom_basematrix = np.zeros((4, 4))
        self.control_points = [points[0]] + list(points) + [points[-1], points[-1]]


class _TrajectoryConstraint(object):      # trajectory_constraint.py:33-52
    constraint_type = "trajectory"

    def __init__(self, spline, joint_name="Hips", root="Hips"):
        self.spline, self.granularity, self.full_arc_length, self.min_arc_length = spline, 500, 200.0, 50.0
        self.joint_name, self.weight_factor = joint_name, 2.0
        self.skeleton = type("S", (), {"root": root})()


POINTS = [[0.0, 1.0, 2.0], [10.0, 0.0, 5.0], [20.0, -1.0, 3.0], [30.0, 2.0, -4.0], [45.0, 0.5, 1.0]]


@pytest.mark.parametrize("cls,spline_type", [(_BSpline, 1), (_FittedBSpline, 2)])
def test_device_form_of_reference_shaped_typed_trajectories(cls, spline_type):
    """trajectory_to_device_form and _spline_control_points on a B-spline and a fitted B-spline object: the type and the control
    points as they are (no padding to undo)."""
    c = _TrajectoryConstraint(cls(POINTS))
    d = trajectory_to_device_form(c, group=3)
    assert d == {"type": "trajectory", "control_points": POINTS, "min_u": 0.25, "weight": 2.0, "granularity": 500, "group": 3, "spline_type": spline_type}
    assert _spline_control_points(c) == {"control_points": POINTS, "granularity": 500, "spline_type": spline_type}
    # another joint than the root: the per-frame kind, the type carried along
    hand = trajectory_to_device_form(_TrajectoryConstraint(cls(POINTS), joint_name="LeftHand"), group=0)
    assert hand["type"] == "frame_joint_trajectory" and hand["spline_type"] == spline_type and hand["control_points"] == POINTS
    # ... and through the list conversion, a local trajectory included
    local = type("L", (), {"constraint_type": "local_trajectory", "trajectory": c, "joint_name": "Hips", "start_t": 1.5, "n_canonical_frames": 7, "weight_factor": 1.0})()
    forms = constraints_to_device_form([c, local])
    assert forms[0] == dict(d, group=0) and forms[1]["type"] == "frame_local_trajectory" and forms[1]["spline_type"] == spline_type
    from morphablegraphs_amd.candidate_scoring import trajectory_record
    assert trajectory_record(forms[1]) == {"type": "trajectory", "control_points": POINTS, "granularity": 500, "spline_type": spline_type}


def test_a_catmull_rom_device_form_is_what_it_was():
    """no "spline_type" key for type 0: existing dicts and cache keys compare equal to the ones made before the types existed"""
    c = _TrajectoryConstraint(_CatmullRom(POINTS))
    d = trajectory_to_device_form(c, group=1)
    assert d == {"type": "trajectory", "control_points": POINTS, "min_u": 0.25, "weight": 2.0, "granularity": 500, "group": 1}
    assert _spline_control_points(c) == {"control_points": POINTS, "granularity": 500}
    from morphablegraphs_amd.candidate_scoring import trajectory_record
    assert trajectory_record(dict(d, spline_type=0)) == {"type": "trajectory", "control_points": POINTS, "granularity": 500}
    with pytest.raises(NotImplementedError):
        trajectory_to_device_form(_TrajectoryConstraint(object()))


def test_the_cache_key_carries_the_type(monkeypatch):
    """cached_trajectory: the same control points under another type are another device object; type 0's key is the old one"""
    from morphablegraphs_amd import _capi, candidate_scoring as cs
    made = []

    class FakeTrajectory(object):
        def __init__(self, prim, cps, granularity=1000, spline_type=0):
            self.handle, self.args = True, (granularity, spline_type)
            made.append(self)

        def close(self):
            self.handle = None
    monkeypatch.setattr(_capi, "Trajectory", FakeTrajectory)
    monkeypatch.setattr(cs, "_TRAJ_CACHE", [])
    prim = type("P", (), {"serial": 1, "handle": type("H", (), {"value": 11})()})()
    base = {"type": "trajectory", "control_points": POINTS, "granularity": 300}
    t0 = cached_trajectory(prim, base)
    t1 = cached_trajectory(prim, dict(base, spline_type=1))
    t2 = cached_trajectory(prim, dict(base, spline_type=2))
    assert [t.args for t in made] == [(300, 0), (300, 1), (300, 2)]
    assert cached_trajectory(prim, dict(base, spline_type=0)) is t0 and cached_trajectory(prim, dict(base, spline_type=1)) is t1
    assert cached_trajectory(prim, dict(base, spline_type=2)) is t2 and len(made) == 3
    assert cs._TRAJ_CACHE[0][0] == (1, 11, cs._freeze(POINTS), 300)


def test_refusals():
    """n_points = 3 for types 1 and 2, an unknown type, points that are not (n, 3) or not finite: ValueError, as the library's
    MG_ERR_INVALID_ARGUMENT (tests/test_gpu_spline_types.py)"""
    three = POINTS[:3]
    for spline_type in (1, 2):
        with pytest.raises(ValueError, match=">= 4 control points"):
            trajectory_polynomials_host(three, spline_type)
        assert trajectory_polynomials_host(POINTS[:4], spline_type).shape == ((1 if spline_type == 1 else 3) * 12 + 3,)
    assert trajectory_polynomials_host(three, 0).shape == (2 * 12 + 3,)
    for bad in (3, -1, None):
        with pytest.raises(ValueError, match="unknown spline type"):
            trajectory_polynomials_host(POINTS, bad)
    with pytest.raises(ValueError):
        trajectory_polynomials_host([[0.0, 1.0]] * 5, 1)
    with pytest.raises(ValueError):
        trajectory_polynomials_host([[0.0, 1.0, float("nan")]] * 5, 2)
    assert st.SPLINE_TYPES == (0, 1, 2)
