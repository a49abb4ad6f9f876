"""The arc-length queries on the device (csrc/mg_trajectory_arc.hip) against their NumPy statements bit for bit
(morphablegraphs_amd/spline_types.py), and against the reference's own numbers (tests/golden/trajectory_arc_queries.npz) to the
tolerances tests/test_trajectory_arc_host.py states.

Shapes: batches of 1, 63, 64, 65 and 257 points (a wave's edge, the eight points of a workgroup, more than one workgroup),
granularities 7, 64, 65 and 1000 (fewer parameters than a wave has lanes, a full stride, a one-parameter tail, the reference's
default), the three spline types with one piece and with many, and a table that leaves LDS for global memory.
"""
import types

import numpy as np
import pytest

from conftest import load_golden
from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import spline_types as st
from morphablegraphs_amd.trajectory_queries import advance_along_trajectory, goals_along_trajectory
from test_trajectory_arc_host import (ANGLE_ATOL, ARC_RTOL, POINT_ATOL, TANGENT_ATOL, TIE_CPS, TIE_GRANULARITY, TIE_K, tie_point)

pytestmark = pytest.mark.gpu
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def prim(ctx):
    p = _capi.Primitive(ctx, synthetic.make_tiny_primitive())
    yield p
    p.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _path(n_points, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(np.column_stack([rng.uniform(20, 60, n_points), rng.uniform(-4, 4, n_points), rng.uniform(-40, 40, n_points)]), axis=0)


def _host_tables(cps, spline_type, granularity):
    poly = st.trajectory_polynomials_host(cps, spline_type)
    arcs, full = st.arc_length_table_host(poly, granularity)
    return poly, arcs, full, st.sample_parameters_host(granularity)


def _scan(ctx, traj, points, min_arc):
    """mg_trajectory_arc_length_of_points with the point rows pre-filled with SENTINEL: (arc, points, index)"""
    n = len(points)
    with ctx.buffers() as bufs:
        d_p, d_o, d_i = bufs.upload(points), bufs.malloc(n * 8), bufs.malloc(n * 4)
        d_q = bufs.upload(np.full((n, 3), SENTINEL))
        d_m = None if min_arc is None else bufs.upload(np.ascontiguousarray(min_arc, dtype=np.float64))
        traj.arc_length_of_points_dev(d_p, n, d_o, d_m, d_q, d_i)
        return ctx.download(d_o, (n,), np.float64), ctx.download(d_q, (n, 3), np.float64), ctx.download(d_i, (n,), np.int32)


def _host_scan(poly, arcs, full, us, points, min_arc):
    arc, pts, idx = np.empty(len(points)), np.full((len(points), 3), SENTINEL), np.empty(len(points), dtype=np.int32)
    for i, p in enumerate(points):
        arc[i], q, idx[i] = st.arc_length_of_point_host(poly, arcs, full, p, 0.0 if min_arc is None else min_arc[i], us)
        if q is not None:
            pts[i] = q
    return arc, pts, idx


CURVES = [(0, 4), (1, 4), (2, 4), (0, 12), (1, 12), (2, 12)]        # (spline type, control points): type 1 with 4 points is ONE piece
BATCHES = {7: (257, 65, 1, 63, 64, 257), 64: (257, 64, 65, 1, 63, 257), 65: (65, 257, 64, 63, 1, 65), 1000: (1, 63, 64, 65, 63, 64)}


@pytest.mark.parametrize("granularity", sorted(BATCHES))
def test_arc_length_of_points_has_the_host_statements_bits(ctx, prim, granularity):
    """Every curve at this granularity, batch sizes across the wave and workgroup edges, min_arc_length 0 / mid-path / exactly a
    sample's arc length (strict >) / the full length and above (-1, the point's row untouched); two calls give the same bytes."""
    rng = np.random.default_rng(100 + granularity)
    seen_none = seen_strict = 0
    for (spline_type, n_cp), n in zip(CURVES, BATCHES[granularity]):
        cps = _path(n_cp, 40 + n_cp + spline_type)
        poly, arcs, full, us = _host_tables(cps, spline_type, granularity)
        traj = _capi.Trajectory(prim, cps, granularity=granularity, spline_type=spline_type)
        try:
            d_poly, d_arcs, d_full = traj.tables()
            assert np.array_equal(_bits(d_poly), _bits(poly)) and np.array_equal(_bits(d_arcs), _bits(arcs)) and d_full == full
            assert np.array_equal(_bits(traj.sample_parameters()), _bits(us))
            on = np.stack([st.polynomial_point(poly, u) for u in rng.uniform(0.0, 1.0, n)])
            points = on + rng.normal(0.0, 0.03 * full, (n, 3)) * [1.0, 0.3, 1.0]
            k_entry = int(rng.integers(1, len(us) - 1))
            entry = st.absolute_arc_length_host(arcs, full, us[k_entry])
            points[0] = st.polynomial_point(poly, us[k_entry])                # ON a sample whose arc length is the bound: the next one wins
            choices = np.array([0.0, 0.45 * full, entry, full, 1.5 * full])
            min_arc = choices[np.arange(n) % 5] if n > 1 else np.array([entry])
            min_arc[0] = entry
            want = _host_scan(poly, arcs, full, us, points, min_arc)
            got = _scan(ctx, traj, points, min_arc)
            again = _scan(ctx, traj, points, min_arc)
            for g, w, a in zip(got, want, again):
                assert g.tobytes() == a.tobytes()
                assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), (spline_type, n_cp, n)
            assert got[2][0] == k_entry + 1 and got[0][0] > entry
            none = got[2] < 0
            assert np.array_equal(none, min_arc >= full) and np.all(got[0][none] == -1.0) and np.all(got[1][none] == SENTINEL)
            assert np.all(got[0][~none] > min_arc[~none])
            seen_none += int(none.sum())
            seen_strict += 1
            # no bound at all is a bound of 0
            zero = _scan(ctx, traj, points[:8], None)
            for g, w in zip(zero, _host_scan(poly, arcs, full, us, points[:8], None)):
                assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
        finally:
            traj.close()
    assert seen_none > 0 and seen_strict == len(CURVES)


def test_the_smaller_index_wins_a_tie_whatever_the_order(ctx, prim):
    """Samples TIE_K and TIE_K + 1 at exactly the same distance (a straight piece, a point on their bisector): the first, in every
    position of a batch -- the two samples sit in neighbouring lanes of one stride -- and the same bytes from call to call."""
    poly, arcs, full, us = _host_tables(np.array(TIE_CPS), 0, TIE_GRANULARITY)
    q = tie_point(poly, us)
    traj = _capi.Trajectory(prim, np.array(TIE_CPS), granularity=TIE_GRANULARITY)
    try:
        points = np.tile(q, (65, 1))
        first = _scan(ctx, traj, points, None)
        assert np.all(first[2] == TIE_K)
        assert first[0].tobytes() == _host_scan(poly, arcs, full, us, points[:1], None)[0].repeat(65).tobytes()
        second = _scan(ctx, traj, points, None)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
        # with the first of the two ruled out by the bound the second is the minimum
        bound = np.full(65, st.absolute_arc_length_host(arcs, full, us[TIE_K]))
        assert np.all(_scan(ctx, traj, points, bound)[2] == TIE_K + 1)
    finally:
        traj.close()


def _query(traj, arcs_q, ref_dir, eval_range=0.5):
    return traj.points_by_arc_length(arcs_q, tangents=True, reference_dir=ref_dir, eval_range=eval_range)


def _host_query(poly, arcs, full, arcs_q, ref_dir, eval_range=0.5):
    rows = [st.angle_at_arc_length_2d_host(poly, arcs, full, a, ref_dir, eval_range) for a in arcs_q]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows])


@pytest.mark.parametrize("spline_type,n_cp", CURVES)
def test_points_tangents_and_angles_have_the_host_statements_bits(ctx, prim, spline_type, n_cp):
    """Arc lengths at 0, near 0 and near the end (the chord's clamped ends), the full length, above it (the widening runs), a negative
    one and seeded ones, for batches of 1, 63, 64, 65 and 257."""
    cps = _path(n_cp, 40 + n_cp + spline_type)
    poly, arcs, full, _ = _host_tables(cps, spline_type, 1000)
    ref_dir = (0.1, 1.0)
    rng = np.random.default_rng(7)
    edge = [0.0, 0.2, 0.5, full - 0.2, full, full + 0.3, full + 2.55, -1.0, 0.5 * full]
    traj = _capi.Trajectory(prim, cps, granularity=1000, spline_type=spline_type)
    try:
        for n in (1, 63, 64, 65, 257):
            arcs_q = np.array((edge + list(rng.uniform(0.0, full, 257)))[:n]) if n > 1 else np.array([full + 2.55])
            got, want = _query(traj, arcs_q, ref_dir), _host_query(poly, arcs, full, arcs_q, ref_dir)
            for g, w in zip(got, want):
                assert np.array_equal(_bits(g), _bits(w)), (n, np.flatnonzero((_bits(g) != _bits(w)).reshape(n, -1).any(axis=1))[:5])
            assert np.allclose(np.linalg.norm(got[1], axis=1), 1.0, rtol=0, atol=1e-15)
        # points alone, and another eval_range
        only = traj.points_by_arc_length(np.array(edge))
        assert np.array_equal(_bits(only), _bits(_host_query(poly, arcs, full, edge, ref_dir)[0]))
        assert np.array_equal(only[5], cps[-1]) and np.array_equal(only[6], cps[-1])         # above the full length: the last control point
        got, want = _query(traj, np.array(edge), ref_dir, 1.25), _host_query(poly, arcs, full, edge, ref_dir, 1.25)
        assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))
    finally:
        traj.close()


def test_tangent_widening_on_a_doubled_control_point_and_its_bound(ctx, prim):
    """A path that starts with coinciding control points: both ends of the chord are the same point until eval_range has grown past
    the dead stretch's end.  A query a thousand units past the end exhausts the bound: MG_ERR_UNSUPPORTED for the call, NaN rows."""
    cps = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [40.0, 0.0, 30.0], [80.0, 0.0, 0.0]])
    poly, arcs, full, _ = _host_tables(cps, 0, 1000)
    traj = _capi.Trajectory(prim, cps, granularity=1000)
    try:
        # past the end by 1: the range is widened from 0.5 until it exceeds 1 (both ends are the last control point before)
        arcs_q = np.array([full + 1.0, full + 7.3, 0.0, 0.05, full])
        got = _query(traj, arcs_q, (0.0, 1.0), 0.5)
        want = _host_query(poly, arcs, full, arcs_q, (0.0, 1.0), 0.5)
        assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))
        p1 = st.point_by_arc_length_host(poly, arcs, full, full + 1.0 - 0.5)
        p2 = st.point_by_arc_length_host(poly, arcs, full, full + 1.0 + 0.5)
        assert np.array_equal(p1, p2)                     # the first chord is degenerate: the loop ran
        with pytest.raises(_capi.MGError) as err:
            _query(traj, np.array([1.0, full + 1000.0]), (0.0, 1.0))
        assert err.value.status == _capi.MG_ERR_UNSUPPORTED
        with pytest.raises(st.TangentWideningExhausted):
            st.tangent_at_arc_length_host(poly, arcs, full, full + 1000.0)
        assert np.array_equal(traj.points_by_arc_length(np.array([full + 1000.0]))[0], cps[-1])       # the point alone needs no chord
    finally:
        traj.close()


def test_against_the_references_numbers(ctx, prim):
    g = load_golden("trajectory_arc_queries")
    ref_dir = tuple(g["reference_dir"])
    total = left_out = 0
    for t in g["spline_types"]:
        for n in g["n_points"]:
            key = "%d_%d" % (t, n)
            traj = _capi.Trajectory(prim, g["control_points_" + key], granularity=1000, spline_type=int(t))
            try:
                np.testing.assert_allclose(traj.tables()[2], float(g["full_arc_length_" + key]), rtol=ARC_RTOL)
                pts, tans, angs = _query(traj, g["arcs_" + key], ref_dir)
                np.testing.assert_allclose(pts, g["points_by_arc_" + key], rtol=0, atol=POINT_ATOL, err_msg=key)
                np.testing.assert_allclose(tans, g["tangents_" + key], rtol=0, atol=TANGENT_ATOL, err_msg=key)
                np.testing.assert_allclose(angs, g["angles_" + key], rtol=0, atol=ANGLE_ATOL, err_msg=key)
                arc, point, idx = traj.arc_length_of_points(g["q_points_" + key], g["q_min_arc_" + key])
                want_idx, amb = g["q_min_index_" + key], g["q_ambiguous_" + key]
                total, left_out = total + len(idx), left_out + int(amb.sum())
                keep = ~amb
                assert np.array_equal(idx[keep], want_idx[keep]), key
                found = keep & (want_idx >= 0)
                np.testing.assert_allclose(arc[found], g["q_arc_" + key][found], rtol=ARC_RTOL, err_msg=key)
                np.testing.assert_allclose(point[found], g["q_min_point_" + key][found], rtol=0, atol=POINT_ATOL, err_msg=key)
                assert np.all(arc[want_idx < 0] == -1.0) and np.isnan(point[want_idx < 0]).all() and (want_idx < 0).any()
            finally:
                traj.close()
    assert left_out <= 0.02 * total


@pytest.mark.parametrize("granularity,in_lds", [(4000, True), (4100, False)])
def test_tables_in_lds_and_in_global_memory_give_the_statements_bits(ctx, prim, granularity, in_lds):
    """12 control points (135 doubles of pieces) with 4001 + 4001 table entries are 65 096 bytes: the last size that fits the 64 KiB
    of LDS; with 4101 + 4101 (66 696 bytes) the kernel reads global memory.  Both against the host statement."""
    cps = _path(12, 52)
    poly, arcs, full, us = _host_tables(cps, 0, granularity)
    assert ((len(poly) + len(arcs) + len(us)) * 8 <= 64 * 1024) == in_lds
    rng = np.random.default_rng(5)
    points = np.stack([st.polynomial_point(poly, u) for u in rng.uniform(0, 1, 9)]) + rng.normal(0.0, 0.03 * full, (9, 3))
    min_arc = np.array([0.0, 0.3 * full, full] * 3)
    traj = _capi.Trajectory(prim, cps, granularity=granularity)
    try:
        for g, w in zip(_scan(ctx, traj, points, min_arc), _host_scan(poly, arcs, full, us, points, min_arc)):
            assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
    finally:
        traj.close()


def test_advance_along_trajectory_is_the_loop_of_its_pieces(ctx, prim):
    """65 walks: the batch against a Python loop of mg_trajectory_closest_points' parameters, the curve's point (no further than the
    window's end) and the host statement of the arc length, -1 replaced by the full length.  Walk 3 stands past the end of the path,
    walk 4 has the whole path behind it (the -1 rule), walk 5's closest point lies beyond its window."""
    cps = _path(9, 61)
    poly, arcs, full, us = _host_tables(cps, 0, 1000)
    traj = _capi.Trajectory(prim, cps, granularity=1000)
    rng = np.random.default_rng(11)
    n, look_ahead = 65, 80.0
    try:
        at = rng.uniform(0.3, 0.9, n)
        positions = np.stack([st.polynomial_point(poly, u) for u in at]) + rng.normal(0.0, 4.0, (n, 3)) * [1.0, 0.2, 1.0]
        travelled = np.array([st.absolute_arc_length_host(arcs, full, u) for u in at]) - rng.uniform(5.0, 40.0, n)
        travelled[:3] = travelled.min()
        positions[3] = cps[-1] + [30.0, 0.0, 5.0]
        travelled[3] = 0.9 * full
        travelled[4] = full
        travelled[5], positions[5] = 0.25 * full, st.polynomial_point(poly, 0.95)
        got = advance_along_trajectory(traj, positions, travelled, look_ahead)
        u_lo = st.parameter_by_arc_length_host(arcs, full, travelled.min())
        params, _ = prim.trajectory_closest_points(traj, positions[:, None, :], min_u=u_lo)
        want = np.empty(n)
        fired = 0
        for i in range(n):
            u_hi = st.parameter_by_arc_length_host(arcs, full, travelled[i] + look_ahead)
            u = min(params[i, 0], 1.0 if u_hi is None else u_hi)
            arc = st.arc_length_of_point_host(poly, arcs, full, st.polynomial_point(poly, min(1.0, max(0.0, u))), travelled[i], us)[0]
            fired += arc == -1.0
            want[i] = full if arc == -1.0 else arc
        assert np.array_equal(_bits(got), _bits(want))
        assert fired >= 1 and got[4] == full and np.all(got >= np.minimum(travelled, full))
        assert got[5] <= st.absolute_arc_length_host(arcs, full, 1.0) and got[5] < 0.25 * full + look_ahead + 1.0
        # device positions give the same bytes; so does a walk whose last frame is on the device
        d_pos = ctx.upload(positions)
        try:
            assert advance_along_trajectory(traj, d_pos, travelled, look_ahead, n=n).tobytes() == got.tobytes()
        finally:
            d_pos.free()
        from morphablegraphs_amd.graph_walk import HipGraphWalk
        walk = HipGraphWalk(types.SimpleNamespace(nodes={}), ctx=ctx)
        frames = np.zeros((3, 7))
        frames[:, 3] = 1.0
        frames[:, :3] = positions[6:9]
        walk.append_quat_frames(frames)
        try:
            last = walk.get_quat_frames()[-1, :3]
            one = advance_along_trajectory(traj, last[None, :], travelled[8], look_ahead)[0]
            assert walk.advance_along_trajectory(traj, travelled[8], look_ahead) == one
        finally:
            walk.close()
        goals = goals_along_trajectory(traj, travelled[:5], look_ahead, with_orientation=True, half_step=True)
        hp, ht, _ = _host_query(poly, arcs, full, travelled[:5] + look_ahead, (0.0, 1.0))
        assert np.array_equal(_bits(goals["positions"]), _bits(hp)) and np.array_equal(_bits(goals["tangents"]), _bits(ht))
        half = np.array([st.point_by_arc_length_host(poly, arcs, full, a) for a in travelled[:5] + look_ahead / 2])
        assert np.array_equal(_bits(goals["half_positions"]), _bits(half))
    finally:
        traj.close()


def test_misuse_is_reported_like_the_neighbouring_entry_points(ctx, prim):
    cps = _path(5, 3)
    traj = _capi.Trajectory(prim, cps, granularity=64)
    other_ctx = _capi.Context(0)
    other = _capi.Primitive(other_ctx, synthetic.make_tiny_primitive())
    other_traj = _capi.Trajectory(other, cps, granularity=64)
    lib, bad = prim.lib, _capi.MG_ERR_INVALID_ARGUMENT
    d = ctx.upload(np.zeros(24))
    try:
        p, t, ot = prim.handle, traj.handle, other_traj.handle
        # n == 0: MG_OK, nothing launched, no pointer looked at
        assert lib.mg_trajectory_points_by_arc_length(p, t, None, 0, 0.5, None, None, None, None) == 0
        assert lib.mg_trajectory_arc_length_of_points(p, t, None, None, 0, None, None, None) == 0
        assert lib.mg_trajectory_points_at_parameters(p, t, None, None, 0, None) == 0
        # NULL handles and pointers, a negative count, a trajectory of another context's primitive
        assert lib.mg_trajectory_points_by_arc_length(None, t, d.ptr, 1, 0.5, d.ptr, None, None, None) == bad
        assert lib.mg_trajectory_points_by_arc_length(p, None, d.ptr, 1, 0.5, d.ptr, None, None, None) == bad
        assert lib.mg_trajectory_points_by_arc_length(p, ot, d.ptr, 1, 0.5, d.ptr, None, None, None) == bad
        assert lib.mg_trajectory_points_by_arc_length(p, t, None, 1, 0.5, d.ptr, None, None, None) == bad
        assert lib.mg_trajectory_points_by_arc_length(p, t, d.ptr, 1, 0.5, None, None, None, None) == bad
        assert lib.mg_trajectory_points_by_arc_length(p, t, d.ptr, 1, 0.5, None, None, d.ptr, None) == bad      # an angle without a reference
        assert lib.mg_trajectory_points_by_arc_length(p, t, d.ptr, -1, 0.5, d.ptr, None, None, None) == bad
        assert lib.mg_trajectory_points_by_arc_length(p, t, d.ptr, 1, float("nan"), d.ptr, None, None, None) == bad
        assert lib.mg_trajectory_arc_length_of_points(p, ot, d.ptr, None, 1, d.ptr, None, None) == bad
        assert lib.mg_trajectory_arc_length_of_points(p, t, None, None, 1, d.ptr, None, None) == bad
        assert lib.mg_trajectory_arc_length_of_points(p, t, d.ptr, None, 1, None, None, None) == bad
        assert lib.mg_trajectory_arc_length_of_points(None, t, d.ptr, None, 1, d.ptr, None, None) == bad
        assert lib.mg_trajectory_points_at_parameters(p, ot, d.ptr, None, 1, d.ptr) == bad
        assert lib.mg_trajectory_points_at_parameters(p, t, None, None, 1, d.ptr) == bad
        assert lib.mg_trajectory_sample_parameters(None, None, None) == bad
        # the other context's own trajectory works on its own primitive
        assert np.array_equal(_bits(other_traj.points_by_arc_length(np.array([3.0]))), _bits(traj.points_by_arc_length(np.array([3.0]))))
        # a point with a non-finite coordinate qualifies nowhere; a non-finite arc length gives NaN rows
        arc, pts, idx = _scan(ctx, traj, np.array([[np.nan, 0.0, 0.0], cps[1]]), None)
        assert arc[0] == -1.0 and idx[0] == -1 and np.all(pts[0] == SENTINEL) and idx[1] >= 0
        assert np.isnan(traj.points_by_arc_length(np.array([np.inf, 1.0]))[0]).all()
    finally:
        d.free()
        for h in (other_traj, other, other_ctx, traj):
            h.close()
