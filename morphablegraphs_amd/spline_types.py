"""The three curves of the reference's ParameterizedSpline (constraints/spatial_constraints/splines/parameterized_spline.py:53-63)
as ONE table of cubic pieces: the host statement of what mg_trajectory_create_typed builds (csrc/mg_trajectory.hip) and what
every trajectory kernel reads.

All three are piecewise cubic in u over [0, 1] on a UNIFORM grid of n_seg pieces:
  0  CatmullRomSpline   n_seg = n_points - 1   (catmull_rom_spline.py:66-71, 118-168)
  1  BSpline            n_seg = n_points - 3   clamped cubic, n_points - 2 uniform knot values (b_spline.py:70-105), de Boor
  2  FittedBSpline      n_seg = n_points - 1   FITPACK splrep(linspace(0, 1, n_points), values, k=3), s = 0: the interpolating cubic
                                               with not-a-knot ends (fitted_b_spline.py:44-47)
Layout (mg_trajectory's `poly`): (n_seg * 12 + 3,) float64 -- per piece [power 3, 2, 1, 0][x, y, z] of the piece's LOCAL parameter
t = n_seg u - floor(n_seg u), point(t) = ((A0 t + A1) t + A2) t + A3; then the last control point, returned for n_seg u >= n_seg.

Pure Python floats in the statement order of the C++ (which is compiled without contraction): the device table is expected to
equal this one bit for bit.  Needs NumPy only -- no library, no GPU."""
import math

import numpy as np

SPLINE_TYPE_CATMULL_ROM = 0
SPLINE_TYPE_BSPLINE = 1
SPLINE_TYPE_FITTED_BSPLINE = 2
SPLINE_TYPES = (SPLINE_TYPE_CATMULL_ROM, SPLINE_TYPE_BSPLINE, SPLINE_TYPE_FITTED_BSPLINE)
MIN_POINTS = {SPLINE_TYPE_CATMULL_ROM: 2, SPLINE_TYPE_BSPLINE: 4, SPLINE_TYPE_FITTED_BSPLINE: 4}

_CATMULL_ROM_BASE = ((-1.0, 3.0, -3.0, 1.0), (2.0, -5.0, 4.0, -1.0), (-1.0, 0.0, 1.0, 0.0), (0.0, 2.0, 0.0, 0.0))


def trajectory_segment_count(n_points, spline_type):
    """n_seg of the table for n_points control points; ValueError where mg_trajectory_create_typed returns MG_ERR_INVALID_ARGUMENT"""
    if spline_type not in SPLINE_TYPES:
        raise ValueError("unknown spline type %r (0 Catmull-Rom, 1 B-spline, 2 fitted B-spline)" % (spline_type,))
    if n_points < MIN_POINTS[spline_type]:
        raise ValueError("spline type %d needs >= %d control points (got %d)" % (spline_type, MIN_POINTS[spline_type], n_points))
    return n_points - 3 if spline_type == SPLINE_TYPE_BSPLINE else n_points - 1


def _checked_points(control_points):
    cp = np.asarray(control_points, dtype=np.float64)
    if cp.ndim != 2 or cp.shape[1] != 3:
        raise ValueError("control_points must be (n, 3)")
    if not np.isfinite(cp).all():
        raise ValueError("control points must be finite")
    return [[float(v) for v in p] for p in cp]


def _catmull_rom(cp, n_seg, poly):
    n = len(cp)
    pad = [cp[0]] + cp + [cp[n - 1], cp[n - 1]]
    for s in range(n_seg):
        for r in range(4):
            for d in range(3):
                v = 0.0
                for j in range(4):
                    v += _CATMULL_ROM_BASE[r][j] * pad[s + j][d]
                poly[s * 12 + r * 3 + d] = 0.5 * v


def _b_spline(cp, n_seg, poly):
    """de Boor's recurrence (b_spline.py:174-188) carried out on polynomials in the piece's local parameter.  In units of the knot
    spacing the knot vector is K_j = clamp(j - 3, 0, n_seg) -- integers -- and on piece s the parameter is s + t, so every weight
    alpha = (s + t - K_j) / (K_(j + 4 - r) - K_j) is a0 + a1 t with small rational a0, a1."""
    def knot(j):
        return float(min(max(j - 3, 0), n_seg))
    for s in range(n_seg):
        i = s + 3                                   # the knot span of the piece: K_i = s, K_(i + 1) = s + 1
        for d in range(3):
            c = [[cp[s + j][d], 0.0, 0.0, 0.0] for j in range(4)]          # c[j]: ascending powers of t, control point s + j
            for r in range(1, 4):
                for jj in range(3, r - 1, -1):      # j = i - 3 + jj, descending: c[jj - 1] is still the level before
                    j = i - 3 + jj
                    den = knot(j + 4 - r) - knot(j)
                    a0, a1 = (float(s) - knot(j)) / den, 1.0 / den
                    lo, hi = c[jj - 1], c[jj]
                    new = [(1.0 - a0) * lo[0] + a0 * hi[0], 0.0, 0.0, 0.0]
                    for k in range(1, 4):
                        new[k] = ((1.0 - a0) * lo[k] + a0 * hi[k]) + a1 * (hi[k - 1] - lo[k - 1])
                    c[jj] = new
            for r in range(4):
                poly[s * 12 + r * 3 + d] = c[3][3 - r]


def _fitted_b_spline(cp, n_seg, poly):
    """The interpolating cubic spline through the points at linspace(0, 1, n) with FITPACK's s = 0 knots (the data sites without the
    second and the last but one): the third derivative is continuous there -- not-a-knot.  Solved for the second derivatives M_i per
    unit spacing: M_(i-1) + 4 M_i + M_(i+1) = 6 (y_(i-1) - 2 y_i + y_(i+1)), and M_0 - 2 M_1 + M_2 = 0 turns the first row into
    M_1 = y_0 - 2 y_1 + y_2 (the last likewise): a tridiagonal system with 4 on the diagonal for M_2 .. M_(n-3), by elimination."""
    m = len(cp)
    for d in range(3):
        y = [cp[i][d] for i in range(m)]
        D2 = [0.0] * m
        for i in range(1, m - 1):
            D2[i] = (y[i + 1] - y[i]) - (y[i] - y[i - 1])
        M = [0.0] * m
        M[1], M[m - 2] = D2[1], D2[m - 2]
        if m >= 5:
            lo, hi = 2, m - 3
            cc, dd = [0.0] * m, [0.0] * m
            for i in range(lo, hi + 1):
                rhs = 6.0 * D2[i]
                if i == lo:
                    rhs -= M[1]
                if i == hi:
                    rhs -= M[m - 2]
                den = 4.0 if i == lo else 4.0 - cc[i - 1]
                cc[i] = 1.0 / den
                dd[i] = (rhs if i == lo else rhs - dd[i - 1]) / den
            M[hi] = dd[hi]
            for i in range(hi - 1, lo - 1, -1):
                M[i] = dd[i] - cc[i] * M[i + 1]
        M[0] = 2.0 * M[1] - M[2]
        M[m - 1] = 2.0 * M[m - 2] - M[m - 3]
        for s in range(n_seg):
            poly[s * 12 + 0 + d] = (M[s + 1] - M[s]) / 6.0
            poly[s * 12 + 3 + d] = 0.5 * M[s]
            poly[s * 12 + 6 + d] = (y[s + 1] - y[s]) - (2.0 * M[s] + M[s + 1]) / 6.0
            poly[s * 12 + 9 + d] = y[s]


def trajectory_polynomials_host(control_points, spline_type=SPLINE_TYPE_CATMULL_ROM):
    """The (n_seg * 12 + 3,) float64 table mg_trajectory_create_typed uploads for these control points (n, 3)."""
    cp = _checked_points(control_points)
    n_seg = trajectory_segment_count(len(cp), spline_type)
    poly = [0.0] * (n_seg * 12 + 3)
    (_catmull_rom, _b_spline, _fitted_b_spline)[spline_type](cp, n_seg, poly)
    for d in range(3):
        poly[n_seg * 12 + d] = cp[-1][d]
    return np.array(poly, dtype=np.float64)


def polynomial_point(poly, u):
    """mg_traj_point (csrc/mg_traj_device.h): the table's point at parameter u"""
    n_seg = (len(poly) - 3) // 12
    scaled = n_seg * float(u)
    index = int(math.floor(scaled))
    if index >= n_seg:
        return np.array([float(poly[n_seg * 12 + d]) for d in range(3)])
    t = scaled - index
    A = poly[index * 12:index * 12 + 12]
    return np.array([((float(A[d]) * t + float(A[3 + d])) * t + float(A[6 + d])) * t + float(A[9 + d]) for d in range(3)])


def arc_length_table_host(poly, granularity=1000):
    """(relative arc lengths (granularity + 1,), full arc length): RelativeArcLengthMap._update_table (arc_length_map.py:45-71) on the
    table's points, as mg_trajectory_create[_typed] builds it -- the same for every spline type."""
    arc = [0.0] * (granularity + 1)
    last, acc = polynomial_point(poly, 0.0), 0.0
    for k in range(1, granularity + 1):
        cur = polynomial_point(poly, k / float(granularity))
        x, y, z = float(cur[0] - last[0]), float(cur[1] - last[1]), float(cur[2] - last[2])
        acc += math.sqrt(x * x + y * y + z * z)
        arc[k] = acc
        last = cur
    if acc > 0.0:
        arc = [v / acc for v in arc]
    return np.array(arc, dtype=np.float64), acc


def point_by_arc_length_host(poly, arcs, full, arc):
    """mg_fc_point_by_arc (csrc/mg_frame_constraints.hip): ParameterizedSpline.query_point_by_absolute_arc_length
    (parameterized_spline.py:131-155, arc_length_map.py:97-160) on the two tables"""
    n_seg = (len(poly) - 3) // 12
    G = len(arcs) - 1
    if arc > full or not full > 0.0:
        return np.array([float(poly[n_seg * 12 + d]) for d in range(3)])
    rel = arc / full
    if rel <= arcs[0]:
        u = 0.0
    elif rel >= arcs[G]:
        u = 1.0
    else:
        lo, hi = 0, G
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if arcs[mid] <= rel:
                lo = mid
            else:
                hi = mid
        l0, l1 = float(arcs[lo]), float(arcs[lo + 1])
        u0, u1 = lo / float(G), (lo + 1) / float(G)
        u = u0 if l0 == rel else u0 + (rel - l0) / (l1 - l0) * (u1 - u0)
    return polynomial_point(poly, u)
