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
import struct

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


def parameter_by_arc_length_host(arcs, full, arc):
    """The parameter mg_traj_point_by_arc (csrc/mg_traj_device.h) evaluates the curve at: the table entries bounding the relative
    arc length, their parameters interpolated linearly (arc_length_map.py:97-160); None beyond the full arc length, where the
    query returns the last control point."""
    G = len(arcs) - 1
    arc, full = float(arc), float(full)
    if arc > full or not full > 0.0:
        return None
    rel = arc / full
    if rel <= arcs[0]:
        return 0.0
    if rel >= arcs[G]:
        return 1.0
    lo, hi = 0, G
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if arcs[mid] <= rel:
            lo = mid
        else:
            hi = mid
    l0, l1 = float(arcs[lo]), float(arcs[lo + 1])
    u0, u1 = lo / float(G), (lo + 1) / float(G)
    return u0 if l0 == rel else u0 + (rel - l0) / (l1 - l0) * (u1 - u0)


def point_by_arc_length_host(poly, arcs, full, arc):
    """mg_traj_point_by_arc (csrc/mg_traj_device.h): ParameterizedSpline.query_point_by_absolute_arc_length
    (parameterized_spline.py:131-155, arc_length_map.py:97-160) on the two tables"""
    n_seg = (len(poly) - 3) // 12
    u = parameter_by_arc_length_host(arcs, full, arc)
    if u is None:
        return np.array([float(poly[n_seg * 12 + d]) for d in range(3)])
    return polynomial_point(poly, u)


# ---- the arc-length queries (csrc/mg_trajectory_arc.hip), statement for statement ------------------------------------------------------
MAX_WIDENINGS = 1024        # MG_ARC_MAX_WIDENINGS


class TangentWideningExhausted(ValueError):
    """The two points of a tangent still coincide after MAX_WIDENINGS widenings (the library: MG_ERR_UNSUPPORTED)."""


def sample_parameters_host(granularity):
    """The parameters get_absolute_arc_length_of_point scans (parameterized_spline.py:251-268): u = 0, u += 1.0 / granularity while
    u <= 1.0 -- repeated addition, so the sums drift and there are granularity or granularity + 1 of them.  What
    mg_trajectory_sample_parameters returns."""
    step_size = 1.0 / int(granularity)
    us, u = [], 0.0
    while u <= 1.0:
        us.append(u)
        u += step_size
    return np.array(us, dtype=np.float64)


def absolute_arc_length_host(arcs, full, t):
    """mg_arc_absolute: RelativeArcLengthMap.get_absolute_arc_length (arc_length_map.py:73-90) on the table of relative arc lengths"""
    G = len(arcs) - 1
    t, full = float(t), float(full)
    step_size = 1.0 / G
    table_index = min(max(int(t / step_size), 0), G)
    if table_index < G:
        t_i, t_i_1 = table_index / float(G), (table_index + 1) / float(G)
        a_i, a_i_1 = float(arcs[table_index]), float(arcs[table_index + 1])
        arc_length = a_i + ((t - t_i) / (t_i_1 - t_i)) * (a_i_1 - a_i)
        return arc_length * full
    return float(arcs[table_index]) * full


def _norm3(x, y, z):
    return math.sqrt(x * x + y * y + z * z)


def arc_length_of_point_host(poly, arcs, full, point, min_arc_length=0.0, us=None):
    """mg_trajectory_arc_length_of_points for one point: ParameterizedSpline.get_absolute_arc_length_of_point
    (parameterized_spline.py:242-273) -> (arc length, the curve's point there, the parameter's index), or (-1.0, None, -1) where no
    parameter's arc length is > min_arc_length.  The distance is sqrt(dx dx + dy dy + dz dz) in that order; the first strict minimum
    wins.  us: sample_parameters_host(granularity), to share between calls."""
    if us is None:
        us = sample_parameters_host(len(arcs) - 1)
    q = [float(v) for v in point]
    min_arc_length = float(min_arc_length)
    min_distance, min_k, min_point = math.inf, -1, None
    for k, u in enumerate(us):
        if absolute_arc_length_host(arcs, full, u) > min_arc_length:
            p = polynomial_point(poly, u)
            distance = _norm3(float(p[0]) - q[0], float(p[1]) - q[1], float(p[2]) - q[2])
            if distance < min_distance:
                min_distance, min_k, min_point = distance, k, p
    if min_k < 0:
        return -1.0, None, -1
    return absolute_arc_length_host(arcs, full, us[min_k]), min_point, min_k


def tangent_at_arc_length_host(poly, arcs, full, arc, eval_range=0.5):
    """mg_trajectory_points_by_arc_length's tangent: ParameterizedSpline.get_tangent_at_arc_length (parameterized_spline.py:186-207)
    -> (start point, unit direction); the chord over [arc - r, arc + r], r += 0.1 while its ends coincide, at most MAX_WIDENINGS
    times (then TangentWideningExhausted)."""
    arc, eval_range = float(arc), float(eval_range)
    start = point_by_arc_length_host(poly, arcs, full, arc)
    for _ in range(MAX_WIDENINGS + 1):
        p1 = point_by_arc_length_host(poly, arcs, full, arc - eval_range)
        p2 = point_by_arc_length_host(poly, arcs, full, arc + eval_range)
        d = [float(p2[0]) - float(p1[0]), float(p2[1]) - float(p1[1]), float(p2[2]) - float(p1[2])]
        magnitude = _norm3(d[0], d[1], d[2])
        eval_range += 0.1
        if magnitude != 0.0:
            return start, np.array([d[0] / magnitude, d[1] / magnitude, d[2] / magnitude])
    raise TangentWideningExhausted("the tangent's two points coincide at arc length %r" % (arc,))


def _clear_low_word(x):
    return struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", x))[0] & 0xffffffff00000000))[0]


def acos_host(x):
    """mg_arc_acos: acos as fdlibm states it (e_acos.c), in plain IEEE operations and sqrt; NaN for |x| > 1"""
    pio2_hi, pio2_lo, pi = 1.57079632679489655800e+00, 6.12323399573676603587e-17, 3.14159265358979311600e+00
    pS = (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01, -4.00555345006794114027e-02,
          7.91534994289814532176e-04, 3.47933107596021167570e-05)
    qS = (-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02)
    x = float(x)
    ax = abs(x)
    if not ax < 1.0:
        if x == 1.0:
            return 0.0
        if x == -1.0:
            return pi + 2.0 * pio2_lo
        return math.nan
    z = x * x if ax < 0.5 else ((1.0 + x) * 0.5 if x < 0.0 else (1.0 - x) * 0.5)
    p = z * (pS[0] + z * (pS[1] + z * (pS[2] + z * (pS[3] + z * (pS[4] + z * pS[5])))))
    q = 1.0 + z * (qS[0] + z * (qS[1] + z * (qS[2] + z * qS[3])))
    r = p / q
    if ax < 0.5:
        return pio2_hi - (x - (pio2_lo - r * x))
    s = math.sqrt(z)
    if x < 0.0:
        w = r * s - pio2_lo
        return pi - 2.0 * (s + w)
    df = _clear_low_word(s)
    c = (z - df * df) / (s + df)
    w = r * s + c
    return 2.0 * (df + w)


def angle_at_arc_length_2d_host(poly, arcs, full, arc, reference_vector, eval_range=0.5):
    """mg_trajectory_points_by_arc_length's angle: ParameterizedSpline.get_angle_at_arc_length_2d (parameterized_spline.py:217-240)
    -> (start point, unit tangent, degrees between (tangent x, tangent z) and the 2-D reference vector)"""
    start, tangent = tangent_at_arc_length_host(poly, arcs, full, arc, eval_range)
    r0, r1 = float(reference_vector[0]), float(reference_vector[1])
    na = math.sqrt(r0 * r0 + r1 * r1)
    a0, a1 = r0 / na, r1 / na
    t0, t2 = float(tangent[0]), float(tangent[2])
    nb = math.sqrt(t0 * t0 + t2 * t2)
    if na == 0.0 or nb == 0.0:           # (a zero reference or a vertical tangent: the device's 0 / 0)
        return start, tangent, math.nan
    b0, b1 = t0 / nb, t2 / nb
    return start, tangent, acos_host(a0 * b0 + a1 * b1) * (180.0 / math.pi)
