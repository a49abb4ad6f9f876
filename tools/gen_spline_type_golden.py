#!/usr/bin/env python3
"""Generate tests/golden/trajectory_spline_types.npz by running the REFERENCE's own, unmodified ParameterizedSpline with
SPLINE_TYPE_BSPLINE (1) and SPLINE_TYPE_FITTED_BSPLINE (2): constraints/spatial_constraints/splines/{parameterized_spline,b_spline,
fitted_b_spline,arc_length_map}.py, imported through a stub parent package the way oracle/gen_golden.py imports them (they need
numpy, scipy and matplotlib only).  The fixture holds inputs and recorded outputs, no program text.

    python tools/gen_spline_type_golden.py <reference checkout>

Per type and n_points in (4, 5, 9), on seeded control points (x and z drawn as oracle/gen_golden.py run_trajectory_spline_case draws
them, y a few units so that the vertical axis is not identically zero):
  parameters / points            query_point_by_parameter at 0, 1, 0.5, 1/3, every interior break, one ulp either side of each break
                                 and 40 seeded parameters (type 1's breaks are its distinct knots, type 2's its data sites)
  full_arc_length                the granularity-1000 table's
  arc_lengths / points_by_arc    query_point_by_absolute_arc_length at 0, full, full / 2, 1.25 full and 40 seeded lengths
  cp_targets / cp_min_u / cp_u / cp_point / cp_distance
                                 find_closest_point_fast (scipy L-BFGS-B from the bound) for 24 seeded targets x min_u in (0, 0.3)

THE ONE SHIM, the same as the Catmull-Rom closest-point fixture's (oracle/gen_golden.py scalar_spline_parameter): scipy hands the
objective its parameter as a 1-element ndarray; the wrapper unwraps it to the float it holds before the reference's own
query_point_by_parameter runs.  BSpline accepts the array as it is (the result is the same); FittedBSpline does not: splev of a
(1,) array gives (1,) arrays, the point becomes (3, 1), and `eval_point - target` broadcasts to a 3 x 3 matrix whose Frobenius norm is
not the distance to the curve.  With the float the objective is the distance the method's name and docstring state.

After writing, the generator checks on the CPU what the GPU test relies on: the repository's own statement of the search
(oracle/mg_oracle.py lbfgsb_1d on morphablegraphs_amd.spline_types.trajectory_polynomials_host) lands in the reference's basin -- within
one cell of the granularity-1000 grid in u -- for at least 95 % of the closest-point cases of every curve."""
import contextlib
import importlib
import io
import math
import os
import sys
import types
import warnings

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_POINTS = (4, 5, 9)
TYPES = (1, 2)
MIN_US = (0.0, 0.3)
N_TARGETS = 24


def import_reference_splines(reference):
    warnings.filterwarnings("ignore")
    if "mg_ref_splines" not in sys.modules:
        pkg = types.ModuleType("mg_ref_splines")
        pkg.__path__ = [os.path.join(reference, "morphablegraphs", "constraints", "spatial_constraints", "splines")]
        sys.modules["mg_ref_splines"] = pkg
    return importlib.import_module("mg_ref_splines.parameterized_spline")


class scalar_spline_parameter(object):
    """see the module docstring"""

    def __enter__(self):
        self.classes = [importlib.import_module("mg_ref_splines.b_spline").BSpline,
                        importlib.import_module("mg_ref_splines.fitted_b_spline").FittedBSpline]
        self.orig = [c.query_point_by_parameter for c in self.classes]
        for c, orig in zip(self.classes, self.orig):
            def unwrapped(spline, u, orig=orig):
                if isinstance(u, np.ndarray) and u.size == 1:
                    u = float(u.reshape(-1)[0])
                return orig(spline, u)
            c.query_point_by_parameter = unwrapped
        return self

    def __exit__(self, *exc):
        for c, orig in zip(self.classes, self.orig):
            c.query_point_by_parameter = orig


def control_points(rng, n_points):
    return np.cumsum(np.column_stack([rng.uniform(20, 60, n_points), rng.uniform(-4, 4, n_points), rng.uniform(-40, 40, n_points)]), axis=0)


def breaks_of(spline_type, n_points):
    return np.linspace(0.0, 1.0, n_points - 2 if spline_type == 1 else n_points)[1:-1]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    reference = sys.argv[1]
    ps = import_reference_splines(reference)
    from morphablegraphs_amd.spline_types import polynomial_point, trajectory_polynomials_host
    from oracle import mg_oracle as orc
    out = {"spline_types": np.array(TYPES, dtype=np.int64), "n_points": np.array(N_POINTS, dtype=np.int64)}
    share = {}
    for st in TYPES:
        for n_points in N_POINTS:
            key = "%d_%d" % (st, n_points)
            rng = np.random.default_rng(9100 + 10 * st + n_points)
            cps = control_points(rng, n_points)
            with contextlib.redirect_stdout(io.StringIO()):      # (BSpline prints its knot vector)
                sp = ps.ParameterizedSpline(cps.tolist(), st)
            br = breaks_of(st, n_points)
            us = np.concatenate([[0.0, 1.0, 0.5, 1.0 / 3.0], br, np.nextafter(br, 0.0), np.nextafter(br, 1.0), rng.uniform(0, 1, 40)])
            out["control_points_" + key] = cps
            out["parameters_" + key] = us
            out["points_" + key] = np.stack([np.asarray(sp.query_point_by_parameter(float(u)), dtype=np.float64).reshape(3) for u in us])
            full = float(sp.full_arc_length)
            out["full_arc_length_" + key] = np.float64(full)
            arcs = np.concatenate([[0.0, full, 0.5 * full, 1.25 * full], rng.uniform(0, full, 40)])
            out["arc_lengths_" + key] = arcs
            out["points_by_arc_" + key] = np.stack([np.asarray(sp.query_point_by_absolute_arc_length(float(a)), dtype=np.float64).reshape(3) for a in arcs])
            # targets beside the curve: a point of it displaced by a few per cent of the path length
            on = np.stack([np.asarray(sp.query_point_by_parameter(float(u)), dtype=np.float64).reshape(3) for u in rng.uniform(0.02, 0.98, N_TARGETS)])
            targets = on + rng.normal(0.0, 0.03 * full, (N_TARGETS, 3)) * np.array([1.0, 0.3, 1.0])
            poly = trajectory_polynomials_host(cps, st)
            t_all, m_all, u_all, p_all, d_all, other = [], [], [], [], [], 0
            with scalar_spline_parameter():
                for min_u in MIN_US:
                    for tg in targets:
                        pt, u = sp.find_closest_point_fast(tg, min_u)
                        pt, u = np.asarray(pt, dtype=np.float64).reshape(3), float(np.ravel(u)[0])
                        t_all.append(tg), m_all.append(min_u), u_all.append(u), p_all.append(pt), d_all.append(float(np.linalg.norm(pt - tg)))

                        def dist(x, tg=tg):
                            v = polynomial_point(poly, x) - tg
                            return math.sqrt(float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
                        mine = orc.lbfgsb_1d(dist, min_u, min_u, 1.0, formk_rule=True)
                        other += abs(mine - u) > 1.0e-3
            share[key] = other / float(len(u_all))
            out["cp_targets_" + key], out["cp_min_u_" + key] = np.array(t_all), np.array(m_all)
            out["cp_u_" + key], out["cp_point_" + key], out["cp_distance_" + key] = np.array(u_all), np.array(p_all), np.array(d_all)
    path = os.path.join(os.environ.get("MG_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden"), "trajectory_spline_types.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    print("closest-point cases in another basin than the reference's (more than 1e-3 in u):", {k: "%.1f %%" % (100 * v) for k, v in share.items()})
    assert max(share.values()) <= 0.05, "choose other seeds: the statement alone leaves the reference's basin too often"


if __name__ == "__main__":
    main()
