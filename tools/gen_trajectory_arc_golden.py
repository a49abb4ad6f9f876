#!/usr/bin/env python3
"""Generate tests/golden/trajectory_arc_queries.npz by running the REFERENCE's own, unmodified ParameterizedSpline
(constraints/spatial_constraints/splines/parameterized_spline.py) for all three spline types, imported through a stub parent package
the way tools/gen_spline_type_golden.py imports it.  The fixture holds inputs and recorded outputs, no program text.

    python tools/gen_trajectory_arc_golden.py <reference checkout>

Per spline type (0, 1, 2) and n_points in (4, 12), granularity 1000, on seeded control points:
  arcs / points_by_arc / tangents / angles   query_point_by_absolute_arc_length, get_tangent_at_arc_length (eval_range 0.5) and
                                             get_angle_at_arc_length_2d against reference_dir, at 0, 0.2, full / 2, full - 0.2, full,
                                             full + 2.55 (the tangent's range is widened to 2.6 there: a chord of 0.05) and 24 seeded lengths
  q_points / q_min_arc / q_arc / q_min_point get_absolute_arc_length_of_point for seeded points off the path by a visible margin (a few
                                             per cent of its length) and for points exactly ON samples of a curved stretch (their
                                             neighbours are not symmetric), with min_arc_length 0, mid-path and -- one query -- the
                                             full length (the result is -1, the point NaN here)
  q_min_u / q_min_index                      the parameter the reference's loop settled on and its place in the loop
  q_ambiguous                                the reference's two smallest distances differ by less than 1e-12 relative: np.linalg.norm's
                                             last bit may decide the index, the query is left out of index comparisons
  uk_granularity / uk_count / uk_last        for granularities 7, 64, 65, 1000, 1024: how many parameters the reference's loop
                                             (u += 1.0 / granularity while u <= 1.0) visits, and the last one

Nothing of the reference is changed: the loop's parameters and points are OBSERVED by shadowing query_point_by_parameter on the
spline INSTANCE with a recorder that calls the class's method and keeps (u, result); the result object the reference returns as the
closest point is found among them by identity.

After writing, the generator checks on the CPU what the tests rely on: at most 2 % of the point queries are ambiguous, and the
repository's own statement (morphablegraphs_amd.spline_types.arc_length_of_point_host) picks the reference's index on all others."""
import contextlib
import io
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
TYPES = (0, 1, 2)
N_POINTS = (4, 12)
UK_GRANULARITIES = (7, 64, 65, 1000, 1024)
REFERENCE_DIR = (0.1, 1.0)      # the paths head along +x within about 65 degrees: every angle stays well away from 0 and 180
N_OFF, N_ON = 20, 4


def control_points(rng, n_points):
    return np.cumsum(np.column_stack([rng.uniform(20, 60, n_points), rng.uniform(-4, 4, n_points), rng.uniform(-40, 40, n_points)]), axis=0)


def make_spline(ps, cps, spline_type, granularity=1000):
    with contextlib.redirect_stdout(io.StringIO()):      # (BSpline prints its knot vector)
        return ps.ParameterizedSpline(cps.tolist(), spline_type, granularity=granularity)


class observed(object):
    """with observed(sp) as seen: every query_point_by_parameter of the spline inside the block lands in seen as (u, result)"""

    def __init__(self, sp):
        self.spline, self.seen = sp.spline, []

    def __enter__(self):
        method = type(self.spline).query_point_by_parameter

        def recorder(u):
            result = method(self.spline, u)
            self.seen.append((u, result))
            return result
        self.spline.query_point_by_parameter = recorder
        return self.seen

    def __exit__(self, *exc):
        del self.spline.query_point_by_parameter


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    from gen_spline_type_golden import import_reference_splines
    from morphablegraphs_amd.spline_types import arc_length_of_point_host, arc_length_table_host, sample_parameters_host, trajectory_polynomials_host
    ps = import_reference_splines(sys.argv[1])
    out = {"spline_types": np.array(TYPES, dtype=np.int64), "n_points": np.array(N_POINTS, dtype=np.int64),
           "reference_dir": np.array(REFERENCE_DIR), "uk_granularity": np.array(UK_GRANULARITIES, dtype=np.int64)}
    counts, lasts = [], []
    cps4 = control_points(np.random.default_rng(77), 4)
    for g in UK_GRANULARITIES:
        sp = make_spline(ps, cps4, 0, g)
        with observed(sp) as seen:
            sp.get_absolute_arc_length_of_point(np.zeros(3), min_arc_length=-1.0)      # (every parameter's arc length is > -1)
        counts.append(len(seen)), lasts.append(float(seen[-1][0]))
    out["uk_count"], out["uk_last"] = np.array(counts, dtype=np.int64), np.array(lasts)
    total = ambiguous = 0
    for st in TYPES:
        for n_points in N_POINTS:
            key = "%d_%d" % (st, n_points)
            rng = np.random.default_rng(9300 + 10 * st + n_points)
            cps = control_points(rng, n_points)
            sp = make_spline(ps, cps, st)
            full = float(sp.full_arc_length)
            out["control_points_" + key], out["full_arc_length_" + key] = cps, np.float64(full)
            arcs = np.concatenate([[0.0, 0.2, 0.5 * full, full - 0.2, full, full + 2.55], rng.uniform(0, full, 24)])
            pts, tans, angs = [], [], []
            for a in arcs:
                start, tangent, angle = sp.get_angle_at_arc_length_2d(float(a), np.array(REFERENCE_DIR))
                pts.append(np.asarray(sp.query_point_by_absolute_arc_length(float(a)), dtype=np.float64).reshape(3))
                assert np.array_equal(pts[-1], np.asarray(start, dtype=np.float64).reshape(3))
                tans.append(np.asarray(tangent, dtype=np.float64).reshape(3)), angs.append(float(angle))
            out["arcs_" + key], out["points_by_arc_" + key], out["tangents_" + key], out["angles_" + key] = arcs, np.array(pts), np.array(tans), np.array(angs)
            # the point queries
            on = np.stack([np.asarray(sp.query_point_by_parameter(float(u)), dtype=np.float64).reshape(3) for u in rng.uniform(0.02, 0.98, N_OFF)])
            off = on + rng.normal(0.0, 0.03 * full, (N_OFF, 3)) * np.array([1.0, 0.3, 1.0])
            us = sample_parameters_host(1000)
            exact = np.stack([np.asarray(sp.query_point_by_parameter(float(us[k])), dtype=np.float64).reshape(3) for k in rng.choice(np.arange(50, 950), N_ON, replace=False)])
            queries = [(p, m) for p in np.concatenate([off, exact]) for m in (0.0, 0.45 * full)] + [(off[0], full)]
            q_arc, q_u, q_k, q_pt, q_amb = [], [], [], [], []
            poly = trajectory_polynomials_host(cps, st)
            table, table_full = arc_length_table_host(poly, 1000)
            for p, m in queries:
                with observed(sp) as seen:
                    arc, min_point = sp.get_absolute_arc_length_of_point(p, min_arc_length=m)
                total += 1
                if min_point is None:
                    assert arc == -1 and not seen
                    q_arc.append(-1.0), q_u.append(np.nan), q_k.append(-1), q_pt.append(np.full(3, np.nan)), q_amb.append(False)
                    assert arc_length_of_point_host(poly, table, table_full, p, m, us)[2] == -1
                    continue
                dist = np.sort([float(np.linalg.norm(r - p)) for _, r in seen])
                amb = len(dist) > 1 and (dist[1] - dist[0]) < 1.0e-12 * max(dist[1], 1.0e-300)
                (u_min,) = [u for u, r in seen if r is min_point]
                k_min = int(np.flatnonzero(us == u_min)[0])
                ambiguous += amb
                q_arc.append(float(arc)), q_u.append(float(u_min)), q_k.append(k_min), q_amb.append(bool(amb))
                q_pt.append(np.asarray(min_point, dtype=np.float64).reshape(3))
                if not amb:
                    mine = arc_length_of_point_host(poly, table, table_full, p, m, us)
                    assert mine[2] == k_min, (key, p, m, mine[2], k_min)
            out["q_points_" + key], out["q_min_arc_" + key] = np.array([p for p, _ in queries]), np.array([m for _, m in queries])
            out["q_arc_" + key], out["q_min_u_" + key], out["q_min_index_" + key] = np.array(q_arc), np.array(q_u), np.array(q_k, dtype=np.int64)
            out["q_min_point_" + key], out["q_ambiguous_" + key] = np.array(q_pt), np.array(q_amb)
    path = os.path.join(os.environ.get("MG_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden"), "trajectory_arc_queries.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    print("parameters per granularity:", dict(zip(UK_GRANULARITIES, counts)))
    print("ambiguous point queries: %d of %d" % (ambiguous, total))
    assert ambiguous <= 0.02 * total, "choose other seeds: too many queries whose two smallest distances coincide"


if __name__ == "__main__":
    main()
