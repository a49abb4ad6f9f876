"""What a path-following planner asks of its trajectory between the scoring launches, for a batch of walks, on the device:

  advance_along_trajectory   GraphWalkPlanner._update_path (graph_walk_planner.py:266-277): how far along the path each walk has come
  goals_along_trajectory     _generate_node_evaluation_constraints (:155-182) with _add_constraint[_with_orientation] (:136-153): where
                             the next step of each walk is to end, and heading which way

`trajectory` is a _capi.Trajectory of any of the three spline types.  The launches of a call follow each other on the context's
stream; nothing is downloaded between them, the results come back in one copy at the end.  Nothing here has been timed.
"""
import numpy as np

from . import _capi
from .spline_types import parameter_by_arc_length_host


def _host_tables(trajectory):
    """(poly, relative arc lengths, full arc length) of the trajectory, read back once and kept on it"""
    tables = getattr(trajectory, "_host_tables", None)
    if tables is None:
        tables = trajectory._host_tables = trajectory.tables()
    return tables


def _parameter_at(arcs, full, arc):
    u = parameter_by_arc_length_host(arcs, full, arc)
    return 1.0 if u is None else u


def advance_along_trajectory(trajectory, positions, travelled, look_ahead, n=None):
    """The rule of _update_path for n walks: positions (n, 3) -- a NumPy array, or a device buffer / address of n rows of 3 float64 with
    n given --, travelled: the arc length each walk has behind it (a number or (n,)), look_ahead: how far ahead of it the closest point
    is looked for.  Returns the new travelled arc lengths (n,).

    Three launches.  mg_trajectory_closest_points finds each position's closest point at or after the parameter of the SMALLEST
    travelled length (the search takes one lower bound per call: walks of one planner step share theirs; a walk further along is
    held to its own by the last launch).  mg_trajectory_points_at_parameters turns the parameters into points, none further than
    the parameter of travelled + look_ahead -- the search has no upper bound of its own: where the distance has one basin inside
    the window this is the bounded search's result.  mg_trajectory_arc_length_of_points takes the arc length of each point among the
    samples beyond the walk's travelled length; where none is (-1: the walk has reached the end) the result is the full arc length."""
    prim, ctx = trajectory.prim, trajectory.prim.ctx
    host_positions = isinstance(positions, np.ndarray) or n is None
    if host_positions:
        positions = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        n = len(positions)
    n = int(n)
    if n == 0:
        return np.empty(0)
    _, arcs, full = _host_tables(trajectory)
    travelled = np.ascontiguousarray(np.broadcast_to(np.asarray(travelled, dtype=np.float64), (n,)))
    u_lo = _parameter_at(arcs, full, float(travelled.min()))
    u_hi = np.array([_parameter_at(arcs, full, float(t) + float(look_ahead)) for t in travelled])
    with ctx.buffers() as bufs:
        d_pos = bufs.upload(positions) if host_positions else positions
        d_trav, d_hi = bufs.upload(travelled), bufs.upload(u_hi)
        d_u, d_pt, d_arc = bufs.malloc(n * 8), bufs.malloc(n * 24), bufs.malloc(n * 8)
        _capi._check(prim.lib.mg_trajectory_closest_points(prim.handle, trajectory.handle, _capi._dev_ptr(d_pos), n, 1, float(u_lo), d_u.ptr, None, None))
        trajectory.points_at_parameters_dev(d_u, n, d_pt, d_hi)
        trajectory.arc_length_of_points_dev(d_pt, n, d_arc, d_trav)
        arc = ctx.download(d_arc, (n,), np.float64)
    arc[arc == -1.0] = full
    return arc


def goals_along_trajectory(trajectory, travelled, look_ahead, with_orientation=False, half_step=False):
    """The goals _generate_node_evaluation_constraints sets for the next step of n walks (travelled: a number or (n,)): a dict with
    'positions' (n, 3), the path's points at travelled + look_ahead; with_orientation: 'tangents' (n, 3), the path's unit tangents
    there (get_tangent_at_arc_length); half_step: 'half_positions' (n, 3), the points at travelled + look_ahead / 2.  One launch."""
    travelled = np.atleast_1d(np.asarray(travelled, dtype=np.float64))
    n = len(travelled)
    arcs = travelled + float(look_ahead)
    if half_step:
        arcs = np.concatenate([arcs, travelled + float(look_ahead) / 2])
    got = trajectory.points_by_arc_length(arcs, tangents=with_orientation)
    points, tangents = got if with_orientation else (got, None)
    out = {"positions": points[:n]}
    if with_orientation:
        out["tangents"] = tangents[:n]
    if half_step:
        out["half_positions"] = points[n:]
    return out
