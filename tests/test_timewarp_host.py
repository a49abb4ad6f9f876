"""The time warp without a device: the plain statement of back_project_time_function's inversion (scipy's splrep / splev, the
reference's own arithmetic) against a 50-digit twin over the whole case table of tests/timewarp_cases.py, the conditions that make
the sample counts of the table safe to compare exactly, the host route's sample count of 0, and the speed semantics of steps
without a time model in assemble_walk_host and HipGraphWalk(host=True).  tests/test_gpu_timewarp_shapes.py runs the kernels
against the same table and bounds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import timewarp_cases as tc
from morphablegraphs_amd import graph_walk as gw
from morphablegraphs_amd.motion_primitive import HipMotionPrimitive
from test_graph_walk_host import SEQUENCE, SHAPES, StubGraph, primitive_jsons, stub_walk


def test_the_table_holds_every_case_the_kernels_branch_on():
    cases = [c[2] for c in tc.CASES]
    assert {c[0] for c in cases} >= {4, 5, 6, 63, 64, 65, 129, 2048} and {c[1] for c in cases} >= {1, 2, 5}
    assert {c[5] for c in cases} >= {1.0, 1.6, 0.37}
    for F in tc.FRAMES:
        assert {(c[1], c[5]) for c in cases if c[0] == F} >= {(lt, s) for lt in tc.TIME_COMPONENTS for s in tc.SPEEDS}
    assert tc.case_figures("count0")[3] == [0] * tc.ROWS and tc.case_figures("count1")[3] == [1] * tc.ROWS
    data, gamma = tc.model_of("first_sample_below_x0")
    for g in gamma:
        c = tc.canonical_time_function(data, g)
        assert c[0] + 1.0 > 2.0 and c[0] > 1.0          # the first increment exceeds 2: the first sample t = 1 lies below x[0]
    assert min(tc.case_figures("long_row")[3]) + 2 > 4 * 64 + 8


@pytest.mark.parametrize("case_id", tc.CASE_IDS)
def test_fitpack_against_the_twin_and_the_count_is_safe(case_id):
    """e_fit: FITPACK's deviation from the 50-digit not-a-knot cubic at the same sample points, which the GPU tests' tolerance is
    made of -- FITPACK must itself be within the tolerance it defines and within the suite's 1e-11 F; and the margins that make a
    last-bit difference of the device's exp() unable to move the sample count."""
    F = tc.CASES[tc.CASE_IDS.index(case_id)][2][0]
    e_fit, half, whole, counts = tc.case_figures(case_id)
    print("%s: e_fit %.3g (%.3g F), tolerance %.3g, t(F-2) is %.3g from a half-integer, the count's product %.3g from an integer, counts %s"
          % (case_id, e_fit, e_fit / F, tc.time_tolerance(case_id), half, whole, counts))
    assert e_fit <= 1.0e-11 * F and e_fit <= tc.time_tolerance(case_id)
    assert half >= tc.MARGIN and whole >= tc.MARGIN


@pytest.mark.parametrize("F", [4, 5, 6, 63, 64, 65])
def test_the_twins_band_solve_is_its_dense_solve(F):
    """The twin solves F <= 6 densely and longer systems inside their band (a dense 50-digit solve of 2048 unknowns is out of reach):
    the two agree to 40 digits where both can run, and the band solution leaves no residual."""
    data, gamma = tc.model_of((F, 2))
    c = tc.canonical_time_function(data, gamma[0])
    _, dense = tc.second_derivatives_mp(c, True)
    _, band = tc.second_derivatives_mp(c, False)
    assert max(abs(a - b) for a, b in zip(dense, band)) <= 1e-40 * max(abs(a) for a in dense)
    assert tc.residual_mp(c, band) <= 1e-40


def test_the_band_solve_leaves_no_residual_at_the_largest_size():
    data, gamma = tc.model_of((2048, 2))
    c = tc.canonical_time_function(data, gamma[1])
    _, band = tc.second_derivatives_mp(c, False)
    assert np.all(np.diff(c) > 0) and tc.residual_mp(c, band) <= 1e-40


def test_the_twin_interpolates_its_data():
    data, gamma = tc.model_of((6, 2))
    c = tc.canonical_time_function(data, gamma[0])
    got = tc.twin_time_function(c, 1.0)
    ref = tc.reference_time_function(c, 1.0)
    assert got[0] == 0.0 and got[-1] == 5.0 and len(got) == len(ref)
    # (1, t(F-2)) are the ends of the sample points; t(F-2) is a data point: its ordinate is F - 2
    assert abs(got[-2] - 4.0) <= 1e-14 and abs(ref[-2] - 4.0) <= 1e-13


# ---- finding 3: a sample count of 0 on the host route ---------------------------------------------------------------------
def _host_primitive(F):
    mp = HipMotionPrimitive(None)            # no file: no device primitive is made; the inversion reads n_canonical_frames alone
    mp.n_canonical_frames = F
    return mp


def test_a_count_of_zero_gives_the_two_pinned_ends_on_the_host_route():
    data, gamma = tc.model_of("count0")
    speed = tc.CONSTANT["count0"][5]
    for g in gamma:
        c = tc.canonical_time_function(data, g)
        got = _host_primitive(4)._invert_canonical_to_sample_time_function(c, speed)
        assert np.array_equal(got, [0.0, 3.0]) and np.array_equal(got, tc.reference_time_function(c, speed))


@pytest.mark.parametrize("case_id", ["count1", "F5-Lt2-speed0.37", "F64-Lt1-speed1.6", "first_sample_below_x0"])
def test_the_host_route_is_the_plain_statement(case_id):
    _, key, (F, _, _, _, _, speed) = tc.CASES[tc.CASE_IDS.index(case_id)]
    data, gamma = tc.model_of(key)
    for g in gamma:
        c = tc.canonical_time_function(data, g)
        assert np.array_equal(_host_primitive(F)._invert_canonical_to_sample_time_function(c, speed), tc.reference_time_function(c, speed))


# ---- finding 1: a step without a time model at a speed other than 1 ------------------------------------------------------------
@pytest.mark.parametrize("speed", [1.6, 0.5, 1.0])
def test_untimed_steps_take_the_grid_of_their_speed(speed):
    """back_project(s, True, speed) of a node without a time model: linspace(0, F, int(F * (1 / speed))) (motion_primitive.py:233)."""
    steps = [primitive_jsons()[k] for k in (0, 1)]
    S = 0.7 * np.random.default_rng(5).standard_normal((1, 5 + 8))
    explicit = [[np.linspace(0, d["n_canonical_frames"], int(d["n_canonical_frames"] * (1.0 / speed))) for d in steps]]
    want, want_off, _ = gw.assemble_walk_host(steps, S, times=explicit)
    got, off, _ = gw.assemble_walk_host(steps, S, speed=speed)
    assert np.array_equal(off, want_off) and np.array_equal(got, want)
    assert off[0].tolist() == [0, int(12 * (1.0 / speed)), int(12 * (1.0 / speed)) + int(33 * (1.0 / speed))]
    mixed, off2, _ = gw.assemble_walk_host(steps, S, times=[[None, explicit[0][1]]], speed=speed)
    assert np.array_equal(off2, want_off) and np.array_equal(mixed, want)
    if speed == 1.0:
        plain, _, _ = gw.assemble_walk_host(steps, S)
        assert np.array_equal(plain, want)
    with pytest.raises(ValueError, match="no sample"):
        gw.assemble_walk_host(steps, S, speed=40.0)


class _MixedGraph(StubGraph):
    """w1 carries a (stub) time model, w0 and w2 none."""

    def __init__(self):
        StubGraph.__init__(self, 0)
        node = self.nodes[("walk", "w1")]
        node.n_time, node.has_time_parameters = 1, True


@pytest.mark.parametrize("speed", [1.6, 0.5])
def test_a_host_walk_mixes_timed_and_untimed_steps_at_a_speed(speed):
    graph = _MixedGraph()
    walk = gw.HipGraphWalk(graph, host=True)
    rng = np.random.default_rng(9)
    for k in SEQUENCE:
        node = graph.nodes[("walk", "w%d" % k)]
        par = np.concatenate((0.7 * rng.standard_normal(SHAPES[k][0]), rng.integers(-3, 4, node.n_time).astype(np.float64)))
        walk.steps.append(gw.HipGraphWalkStep.from_graph(graph, ("walk", "w%d" % k), par))
    walk.convert_graph_walk_to_quaternion_frames(use_time_parameters=True, step_size=speed)
    lengths = [SHAPES[k][1] + int(s.parameters[-1]) if k == 1 else int(SHAPES[k][1] * (1.0 / speed)) for k, s in zip(SEQUENCE, walk.steps)]
    starts = np.concatenate(([0], np.cumsum(lengths)[:-1]))
    assert [s.start_frame for s in walk.steps] == starts.tolist()
    assert [s.end_frame for s in walk.steps] == (starts + np.array(lengths) - 1).tolist()
    assert walk.get_num_of_frames() == sum(lengths) and not np.isnan(walk.get_quat_frames()).any()
    # the same walk step by step: every step's own time function, explicit
    nodes = [graph.nodes[s.node_key] for s in walk.steps]
    times = [[node.back_project_time_function(s.parameters[s.n_spatial_components:], speed) if node.n_time else
              np.linspace(0, node.n_canonical_frames, int(node.n_canonical_frames * (1.0 / speed))) for node, s in zip(nodes, walk.steps)]]
    ref, _, _ = gw.assemble_walk_host(nodes, np.array(walk.get_global_spatial_parameter_vector())[None, :], times=times)
    assert np.array_equal(walk.get_quat_frames(), ref[0])


def test_an_unwarped_walk_at_another_step_size_is_still_refused():
    _, walk = stub_walk()
    with pytest.raises(NotImplementedError):
        walk.convert_graph_walk_to_quaternion_frames(step_size=1.6)


# ---- finding 2: rows beyond the bound assumed before the lengths are known, on the host store -------------------------------------
def test_a_host_walk_grows_its_rows_with_the_lengths():
    graph = StubGraph(1)
    walk = gw.HipGraphWalk(graph, host=True)
    rng = np.random.default_rng(2)
    for k, extra in ((0, 400.0), (1, 0.0)):  # 412 samples: more than the (4 * 12 + 8) + (4 * 33 + 8) = 196 rows assumed for the whole walk
        walk.steps.append(gw.HipGraphWalkStep.from_graph(graph, ("walk", "w%d" % k), np.concatenate((0.7 * rng.standard_normal(SHAPES[k][0]), [extra]))))
    walk.convert_graph_walk_to_quaternion_frames(use_time_parameters=True)
    assert walk.get_num_of_frames() == 412 + 33 and not np.isnan(walk.get_quat_frames()).any()
    assert (walk.steps[1].start_frame, walk.steps[1].end_frame) == (412, 444)
