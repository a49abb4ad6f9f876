"""Time-warped random walks without a device: the NumPy statements random_walks.walk_time_rows_host and
assemble_walks_mixed_host(times=...), and the ctypes prototypes of the four entry points behind RandomWalks.frames(
use_time_parameters=True).

The time rows are held to the reference's rule as tests/timewarp_cases.py states it (reference_time_function on the canonical time
function), within that module's own time_tolerance; the sample counts are compared exactly, on rows whose count margins that module
chose to be at least MARGIN.  No number is introduced here.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import random_walk_cases as rc
import timewarp_cases as tc
from morphablegraphs_amd import _capi, graph_walk as gw, random_walks as rw

SPEEDS = (1.0, 0.37, 1.6)
# three time models of timewarp_cases (the m == 4 solve, two and five time latents) and, between them, random_walk_cases' node a,
# which has none: one n_dim (11), 3 + Lt or 5 latent columns a step
TIMED = [(4, 1), (6, 2), (65, 5)]
WALKS = [[0, 3, 1], [2], [1, 1, 2, 0], [3, 2]]               # node 3: untimed


def _population():
    jsons = [tc.model_of(key)[0] for key in TIMED] + [rc.primitive_jsons()[0]]
    node_of, n_steps = rc.tables(WALKS)
    P = rc.latents(node_of, 9, seed=31)
    row_of = {}
    for w, seq in enumerate(WALKS):
        for i, k in enumerate(seq):
            if k < len(TIMED):
                Lt = TIMED[k][1]
                row_of[(w, i)] = (w + i) % tc.ROWS
                P[w, i, tc.N_SPATIAL:tc.N_SPATIAL + Lt] = tc.model_of(TIMED[k])[1][row_of[(w, i)]]     # the rows the cases' seeds were chosen for
    return jsons, node_of, n_steps, P, row_of


@pytest.mark.parametrize("speed", SPEEDS)
def test_time_rows_follow_the_references_rule(speed):
    jsons, node_of, n_steps, P, row_of = _population()
    times = rw.walk_time_rows_host(jsons, node_of, n_steps, P, speed)
    assert [len(t) for t in times] == [len(seq) for seq in WALKS]
    for w, seq in enumerate(WALKS):
        for i, k in enumerate(seq):
            if k == len(TIMED):
                F = rc.SHAPES[0][1]
                assert np.array_equal(times[w][i], np.linspace(0, F, int(F * (1.0 / speed))))
                continue
            F, Lt = TIMED[k]
            case = "F%d-Lt%d-speed%g" % (F, Lt, speed)
            canonical = tc.canonical_time_function(jsons[k], tc.model_of(TIMED[k])[1][row_of[(w, i)]])
            assert min(tc.count_margins(canonical, speed)) >= tc.MARGIN, (case, w, i)
            want = tc.reference_time_function(canonical, speed)
            worst = float(np.max(np.abs(times[w][i] - want))) if len(want) == len(times[w][i]) else np.inf
            print("%s walk %d step %d: %d samples, worst %.3g (bound %.3g)" % (case, w, i, len(want), worst, tc.time_tolerance(case)))
            assert len(times[w][i]) == len(want) and worst <= tc.time_tolerance(case), (case, w, i)


@pytest.mark.parametrize("speed", SPEEDS)
def test_untimed_rows_are_numpys_linspace(speed):
    jsons = rc.primitive_jsons()
    walks = [[0, 1], [1], [1, 0, 0]]
    node_of, n_steps = rc.tables(walks)
    times = rw.walk_time_rows_host(jsons, node_of, n_steps, rc.latents(node_of, 14), speed)
    for w, seq in enumerate(walks):
        for i, k in enumerate(seq):
            F = rc.SHAPES[k][1]
            assert int(F * (1.0 / speed)) == int(F / speed)
            assert np.array_equal(times[w][i], np.linspace(0, F, int(F / speed))), (w, i)
    with pytest.raises(ValueError):
        rw.walk_time_rows_host(jsons, node_of, n_steps, rc.latents(node_of, 14), 40.0)        # int(31 / 40) = 0 samples


@pytest.mark.parametrize("kind", ["none", "previous", "start_pose", "previous_spine"])
def test_assemble_walks_mixed_host_with_times_is_assemble_walk_host_per_walk(kind):
    jsons, sk = rc.primitive_jsons(), rc.skeleton()
    _, alignment, skeleton = next(a for a in rc.alignments(sk, jsons) if a[0] == kind)
    walks = rc.CONTRACT_WALKS
    node_of, n_steps = rc.tables(walks)
    P = rc.latents(node_of, 16)
    width = [L for L, _, _, _, _ in rc.SHAPES]
    times = rw.walk_time_rows_host(jsons, node_of, n_steps, P, 1.6)
    assert len({len(times[w][i]) for w, seq in enumerate(walks) for i, k in enumerate(seq) if k == 2}) > 1      # node c's rows differ in length
    frames, offsets, transforms = rw.assemble_walks_mixed_host(jsons, node_of, n_steps, P, alignment, skeleton, times=times, speed=1.6)
    plain = rw.assemble_walks_mixed_host(jsons, node_of, n_steps, P, alignment, skeleton)
    for w, seq in enumerate(walks):
        S = np.concatenate([P[w, i, :width[k]] for i, k in enumerate(seq)])[None, :]
        fr, offs, tr = gw.assemble_walk_host([jsons[k] for k in seq], S, times=[times[w]], alignment=alignment, skeleton=skeleton, speed=1.6)
        assert np.array_equal(frames[w], fr[0]) and np.array_equal(offsets[w], offs[0]) and np.array_equal(transforms[w, :len(seq)], tr[0])
        assert frames[w].shape[0] == sum(len(t) for t in times[w]) and np.isnan(transforms[w, len(seq):]).all()
        # times=None: what it returns today, the canonical grids
        fr0, offs0, tr0 = gw.assemble_walk_host([jsons[k] for k in seq], S, alignment=alignment, skeleton=skeleton)
        assert np.array_equal(plain[0][w], fr0[0]) and np.array_equal(plain[1][w], offs0[0]) and np.array_equal(plain[2][w, :len(seq)], tr0[0])


def test_the_four_entry_points_have_prototypes():
    try:
        lib = _capi.load_library()
    except OSError:
        pytest.skip("libmg_hip.so is not built")
    vp, i32, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    time_functions = [i32, vp, vp, vp, vp, i32, i64, i32, i64, dbl, vp, vp, i32]
    frames_at = [i32, vp, vp, vp, vp, i32, i64, i32, i64, vp, vp, i32, vp, vp, vp, vp, i64, vp]
    assert len(time_functions) == 13 and len(frames_at) == 18
    for name, want in (("mg_walks_time_functions", time_functions), ("mg_walks_time_functions_host", time_functions),
                       ("mg_walks_frames_at", frames_at), ("mg_walks_frames_at_host", frames_at)):
        assert name in _capi.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want and fn.restype is C.c_int, name
    assert _capi.DEVICE_TABLES["walks_warped"] == 12 and _capi.DEVICE_TABLES["walks_time"] == 13
    assert _capi.DEVICE_TABLES["walks_mixed"] == 10 and _capi.DEVICE_TABLES["walks_sample"] == 11
