"""csrc/mg_timewarp.hip at its shape edges: mg_time_function_sample / _rows against the reference's own arithmetic (scipy's splrep /
splev: timewarp_cases.reference_time_function) over the case table of tests/timewarp_cases.py, their capacity reports, exits and
refusals, mg_back_project_frames_at against mg_back_project_frames_f64 with a time grid per candidate, and the walks that reach
these kernels through graph_walk.py.  The tolerance of the times is timewarp_cases.time_tolerance: 16 x FITPACK's own
deviation from a 50-digit twin, at least 4 ulp of F, never above the suite's 1e-11 F; the times are held to FITPACK run on the
HOST's canonical time function, the statement that does not depend on the kernel."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import timewarp_cases as tc
from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import graph_walk as gw
from morphablegraphs_amd.motion_primitive import HipMotionPrimitive, get_context
from morphablegraphs_amd.motion_state_graph import HipPrimitiveSet
from test_graph_walk_host import WALK_TOLERANCE, primitive_jsons, root_scale

pytestmark = pytest.mark.gpu

TILE = _capi.MG_WALK_TILE
LENS_SENTINEL = -12345
_primitives = {}


def primitive(key, data=None):
    """One HipMotionPrimitive per model of the table (or per given JSON), kept for the module."""
    if key not in _primitives:
        mp = HipMotionPrimitive(None, context=get_context(0))
        mp._initialize_from_json(data if data is not None else tc.model_of(key)[0])
        _primitives[key] = mp
    return _primitives[key]


def sample(mp, G, speed, t_cap, pitch=None, ld=None, col0=0, rows=True, canonical=False):
    """One mg_time_function_sample (pitch None) or mg_time_function_sample_rows call over a NaN sentinel: (the whole times buffer
    (B, pitch), lengths over a sentinel of their own[, canonical_out (B, F)]).  The gamma columns lie at col0 of rows ld wide whose
    other columns hold 7.5."""
    prim, ctx = mp._prim, mp._prim.ctx
    G = np.asarray(G)
    B, Lt = G.shape
    ld = Lt if ld is None else ld
    wide = np.full((B, ld), 7.5, dtype=G.dtype)
    if ld >= col0 + Lt:
        wide[:, col0:col0 + Lt] = G
    p = t_cap if pitch is None else pitch
    F = mp.n_canonical_frames
    with ctx.buffers() as bufs:
        d_g, d_t = bufs.upload(wide), bufs.upload(np.full((B, max(p, t_cap, 1)), np.nan))
        d_l, d_c = bufs.upload(np.full(B, LENS_SENTINEL, dtype=np.int32)), (bufs.upload(np.full((B, F), np.nan)) if canonical else None)
        gp = C.c_void_p(d_g.address + col0 * wide.dtype.itemsize)
        if pitch is None:
            _capi._check(prim.lib.mg_time_function_sample(prim.handle, gp, _capi._dtype_code(wide), B, ld, float(speed), d_t.ptr, d_l.ptr, int(t_cap),
                                                          d_c.ptr if d_c is not None else None))
        else:
            _capi._check(prim.lib.mg_time_function_sample_rows(prim.handle, gp, _capi._dtype_code(wide), B, ld, float(speed), d_t.ptr, d_l.ptr, int(t_cap),
                                                               int(pitch), d_c.ptr if d_c is not None else None))
        out = (ctx.download(d_t, (B, max(p, t_cap, 1)), np.float64), ctx.download(d_l, (B,), np.int32))
        return out + (ctx.download(d_c, (B, F), np.float64),) if canonical else out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def needed(mp, G, speed):
    """The samples every row needs: a call whose rows hold 2 samples reports them negated and writes nothing (rows of 2 fit as they are)."""
    times, lens = sample(mp, G, speed, 2)
    assert np.all((lens == 2) | (lens < -2)) and np.isnan(times[lens < 0]).all()
    return np.abs(lens)


# ---- mg_time_function_sample over the case table ----------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", tc.CASE_IDS)
def test_time_functions_match_the_reference(case_id):
    _, key, (F, Lt, _, _, rows, speed) = tc.CASES[tc.CASE_IDS.index(case_id)]
    data, gamma = tc.model_of(key)
    mp = primitive(key)
    tol = tc.time_tolerance(case_id)
    host_canonical = [tc.canonical_time_function(data, g) for g in gamma]
    want_len = np.array([tc.sample_count(c, speed) + 2 for c in host_canonical])
    # 70 rows: the case's own and 67 more draws; rows of exactly the longest row's length, so that T == t_cap is written
    G70 = np.concatenate((gamma, np.random.default_rng(F * 31 + Lt).standard_normal((67, Lt))))
    need = needed(mp, G70, speed)
    assert np.array_equal(need[:rows], want_len)                                   # the sample counts: exact
    cap = int(need.max())
    t70, l70, c70 = sample(mp, G70, speed, cap, canonical=True)
    assert np.array_equal(l70, need) and not np.isnan(t70[int(np.argmax(need))]).any()
    worst, worst_host = 0.0, 0.0
    for b in range(rows):
        n = int(l70[b])
        np.testing.assert_allclose(c70[b], host_canonical[b], rtol=1e-12, atol=1e-11)       # canonical_out: the NumPy cumulative statement
        ref = tc.reference_time_function(host_canonical[b], speed)                 # the independent statement: FITPACK through the host's abscissae
        assert len(ref) == n
        worst_host = max(worst_host, float(np.max(np.abs(t70[b, :n] - ref))))
        worst = max(worst, float(np.max(np.abs(t70[b, :n] - tc.reference_time_function(c70[b], speed)))))     # (diagnostic: through the kernel's own)
    print("%s: device deviation %.3g (through the kernel's own abscissae %.3g), tolerance %.3g, e_fit %.3g, lengths %s"
          % (case_id, worst_host, worst, tol, tc.case_figures(case_id)[0], l70[:rows].tolist()))
    assert worst_host <= tol
    for b in range(70):
        n = int(l70[b])
        assert same_bits(t70[b, 0], 0.0) and same_bits(t70[b, n - 1], F - 1.0)      # the pinned ends, exactly
        assert not np.isnan(t70[b, :n]).any() and np.isnan(t70[b, n:]).all()       # everything behind a row's length keeps the sentinel
    # batches of 3 and 1: a row alone is the row inside a batch, bit for bit
    t3, l3 = sample(mp, gamma, speed, cap)
    assert np.array_equal(l3, l70[:3]) and same_bits(t3, t70[:3])
    for b in (0, 2, 69):
        t1, l1 = sample(mp, G70[b:b + 1], speed, cap)
        assert l1[0] == l70[b] and same_bits(t1[0], t70[b])
    # float32 gamma is the float64 result of the widened values
    G32 = G70[:3].astype(np.float32)
    t32, l32, c32 = sample(mp, G32, speed, cap, canonical=True)
    tw, lw, cw = sample(mp, G32.astype(np.float64), speed, cap, canonical=True)
    assert np.array_equal(l32, lw) and same_bits(t32, tw) and same_bits(c32, cw)
    # gamma columns from inside a wider row
    for G in (G70[:3], G32):
        ta, la = sample(mp, G, speed, cap, ld=Lt + 3, col0=2)
        tb, lb = sample(mp, G, speed, cap)
        assert np.array_equal(la, lb) and same_bits(ta, tb)
    # rows one sample too short for the longest row: it reports -T and keeps its sentinel, the others are what they were
    if cap > 2:
        ts, ls = sample(mp, G70, speed, cap - 1)
        long = need == cap
        assert np.array_equal(ls[long], -need[long]) and np.isnan(ts[long]).all()
        assert np.array_equal(ls[~long], need[~long]) and same_bits(ts[~long], t70[~long, :cap - 1])


# ---- capacity and exits ---------------------------------------------------------------------------------------------------
def test_a_count_of_zero_fits_rows_of_two():
    data, gamma = tc.model_of("count0")
    times, lens = sample(primitive("count0"), gamma, tc.CONSTANT["count0"][5], 2)
    assert np.array_equal(lens, [2, 2, 2]) and same_bits(times, np.tile([0.0, 3.0], (3, 1)))


def _overflowing_gamma(data, Lt):
    for sign in (1.0, -1.0):
        g = np.full(Lt, sign * 1.0e6)
        with np.errstate(over="ignore", invalid="ignore"):
            if not np.isfinite(tc.canonical_time_function(data, g)[-2]):
                return g
    raise AssertionError("no overflowing gamma")


@pytest.mark.parametrize("key", [(5, 1), (65, 2)])
def test_a_time_function_that_is_not_finite_has_no_row(key):
    data, gamma = tc.model_of(key)
    mp = primitive(key)
    G = np.stack((gamma[0], _overflowing_gamma(data, key[1]), gamma[1]))
    cap = int(needed(mp, gamma, 1.0).max()) + 3
    times, lens = sample(mp, G, 1.0, cap)
    assert lens[1] == 0 and np.isnan(times[1]).all()
    for b, g in ((0, gamma[0]), (2, gamma[1])):                                    # the rows before and after it are their stand-alone values
        t1, l1 = sample(mp, g[None, :], 1.0, cap)
        assert lens[b] == l1[0] > 0 and same_bits(times[b], t1[0])


def test_more_than_2_to_the_24_samples_has_no_row():
    data = tc.time_model(2048, 1, 20, 1.0e-3, 77, constant=9.1, name="tw_huge")     # t(F - 2) = 2047 e^9.1 - 1 = 1.83e7 > 2^24
    gamma = np.zeros((2, 1))
    assert np.isfinite(tc.canonical_time_function(data, gamma[0])[-2]) and tc.canonical_time_function(data, gamma[0])[-2] > 2.0 ** 24
    times, lens = sample(primitive("huge", data), gamma, 1.0, 64)
    assert np.array_equal(lens, [0, 0]) and np.isnan(times).all()


def test_bad_calls_are_refused_before_any_launch():
    mp = primitive((6, 2))
    gamma = tc.model_of((6, 2))[1]
    cases = []
    for F in (3, 2049):                                                            # below and above what the inversion holds in LDS
        data = tc.time_model(F, 1, 4 if F == 3 else 20, 0.05, 30 + F, name="tw_refused_%d" % F)
        cases.append((_capi.MG_ERR_UNSUPPORTED, "%d canonical frames (4 .. 2048 supported)" % F, dict(mp=primitive(("refused", F), data), G=np.zeros((1, 1)), speed=1.0, t_cap=16)))
    cases.append((_capi.MG_ERR_INVALID_ARGUMENT, "t_cap >= 2", dict(mp=mp, G=gamma, speed=1.0, t_cap=1)))
    for speed in (0.0, -1.0, np.inf, np.nan):
        cases.append((_capi.MG_ERR_INVALID_ARGUMENT, "speed must be positive and finite", dict(mp=mp, G=gamma, speed=speed, t_cap=16)))
    cases.append((_capi.MG_ERR_INVALID_ARGUMENT, "a row pitch of 15 doubles is shorter than t_cap 16", dict(mp=mp, G=gamma, speed=1.0, t_cap=16, pitch=15)))
    cases.append((_capi.MG_ERR_INVALID_ARGUMENT, "bad arguments (ld 1, n_time_components 2)", dict(mp=mp, G=gamma, speed=1.0, t_cap=16, ld=1)))
    untimed = primitive("untimed", primitive_jsons()[0])
    cases.append((_capi.MG_ERR_INVALID_ARGUMENT, "the primitive has no time model", dict(mp=untimed, G=np.zeros((1, 1)), speed=1.0, t_cap=16)))
    for status, text, kw in cases:
        with pytest.raises(_capi.MGError) as e:
            sample(**kw)
        assert e.value.status == status and text in str(e.value), (text, str(e.value))
    times, lens = sample(mp, gamma, 1.0, 16)                                       # the context still works
    assert np.all(lens > 2) and same_bits(times[:, 0], np.zeros(3))


# ---- mg_time_function_sample_rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,speed", [((5, 5), 0.37), ((64, 2), 1.0), ((129, 1), 1.6)])
def test_rows_at_a_pitch_are_the_rows_back_to_back(key, speed):
    mp = primitive(key)
    G = np.concatenate((tc.model_of(key)[1], np.random.default_rng(1).standard_normal((4, key[1]))))
    cap = int(needed(mp, G, speed).max()) + 1                                      # one sample of room: rows end before t_cap
    want, want_len, want_c = sample(mp, G, speed, cap, canonical=True)
    for pitch in (cap, cap + 1, 3 * cap):
        got, lens, c = sample(mp, G, speed, cap, pitch=pitch, canonical=True)
        assert np.array_equal(lens, want_len) and same_bits(got[:, :cap], want) and same_bits(c, want_c)
        assert np.isnan(got[:, cap:]).all()                                        # every double between a row's t_cap and the next row's start


# ---- mg_back_project_frames_at ------------------------------------------------------------------------------------------
def _spatial(n_dim, n_components, F=20, seed=50):
    key = ("spatial", n_dim, n_components, F)
    data = synthetic.make_primitive(seed=seed + n_dim + n_components, n_components=n_components, n_frames=F, n_basis=tc.N_BASIS, n_dim=n_dim, n_gmm=2,
                                    name="fa_%d_%d_%d" % (n_dim, n_components, F))
    return primitive(key, data), data


def _frames_by_grid(prim, S, times):
    grid = prim.time_grid(times)
    try:
        return prim.back_project_frames_f64(S, grid)[0]
    finally:
        grid.close()


@pytest.mark.parametrize("t_cap", [1, 255, 256, 257])
@pytest.mark.parametrize("n_dim,n_components", [(11, 3), (3, 1)])
def test_frames_at_are_the_float64_frames_of_a_grid_per_candidate(t_cap, n_dim, n_components):
    mp, _ = _spatial(n_dim, n_components)
    prim, F, L = mp._prim, mp.n_canonical_frames, n_components
    rng = np.random.default_rng(t_cap)
    lengths = np.array([t_cap, 0, -3, t_cap + 1, max(1, t_cap - 1), t_cap], dtype=np.int32)
    S = 0.7 * rng.standard_normal((len(lengths), L))
    times = np.sort(rng.uniform(0.0, F - 1.0, (len(lengths), t_cap)), axis=1)
    got = prim.back_project_frames_at(S, times, lengths)
    full = prim.back_project_frames_at(S, times, None)                              # lengths NULL: every row has t_cap samples
    wide32 = np.concatenate((S, np.full((len(S), 2), 9.0)), axis=1).astype(np.float32)       # float32 latents in rows wider than L
    got32 = prim.back_project_frames_at(wide32, times, lengths)
    out32 = prim.back_project_frames_at(S, times, lengths, dtype=np.float32)
    for b, n in enumerate(lengths):
        if n <= 0 or n > t_cap:
            assert np.isnan(got[b]).all() and np.isnan(got32[b]).all() and np.isnan(out32[b]).all()       # skipped: the sentinel stays
        else:
            want = _frames_by_grid(prim, S[b:b + 1], times[b, :n])
            assert same_bits(got[b, :n], want) and np.isnan(got[b, n:]).all()
            assert same_bits(got32[b, :n], _frames_by_grid(prim, wide32[b:b + 1, :L].astype(np.float64), times[b, :n])) and np.isnan(got32[b, n:]).all()
            assert np.array_equal(out32[b, :n].view(np.uint32), want.astype(np.float32).view(np.uint32)) and np.isnan(out32[b, n:]).all()
        assert same_bits(full[b], _frames_by_grid(prim, S[b:b + 1], times[b]))


@pytest.mark.parametrize("n_dim,n_components", [(11, 3), (3, 1)])
def test_frames_at_on_the_knots_and_outside_them(n_dim, n_components):
    """the l == n - k - 2 stop of mg_basis_row_dev: every interior knot, F - 1 (the last knot), F and -0.5"""
    mp, data = _spatial(n_dim, n_components)
    prim, F = mp._prim, mp.n_canonical_frames
    knots = np.asarray(data["b_spline_knots_spatial"])
    special = np.concatenate((knots[4:-4], [F - 1.0, float(F), -0.5, 0.0, np.nextafter(F - 1.0, 0.0)]))
    S = 0.7 * np.random.default_rng(6).standard_normal((2, n_components))
    times = np.stack((special, special[::-1]))
    got = prim.back_project_frames_at(S, times, None)
    host = gw._HostModel(data)
    for b in range(2):
        assert same_bits(got[b], _frames_by_grid(prim, S[b:b + 1], times[b]))
        _, want = host.frames(S[b], times[b])
        scale = max(1.0, float(np.max(np.abs(want))))
        worst = float(np.max(np.abs(got[b] - want)))
        print("special times, D = %d, row %d: %.3g of the scale %.4g" % (n_dim, b, worst / scale, scale))
        assert worst <= 4e-12 * scale


def test_frames_at_up_to_the_lds_budget():
    mp, _ = _spatial(11, 3)
    prim, F = mp._prim, mp.n_canonical_frames
    R, L = tc.N_BASIS * 11, 3
    fits = lambda t: (R + L + 4 * t) * 8 + 4 * t + 16 <= 160 * 1024 - 64          # mg_launch_frames_at's budget
    t_max = (160 * 1024 - 64 - 16 - 8 * (R + L)) // 36
    assert fits(t_max) and not fits(t_max + 1)
    rng = np.random.default_rng(3)
    S = 0.7 * rng.standard_normal((2, L))
    times = np.sort(rng.uniform(0.0, F - 1.0, (2, t_max)), axis=1)
    got = prim.back_project_frames_at(S, times, np.array([t_max, t_max - 1], dtype=np.int32))
    assert same_bits(got[0], _frames_by_grid(prim, S[0:1], times[0]))
    assert same_bits(got[1, :t_max - 1], _frames_by_grid(prim, S[1:2], times[1, :t_max - 1])) and np.isnan(got[1, t_max - 1]).all()
    with pytest.raises(_capi.MGError) as e:
        prim.back_project_frames_at(S, np.zeros((2, t_max + 1)), None)
    assert e.value.status == _capi.MG_ERR_UNSUPPORTED and "%d time samples per candidate do not fit LDS" % (t_max + 1) in str(e.value)
    assert same_bits(prim.back_project_frames_at(S, times[:, :8], None)[0], _frames_by_grid(prim, S[0:1], times[0, :8]))       # the context still works


# ---- walks --------------------------------------------------------------------------------------------------------------
class _Graph(object):
    def __init__(self, pset):
        self.nodes = {("walk", name): node for name, node in pset.nodes.items()}


@pytest.fixture(scope="module")
def graph():
    """w0 .. w2 without a time model (12, 33, 20 frames); `timed` (F = 16, Lt = 2, mild); `long` (the table's long_row: F = 64, about
    283 samples); m31, m32, m33: F = 16 with constant log-increments that give tile - 1, tile and tile + 1 samples."""
    jsons = primitive_jsons()
    jsons.append(synthetic.make_primitive(seed=90, n_components=4, n_frames=16, n_basis=6, n_dim=tc.D, n_gmm=2, name="timed", n_time_components=2, n_basis_time=5))
    long = dict(tc.model_of("long_row")[0])
    long["name"] = "long"
    jsons.append(long)
    for n in (TILE - 1, TILE, TILE + 1):                                           # T = round(15 e^c - 1) + 2 = n
        jsons.append(tc.time_model(16, 1, 5, 1.0e-3, 160 + n, constant=float(np.log((n - 1) / 15.0)), name="m%d" % n))
    return _Graph(HipPrimitiveSet(jsons))


def _walk_case(graph, names, n_walks, seed):
    keys = [("walk", n) for n in names]
    mps = [graph.nodes[k] for k in keys]
    rng = np.random.default_rng(seed)
    S = 0.7 * rng.standard_normal((n_walks, sum(mp.get_n_spatial_components() for mp in mps)))
    G = rng.standard_normal((n_walks, sum(mp.get_n_time_components() for mp in mps)))
    return keys, mps, S, G


def _chain(mps, S, G, speed, alignment=None):
    """The reference's chain: back_project(s, True, speed) step by step, the steps' own time functions aligned and appended by
    assemble_walk_host.  Returns (frames, offsets, the frames' largest slope against time)."""
    times, slope = [], 0.0
    for w in range(len(S)):
        row, so, go = [], 0, 0
        for mp in mps:
            ns, nt = mp.get_n_spatial_components(), mp.get_n_time_components()
            spline = mp.back_project(np.concatenate((S[w, so:so + ns], G[w, go:go + nt])), True, speed)
            t = np.asarray(spline.time_function, dtype=np.float64)
            fr = np.asarray(spline.get_motion_vector())
            dt = np.diff(t)
            ok = dt > 0
            if ok.any():
                slope = max(slope, float(np.max(np.max(np.abs(np.diff(fr, axis=0)), axis=1)[ok] / dt[ok])))
            row.append(t)
            so, go = so + ns, go + nt
        times.append(row)
    ref, offsets, _ = gw.assemble_walk_host(mps, S, times=times, alignment=alignment)
    return ref, offsets, slope


def _assert_walk(got, ref, slope, time_tol):
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    worst, bound = float(np.nanmax(np.abs(got - ref))), WALK_TOLERANCE * root_scale(ref) + time_tol * slope
    print("walk: disagreement %.3g, bound %.3g (root scale %.4g, largest slope %.4g, time tolerance %.3g)" % (worst, bound, root_scale(ref), slope, time_tol))
    assert worst <= bound


def _device_walk(graph, keys, S, G, speed, row=0):
    walk = gw.HipGraphWalk(graph, use_time_parameters=True)
    so, go = 0, 0
    for k in keys:
        node = graph.nodes[k]
        ns, nt = node.get_n_spatial_components(), node.get_n_time_components()
        walk.steps.append(gw.HipGraphWalkStep.from_graph(graph, k, np.concatenate((S[row, so:so + ns], G[row, go:go + nt]))))
        so, go = so + ns, go + nt
    walk.convert_graph_walk_to_quaternion_frames(use_time_parameters=True, step_size=speed)
    return walk


@pytest.mark.parametrize("speed", [1.6, 0.5])
def test_a_walk_mixes_timed_and_untimed_steps_at_a_speed(graph, speed):
    keys, mps, S, G = _walk_case(graph, ["timed", "w0", "timed", "w2"], 3, 14)
    ref, offsets, slope = _chain(mps, S, G, speed)
    tol_t = 4.0 * np.spacing(16.0)
    assert np.all(np.diff(offsets, axis=1)[:, 1] == int(12 * (1.0 / speed))) and np.all(np.diff(offsets, axis=1)[:, 3] == int(20 * (1.0 / speed)))
    frames, offs = gw.assemble_walks(graph, keys, S, time_parameters=G, speed=speed)
    assert np.array_equal(offs, offsets)
    _assert_walk(frames, ref, slope, tol_t)
    walk = _device_walk(graph, keys, S, G, speed, row=1)
    n = int(offsets[1, -1])
    assert walk.get_num_of_frames() == n and [s.start_frame for s in walk.steps] == offsets[1, :-1].tolist()
    _assert_walk(walk.get_quat_frames()[None], ref[1:2, :n], slope, tol_t)
    walk.close()


def test_a_walk_whose_step_needs_more_rows_than_assumed(graph):
    keys, mps, S, G = _walk_case(graph, ["w0", "long", "w2"], 2, 15)
    ref, offsets, slope = _chain(mps, S, G, 1.0)
    lengths = np.diff(offsets, axis=1)
    assert np.all(lengths[:, 1] > 4 * 64 + 8)                                      # beyond the rows assumed for the step before its length is known
    tol_t = tc.time_tolerance("long_row")
    frames, offs = gw.assemble_walks(graph, keys, S, time_parameters=G)
    assert np.array_equal(offs, offsets)
    _assert_walk(frames, ref, slope, tol_t)
    # a single long step: more than the whole walk's assumed rows, on the store that grows
    keys1, mps1, S1, G1 = _walk_case(graph, ["long"], 1, 16)
    ref1, offsets1, slope1 = _chain(mps1, S1, G1, 1.0)
    assert offsets1[0, -1] > 4 * 64 + 8
    walk = _device_walk(graph, keys1, S1, G1, 1.0)
    assert walk.get_num_of_frames() == offsets1[0, -1]
    _assert_walk(walk.get_quat_frames()[None], ref1, slope1, tol_t)
    walk.close()
    frames1, offs1 = gw.assemble_walks(graph, keys1, S1, time_parameters=G1)
    assert np.array_equal(offs1, offsets1)
    _assert_walk(frames1, ref1, slope1, tol_t)


def test_time_functions_give_lengths_around_the_tile(graph):
    names = ["m%d" % (TILE - 1), "m%d" % TILE, "m%d" % (TILE + 1), "m%d" % TILE]
    keys, mps, S, G = _walk_case(graph, names, 3, 17)
    ref, offsets, slope = _chain(mps, S, G, 1.0)
    assert np.array_equal(np.diff(offsets, axis=1), np.tile([TILE - 1, TILE, TILE + 1, TILE], (3, 1)))
    frames, offs = gw.assemble_walks(graph, keys, S, time_parameters=G)
    assert np.array_equal(offs, offsets)
    _assert_walk(frames, ref, slope, 4.0 * np.spacing(16.0))
    walk = _device_walk(graph, keys, S, G, 1.0, row=2)
    assert walk.get_num_of_frames() == offsets[2, -1] and [s.start_frame for s in walk.steps] == offsets[2, :-1].tolist()
    _assert_walk(walk.get_quat_frames()[None], ref[2:3], slope, 4.0 * np.spacing(16.0))
    walk.close()


def test_a_timed_walk_one_step_past_the_call_limit_is_joined_from_pieces(graph):
    """assemble_walks samples the time tables of every (walk, piece) before it sizes the frame rows: 65 steps, two pieces, two walks"""
    names = [("timed", "w0", "m%d" % TILE)[i % 3] for i in range(_capi.MG_WALK_MAX_STEPS + 1)]
    keys, mps, S, G = _walk_case(graph, names, 2, 18)
    ref, offsets, slope = _chain(mps, S, G, 1.6)
    frames, offs = gw.assemble_walks(graph, keys, S, time_parameters=G, speed=1.6)
    assert np.array_equal(offs, offsets)
    _assert_walk(frames, ref, slope, 4.0 * np.spacing(16.0))
    walk = _device_walk(graph, keys, S, G, 1.6, row=1)
    assert walk.get_num_of_frames() == offsets[1, -1]
    _assert_walk(walk.get_quat_frames()[None], ref[1:2, :int(offsets[1, -1])], slope, 4.0 * np.spacing(16.0))
    walk.close()
