"""The Savitzky-Golay pass as a table, without a device: time_smoothing.savgol_hat_matrix against exact rationals and against the
stand-alone program over csrc/mg_savgol_table.h, smooth_time_row_host against scipy.signal.savgol_filter(row, 15, 3), the routing of
the opt-in (HipMotionPrimitive.smooth_on_device) with the library stubbed, and the frames at the smoothed end times -- below 0 and
off F - 1 -- against scipy's splev on the primitive's own knots.

BOUNDS.  Against savgol_filter: 1e-12 F, the bound the time warp is held to against FITPACK (csrc/mg_timewarp.hip); measured 7e-15
of the row's largest value.  The frames outside [0, F - 1]: 4e-12 of the scale, tests/test_gpu_timewarp_shapes.py's bound for
mg_back_project_frames_at on and outside the knots."""
import os
import subprocess
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import random_walk_cases as rc
from morphablegraphs_amd import _capi, feature_point_model as fpm, graph_walk as gw, random_walks as rw, time_smoothing as ts
from morphablegraphs_amd.motion_primitive import HipMotionPrimitive

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
LENGTHS = [15, 16, 21, 22, 29, 30, 78, 79, 142, 143]


def _monotone_row(T, F, seed):
    """A time function's shape: T samples rising from 0 to F - 1."""
    steps = np.random.default_rng(seed).uniform(0.2, 1.8, T - 1)
    return np.concatenate(([0.0], np.cumsum(steps) * ((F - 1.0) / steps.sum())[()]))[:T] * 1.0


# ---- the table ----------------------------------------------------------------------------------------------------------------
def test_the_hat_matrix_is_the_projection_rounded_once():
    H = ts.savgol_hat_matrix()
    assert H.shape == (15, 15) and H.dtype == np.float64
    classic = [-78, -13, 42, 87, 122, 147, 162, 167, 162, 147, 122, 87, 42, -13, -78]
    assert all(H[7, k] == classic[k] / 1105 for k in range(15))
    assert np.array_equal(H, H.T)
    assert np.abs(H @ H - H).max() <= 1e-15
    exact = ts._hat_matrix_fractions()
    for i in range(15):
        for j in range(15):
            f = exact[i][j]
            got = Fraction(float(H[i, j]))
            lo, hi = Fraction(float(np.nextafter(H[i, j], -np.inf))), Fraction(float(np.nextafter(H[i, j], np.inf)))
            assert abs(got - f) <= abs(lo - f) and abs(got - f) <= abs(hi - f), (i, j)                  # no neighbour is nearer
    assert exact[7][7] == Fraction(167, 1105) and sum(exact[0]) == 1


def test_the_native_table_has_the_same_225_doubles():
    subprocess.check_call(["make", "-s", "-C", NATIVE, "-f", "savgol_table_check.mk", "savgol_table_check"])
    done = subprocess.run([os.path.join(NATIVE, "savgol_table_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert done.returncode == 0, done.stderr.decode()
    lines = done.stdout.decode().split("\n")[:-1]
    assert len(lines) == 225
    H = ts.savgol_hat_matrix()
    for line in lines:
        i, j, value = line.split()
        assert float.fromhex(value) == H[int(i), int(j)], line


# ---- the statement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", LENGTHS)
def test_the_statement_is_savgol_filter(T):
    from scipy.signal import savgol_filter
    worst = 0.0
    for F in (16, 65, 200):
        for seed in range(5):
            row = _monotone_row(T, F, 1000 * T + seed)
            assert row[0] == 0.0 and abs(row[-1] - (F - 1.0)) <= 1e-12 * F and (np.diff(row) > 0).all()
            got = ts.smooth_time_row_host(row)
            err = float(np.abs(got - savgol_filter(row, 15, 3)).max())
            worst = max(worst, err / F)
            assert err <= 1e-12 * F, (T, F, seed, err)
    print("T = %d: %.3g of F" % (T, worst))


def test_the_windows_edges():
    with pytest.raises(ValueError, match="window_length must be less than or equal to the size of x"):
        ts.smooth_time_row_host(_monotone_row(14, 20, 1))
    # T = 15: every sample reads all 15 -- sample q is row q of H on them, the matrix product H row.  Its exact statement is the sum in
    # the kernels' order with plain Python floats (no fused multiply-add, no blocked summation: what `H @ row` through BLAS may use,
    # which is why that product is held to rounding instead of bits)
    H, row = ts.savgol_hat_matrix(), _monotone_row(15, 40, 2)
    assert [ts.smooth_window(q, 15) for q in range(15)] == [(q, 0) for q in range(15)]
    want = []
    for q in range(15):
        acc = float(H[q, 0]) * float(row[0])
        for k in range(1, 15):
            acc = acc + float(H[q, k]) * float(row[k])
        want.append(acc)
    got = ts.smooth_time_row_host(row)
    assert np.array_equal(got, np.array(want))
    assert np.abs(got - H @ row).max() <= 16 * 2.0 ** -53 * float(np.abs(H).sum(axis=1).max() * np.abs(row).max())
    # the case split of a longer row
    assert [ts.smooth_window(q, 22) for q in (0, 6, 7, 14, 15, 21)] == [(0, 0), (6, 0), (7, 0), (7, 7), (8, 7), (14, 7)]
    times = np.stack((np.pad(_monotone_row(20, 30, 3), (0, 5)), np.full(25, 3.5)))
    out = ts.smooth_time_rows_host(times, [20, 0])
    assert np.array_equal(out[0, :20], ts.smooth_time_row_host(times[0, :20])) and np.array_equal(out[0, 20:], times[0, 20:]) and np.array_equal(out[1], times[1])
    with pytest.raises(ValueError, match="row 1: 9 samples"):
        ts.smooth_time_rows_host(times, [20, 9])
    with pytest.raises(ValueError, match=r"walk 1, step 0: 14 samples: If mode is 'interp', window_length"):
        ts.require_smoothing_window(np.array([[15, 0], [14, 3]]), "walk %d, step %d")
    ts.require_smoothing_window(np.array([0, 15, 200]), "candidate %d")


# ---- the opt-in, the library stubbed --------------------------------------------------------------------------------------------
class _Prim(object):
    """What HipMotionPrimitive asks of its _capi.Primitive on the time path."""

    def __init__(self, row):
        self.row, self.calls = row, []

    def time_function_sample(self, gamma, speed=1.0, **kw):
        self.calls.append(("sample", kw))
        B = len(gamma)
        return np.tile(np.pad(self.row, (0, 3), constant_values=np.nan), (B, 1)), np.full(B, len(self.row), dtype=np.int32)

    def back_project_frames_at(self, S, times, lens, dtype=np.float64):
        self.calls.append(("frames_at", times.copy()))
        return np.zeros(times.shape + (3,))

    def back_project_warped_smoothed(self, S, n_s, speed, dtype=np.float64):
        self.calls.append(("warped_smoothed", n_s))
        return "frames", "lens", "times"


def _primitive(row, smooth, on_device):
    mp = HipMotionPrimitive()
    mp._prim, mp.s_pca, mp.has_time_parameters = _Prim(row), {"n_components": 2}, True
    mp.smooth_time_parameters = smooth
    if on_device is not None:
        mp.smooth_on_device = on_device
    return mp


def test_the_primitive_smooths_on_the_host_unless_it_opts_in():
    from scipy.signal import savgol_filter
    row = _monotone_row(20, 30, 7)
    assert HipMotionPrimitive().smooth_on_device is False
    for on_device in (None, False):
        mp = _primitive(row, True, on_device)
        got = mp.back_project_time_function(np.zeros(2))
        assert np.array_equal(got, np.array(savgol_filter(row, 15, 3))) and mp._prim.calls == [("sample", {})]           # scipy's bits, as today
        mp._prim.calls = []
        frames, lens, times = mp.back_project_warped_batch(np.zeros((2, 4)))
        assert [c[0] for c in mp._prim.calls] == ["sample", "frames_at"] and mp._prim.calls[0][1] == {}
        assert np.array_equal(mp._prim.calls[1][1], np.tile(savgol_filter(row, 15, 3), (2, 1)))                      # smoothed on the host, uploaded again
    plain = _primitive(row, False, True)                                          # the switch alone changes nothing
    assert np.array_equal(plain.back_project_time_function(np.zeros(2)), row) and plain._prim.calls == [("sample", {})]
    mp = _primitive(row, True, True)
    mp._smooth_time_function = None                                               # (the host pass is not reached)
    assert np.array_equal(mp.back_project_time_function(np.zeros(2)), row) and mp._prim.calls == [("sample", {"smoothed": True})]
    assert mp.back_project_warped_batch(np.zeros((2, 4))) == ("frames", "lens", "times") and mp._prim.calls[-1] == ("warped_smoothed", 2)
    short = _primitive(row[:14], True, True)
    with pytest.raises(ValueError, match="candidate 0: 14 samples"):
        short.back_project_time_function(np.zeros(2))


class _Buffer(object):
    address = 4096


class _Buffers(object):
    def __init__(self, log):
        self.log, self.bufs = log, []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def upload(self, array):
        self.log.append(("upload", np.asarray(array).shape))
        return _Buffer()

    def malloc(self, n):
        return _Buffer()

    def release(self, buf):
        return buf


class _Ctx(object):
    def __init__(self, lengths):
        self.lengths, self.log = lengths, []

    def buffers(self):
        return _Buffers(self.log)

    def download(self, buf, shape, dtype):
        self.log.append(("download", tuple(shape)))
        return np.full(shape, self.lengths, dtype=dtype) if np.dtype(dtype) == np.int32 else np.tile(_monotone_row(shape[-1], 30, 1), shape[:-1] + (1,))


def _step(lib, smooth, on_device, log):
    def smoother(row):
        log.append(("host_pass", len(row)))
        return row
    return types.SimpleNamespace(has_time_parameters=True, get_n_time_components=lambda: 2, n_canonical_frames=30, smooth_time_parameters=smooth,
                                 smooth_on_device=on_device, _smooth_time_function=smoother, _prim=types.SimpleNamespace(lib=lib, handle=None))


@pytest.mark.parametrize("on_device", [False, True])
def test_graph_walk_times_smooth_where_the_primitive_says(on_device):
    calls = []
    lib = types.SimpleNamespace(mg_time_function_sample_rows=lambda *a: calls.append("rows") or 0,
                                mg_time_function_sample_smoothed_rows=lambda *a: calls.append("smoothed_rows") or 0)
    ctx = _Ctx(20)
    mps = [_step(lib, True, on_device, ctx.log), _step(lib, False, on_device, ctx.log)]
    G = np.zeros((3, 4))
    d_t, lengths, t_cap = gw._sample_times(ctx, _Buffers(ctx.log), mps, _Buffer(), G, [0, 2], 1.0)
    assert (lengths == 20).all() and t_cap == 128
    if on_device:
        assert calls == ["smoothed_rows", "rows"]
        assert [e for e in ctx.log if e[0] in ("host_pass", "upload")] == [] and ctx.log == [("download", (2, 3))]   # the lengths alone cross the bus
    else:
        assert calls == ["rows", "rows"]
        assert [e for e in ctx.log if e[0] == "host_pass"] == [("host_pass", 20)] * 3 and ("upload", (3, 2, 128)) in ctx.log        # as today
    short = _Ctx(14)
    mps = [_step(lib, False, True, short.log), _step(lib, True, True, short.log)]
    with pytest.raises(ValueError, match=r"walk 0, step 1: 14 samples"):
        gw._sample_times(short, _Buffers(short.log), mps, _Buffer(), G, [0, 2], 1.0)


@pytest.mark.parametrize("on_device", [False, True])
def test_random_walks_refuse_or_call_the_smoothed_entry_point(monkeypatch, on_device):
    calls = []
    monkeypatch.setattr(rw, "walks_time_functions_dev", lambda *a: calls.append(("plain",)))
    monkeypatch.setattr(rw, "walks_time_functions_smoothed_dev", lambda prims, node_of, n_steps, smooth, *a: calls.append(("smoothed", list(smooth))))
    node = lambda timed, smooth: types.SimpleNamespace(has_time_parameters=timed, get_n_time_components=lambda: 2 if timed else 0, n_canonical_frames=30,
                                                       smooth_time_parameters=smooth, smooth_on_device=on_device)
    walks = object.__new__(rw.RandomWalks)
    walks._mps, walks._prims = [node(True, True), node(True, False), node(False, True)], ["p0", "p1", "p2"]
    walks.node_of, walks.n_steps = np.array([[0, 1], [2, -1]], dtype=np.int32), np.array([2, 1], dtype=np.int32)
    walks.parameters, walks.dtype, walks.ld, walks.ctx = _Buffer(), np.dtype(np.float64), 8, _Ctx(20)
    if not on_device:
        with pytest.raises(NotImplementedError, match="Savitzky-Golay"):
            walks.time_functions()
        assert calls == []
        walks._mps[0].smooth_time_parameters = False                              # nothing smoothed: the plain entry point, as today
        walks.time_functions()
        assert calls == [("plain",)]
        return
    d_t, lengths, t_cap = walks.time_functions()
    assert calls == [("smoothed", [True, False, False])] and t_cap == 128
    walks.ctx = _Ctx(14)
    with pytest.raises(ValueError, match=r"walk 0, step 0: 14 samples"):
        walks.time_functions()


def test_feature_points_refuse_or_call_the_smoothed_entry_point(monkeypatch):
    calls = []

    def warped(items, wanted, **kw):
        calls.append((len(items), kw))
        return [dict({"root_end": np.zeros((3, 2)), "heading_end": np.zeros((3, 2)), "heading_len": np.ones(3)}, n_frames=np.array(frames, dtype=np.int32))
                for _ in items]
    monkeypatch.setattr(_capi, "feature_points_warped", warped)
    node = lambda smooth, on_device: types.SimpleNamespace(name="t", has_time_parameters=True, t_pca={"n_components": 2}, smooth_time_parameters=smooth,
                                                           smooth_on_device=on_device, _prim="prim")
    frames = [20, 15, 31]
    with pytest.raises(NotImplementedError, match="Savitzky-Golay"):                  # as today
        fpm.HipFeaturePointModel(node(True, False), None, latents=np.zeros((3, 5)), time_warped=True).create_root_pos_ori(3)
    assert calls == []
    fpm.HipFeaturePointModel(node(False, True), None, latents=np.zeros((3, 5)), time_warped=True).create_root_pos_ori(3)
    assert calls == [(1, {})]                                                         # the switch alone: the plain warped call, as today
    model = fpm.HipFeaturePointModel(node(True, True), None, latents=np.zeros((3, 5)), time_warped=True)
    model.create_root_pos_ori(3)
    assert calls[-1] == (1, {"smooth": [True]}) and len(model.root_pos) == 3
    frames = [20, 14, 31]
    with pytest.raises(ValueError, match="candidate 1: 14 samples: If mode is 'interp', window_length"):
        fpm.HipFeaturePointModel(node(True, True), None, latents=np.zeros((3, 5)), time_warped=True).create_root_pos_ori(3)


# ---- the host twins --------------------------------------------------------------------------------------------------------------
def test_the_host_twins_apply_the_statement():
    jsons = rc.primitive_jsons()
    node_of, n_steps = rc.tables([[2, 0], [2]])
    P = rc.latents(node_of, 16)
    plain = rw.walk_time_rows_host(jsons, node_of, n_steps, P)
    smoothed = rw.walk_time_rows_host(jsons, node_of, n_steps, P, smooth=[True, False, True])
    for w, i, same in ((0, 0, False), (0, 1, True), (1, 0, False)):
        want = plain[w][i] if same else ts.smooth_time_row_host(plain[w][i])
        assert np.array_equal(smoothed[w][i], want)
    with pytest.raises(ValueError, match="window_length"):
        rw.walk_time_rows_host(jsons, node_of, n_steps, P, speed=8.0, smooth=[False, False, True])
    S = P[:, 0, :14]
    a, b = fpm.feature_points_warped_host(jsons[2], S, frame_idx=9), fpm.feature_points_warped_host(jsons[2], S, frame_idx=9, smooth=True)
    assert np.array_equal(a["n_frames"], b["n_frames"]) and (a["n_frames"] >= 15).all()
    for r in range(len(S)):
        assert b["time_mid"][r] == ts.smooth_time_row_host(plain[r][0])[9] != a["time_mid"][r]
    assert not np.array_equal(a["start_root"], b["start_root"]) and np.isfinite(b["root_end"]).all()


# ---- times outside [0, F - 1] ------------------------------------------------------------------------------------------------------
def test_frames_at_the_smoothed_end_times_are_splev_on_the_end_pieces():
    """Smoothing moves the first time below 0 (or above) and the last one off F - 1.  The frames statements find the knot span as
    FITPACK's splev does (ext = 0) and evaluate the END piece's polynomial there: extrapolation, not clamping."""
    from scipy.interpolate import splev
    data = rc.primitive_jsons()[2]
    host = gw._HostModel(data)
    F, L = host.n_canonical_frames, host.n_components
    node_of, n_steps = rc.tables([[2], [2], [2]])
    P = rc.latents(node_of, 16, seed=8)
    rows = rw.walk_time_rows_host([data] * 3, node_of, n_steps, P, smooth=[False, False, True])
    seen_below = False
    for w in range(3):
        times = np.array([rows[w][0][0], rows[w][0][-1], -0.75, F - 0.25])          # (and one time on each side for certain)
        seen_below = seen_below or times[0] < 0.0
        assert times[0] != 0.0 and times[1] != F - 1.0
        cp, got = host.frames(P[w, 0, :L], times)
        want = np.stack([splev(times, (host.knots, cp[:, d].copy(), 3)) for d in range(cp.shape[1])], axis=1)
        scale = max(1.0, float(np.abs(want).max()))
        worst = float(np.abs(got - want).max())
        print("walk %d: times %s: %.3g of the scale %.4g" % (w, times, worst / scale, scale))
        assert worst <= 4e-12 * scale
        inside = host.frames(P[w, 0, :L], np.clip(times, 0.0, F - 1.0))[1]
        assert np.abs(inside[2:] - got[2:]).max() > 1e-6 * scale                      # clamping would give other frames
    assert seen_below
