"""Smoothed time functions on the device: mg_time_function_sample_smoothed / _rows and mg_walks_time_functions_smoothed against
time_smoothing.smooth_time_row_host -- the Savitzky-Golay pass stated as a table (csrc/mg_savgol_table.h) -- applied to the row the
unsmoothed entry point gives for the same gamma.  Every comparison is of bits: csrc/mg_timewarp_device.h states the unsmoothed
sample once for both kernels, and the smoothing sums 15 products in the order the NumPy statement sums them, each rounded on its own.

The primitive is random_walk_cases' node c (65 canonical frames, two time latents).  `speed` steers the row's length T at that F:
num = int(round(t(F - 2)) * (1 / speed)), so speed = round(t(F - 2)) / (T - 2 + 0.5) gives T for the row it is sized by.  The
lengths are the window's edges (14: no smoothed form; 15, 16; 21, 22, 23: head and tail windows touch) and the 64-sample chunk's
(70, 71, 72: the tail begins in the first chunk or the second; 78, 79: the inner window's last sample; 142, 143: a third chunk)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import random_walk_cases as rc
from morphablegraphs_amd import _capi, feature_point_model as fpm, random_walks as rw, synthetic
from morphablegraphs_amd.motion_state_graph import HipPrimitiveSet
from morphablegraphs_amd.time_smoothing import WINDOW, smooth_time_row_host

pytestmark = pytest.mark.gpu

LENGTHS = [14, 15, 16, 21, 22, 23, 70, 71, 72, 78, 79, 142, 143]
LENS_SENTINEL = -12345
SENTINEL = -7777.25
LD = 16


class _World(object):
    def __init__(self):
        self.ctx = _capi.Context(0)
        c = rc.primitive_jsons()[2]
        d = synthetic.make_primitive(seed=191, n_components=8, n_frames=40, n_basis=9, n_dim=3 + 4 * rc.N_ANIMATED, n_gmm=2, name="d", dirichlet_weights=True,
                                     n_time_components=2)
        self.jsons = [c, d, rc.primitive_jsons()[0]]                   # timed (smoothed in the walks), timed, untimed
        self.prims = [_capi.Primitive(self.ctx, j) for j in self.jsons]
        self.gammas = 0.5 * np.random.default_rng(23).standard_normal((4, 2))
        self._rounded = None

    def rounded_stop(self):
        """round(t(F - 2)) of every gamma: the unsmoothed row at speed 1 has that many inner samples."""
        if self._rounded is None:
            _, lens = sample(self, self.gammas, 1.0, 4 * 65 + 8)
            assert (lens > 2).all()
            self._rounded = lens - 2
        return self._rounded

    def close(self):
        for p in self.prims:
            p.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def sample(world, G, speed, t_cap, pitch=None, smoothed=False, ld=None, col0=0):
    """One call of the sampler (pitch None: the plain form, else the _rows form) on node c over a NaN sentinel: (times (B, pitch or
    t_cap), lengths over a sentinel of their own).  The gamma columns lie at col0 of rows ld wide whose other columns hold 7.5."""
    prim, ctx = world.prims[0], world.ctx
    G = np.asarray(G)
    B, Lt = G.shape
    ld = Lt if ld is None else ld
    wide = np.full((B, ld), 7.5, dtype=G.dtype)
    wide[:, col0:col0 + Lt] = G
    p = t_cap if pitch is None else pitch
    name = "mg_time_function_sample" + ("_smoothed" if smoothed else "") + ("" if pitch is None else "_rows")
    with ctx.buffers() as bufs:
        d_g, d_t, d_l = bufs.upload(wide), bufs.upload(np.full((B, p), np.nan)), bufs.upload(np.full(B, LENS_SENTINEL, dtype=np.int32))
        args = (prim.handle, C.c_void_p(d_g.address + col0 * wide.dtype.itemsize), _capi._dtype_code(wide), B, ld, float(speed), d_t.ptr, d_l.ptr, int(t_cap))
        _capi._check(getattr(prim.lib, name)(*(args + ((None,) if pitch is None else (int(pitch), None)))))
        return ctx.download(d_t, (B, p), np.float64), ctx.download(d_l, (B,), np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def speed_for(world, T, row=0):
    return float(world.rounded_stop()[row]) / (T - 2 + 0.5)


def assert_smoothed_rows(plain_t, plain_l, got_t, got_l):
    """Every row of the smoothed call against the NumPy statement on the unsmoothed call's row; a row below the window reports its
    length and is not written."""
    assert np.array_equal(got_l, plain_l)
    for b, T in enumerate(plain_l):
        if T >= WINDOW:
            assert same_bits(got_t[b, :T], smooth_time_row_host(plain_t[b, :T])), (b, T)
            assert np.isnan(got_t[b, T:]).all()
        else:
            assert np.isnan(got_t[b]).all(), (b, T)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", LENGTHS)
def test_a_smoothed_row_is_the_table_applied_to_the_unsmoothed_row(world, T, dtype):
    G = world.gammas.astype(dtype)
    if dtype == np.float32:                                                      # (the float32 gammas have sample counts of their own)
        _, l32 = sample(world, G, 1.0, 4 * 65 + 8)
        speed = float(l32[0] - 2) / (T - 2 + 0.5)
    else:
        speed = speed_for(world, T)
    needed = np.abs(sample(world, G, speed, 2)[1])
    assert needed[0] == T
    t_cap = int(needed.max()) + 3
    plain_t, plain_l = sample(world, G, speed, t_cap)
    got_t, got_l = sample(world, G, speed, t_cap, smoothed=True)
    assert plain_l[0] == T and (plain_l > 0).all()
    assert_smoothed_rows(plain_t, plain_l, got_t, got_l)
    if T >= WINDOW:
        assert got_t[0, 0] != 0.0 and got_t[0, T - 1] != 64.0                    # smoothing moves both ends
    # the _rows form, the gammas inside wider rows; a row does not depend on its place in the batch
    pitch = t_cap + 5
    rows_t, rows_l = sample(world, G[::-1], speed, t_cap, pitch=pitch, smoothed=True, ld=7, col0=3)
    assert np.array_equal(rows_l, got_l[::-1]) and np.isnan(rows_t[:, t_cap:]).all()
    for b in range(len(G)):
        r = len(G) - 1 - b
        assert same_bits(rows_t[r, :t_cap], got_t[b]), b


@pytest.mark.parametrize("T", [15, 79])
def test_a_row_one_sample_too_long_reports_its_length_and_is_not_written(world, T):
    speed = speed_for(world, T)
    for pitch in (None, T + 4):
        times, lens = sample(world, world.gammas[:1], speed, T - 1, pitch=pitch, smoothed=True)
        assert lens[0] == -T and np.isnan(times).all()


def test_the_wrapper_returns_the_device_row_and_raises_below_the_window(world):
    graph = HipPrimitiveSet([world.jsons[0]], context=world.ctx)
    mp = graph.nodes[world.jsons[0]["name"]]
    try:
        mp.smooth_time_parameters, mp.smooth_on_device = True, True
        gamma = world.gammas[0]
        speed = speed_for(world, 22)
        want_t, want_l = sample(world, world.gammas[:1], speed, 30, smoothed=True)
        assert want_l[0] == 22 and same_bits(mp.back_project_time_function(gamma, speed), want_t[0, :22])
        with pytest.raises(ValueError, match="candidate 0: 14 samples: If mode is 'interp', window_length"):
            mp.back_project_time_function(gamma, speed_for(world, 14))
        # the batch: times smoothed on the device, the frames those of mg_back_project_frames_at at them
        S = np.concatenate((0.7 * np.random.default_rng(4).standard_normal((4, 12)), world.gammas), axis=1)
        frames, lens, times = mp.back_project_warped_batch(S, speed)
        plain_t, plain_l = sample(world, world.gammas, speed, int(lens.max()))
        assert np.array_equal(lens, plain_l) and lens[0] == 22
        for b, T in enumerate(lens):
            assert same_bits(times[b, :T], smooth_time_row_host(plain_t[b, :T])) and np.isnan(times[b, T:]).all()
        want = mp._prim.back_project_frames_at(S[:, :12], times, lens)
        assert same_bits(np.nan_to_num(frames, nan=SENTINEL), np.nan_to_num(want, nan=SENTINEL))
        with pytest.raises(ValueError, match="candidate [0-3]: 1[0-4] samples"):
            mp.back_project_warped_batch(S, speed_for(world, 14))
    finally:
        mp._prim.close()


# ---- mixed walks ------------------------------------------------------------------------------------------------------------
WALKS = [[0], [1, 2], [2, 0, 1], [0, 0, 2], [1], [2, 1, 0]]                     # node 0: timed, smoothed; 1: timed; 2: no time model
SMOOTH = [1, 0, 1]                                                              # (the flag of a node without a time model changes nothing)


def _walk_rows(world, P, speed, t_cap, smooth=None, host=False):
    node_of, n_steps = rc.tables(WALKS)
    if host:
        times, lens = np.full(node_of.shape + (t_cap,), SENTINEL), np.full(node_of.shape, 77, dtype=np.int32)
        rw.walks_time_functions_smoothed_host(world.prims, node_of, n_steps, smooth, P, speed, times, lens)
        return times, lens
    with world.ctx.buffers() as bufs:
        d_t = bufs.upload(np.full(node_of.shape + (t_cap,), SENTINEL))
        d_l = bufs.upload(np.full(node_of.shape, 77, dtype=np.int32))
        if smooth is None:
            rw.walks_time_functions_dev(world.prims, node_of, n_steps, bufs.upload(P), P.dtype, P.shape[2], speed, d_t, d_l, t_cap)
        else:
            rw.walks_time_functions_smoothed_dev(world.prims, node_of, n_steps, smooth, bufs.upload(P), P.dtype, P.shape[2], speed, d_t, d_l, t_cap)
        return world.ctx.download(d_t, node_of.shape + (t_cap,), np.float64), world.ctx.download(d_l, node_of.shape, np.int32)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("speed", [1.0, 0.6, 6.0])
def test_mixed_walks_smooth_the_flagged_nodes_and_leave_the_others_their_bits(world, speed, dtype):
    node_of, n_steps = rc.tables(WALKS)
    P = rc.latents(node_of, LD, dtype=dtype)
    t_cap = int(4 * 65 / min(speed, 1.0)) + 8
    uploads = {name: world.ctx.table_uploads(name) for name in _capi.DEVICE_TABLES if name not in ("walks_time_smoothed", "savgol")}
    plain_t, plain_l = _walk_rows(world, P, speed, t_cap)
    uploads["walks_time"] = world.ctx.table_uploads("walks_time")
    got_t, got_l = _walk_rows(world, P, speed, t_cap, SMOOTH)
    assert {name: world.ctx.table_uploads(name) for name in uploads} == uploads            # the existing tables' counts do not move
    assert world.ctx.table_uploads("savgol") == 1                                          # the hat matrix goes up once per context
    assert np.array_equal(got_l, plain_l)
    smoothed_rows = short_rows = 0
    for w in range(node_of.shape[0]):
        for i in range(node_of.shape[1]):
            T = int(plain_l[w, i])
            if i < n_steps[w] and node_of[w, i] == 0:
                assert T > 0
                if T >= WINDOW:
                    assert same_bits(got_t[w, i, :T], smooth_time_row_host(plain_t[w, i, :T])) and (got_t[w, i, T:] == SENTINEL).all(), (w, i)
                    smoothed_rows += 1
                else:
                    assert (got_t[w, i] == SENTINEL).all(), (w, i)
                    short_rows += 1
            else:
                assert same_bits(got_t[w, i], plain_t[w, i]), (w, i)
    assert (short_rows if speed == 6.0 else smoothed_rows) == 5 and short_rows * smoothed_rows == 0
    host_t, host_l = _walk_rows(world, P, speed, t_cap, SMOOTH, host=True)
    assert same_bits(host_t, got_t) and np.array_equal(host_l, got_l)
    none_t, none_l = _walk_rows(world, P, speed, t_cap, [0, 0, 0])                          # no node flagged: mg_walks_time_functions' bits
    assert same_bits(none_t, plain_t) and np.array_equal(none_l, plain_l)


def test_random_walks_take_the_smoothed_rows_to_the_frames(world):
    graph = HipPrimitiveSet(world.jsons, context=world.ctx)
    names = [j["name"] for j in world.jsons]
    try:
        walks = rw.RandomWalks(graph, [[names[k] for k in seq] for seq in WALKS], seed=9, ctx=world.ctx)
        graph.nodes[names[0]].smooth_time_parameters = True
        with pytest.raises(NotImplementedError):
            walks.time_functions()
        graph.nodes[names[0]].smooth_on_device = True
        d_t, lengths, t_cap = walks.time_functions()
        try:
            times = world.ctx.download(d_t, walks.node_of.shape + (t_cap,), np.float64)
            P = walks.parameters_host()
            want_t, want_l = _walk_rows_of(world, walks, P, t_cap)
            assert np.array_equal(lengths, want_l)
            kinds = set()
            for w in range(walks.n_walks):
                for i in range(int(walks.n_steps[w])):
                    T, name = int(lengths[w, i]), walks.nodes[walks.node_of[w, i]]
                    row = smooth_time_row_host(want_t[w, i, :T]) if name == names[0] else want_t[w, i, :T]
                    assert same_bits(times[w, i, :T], row), (w, i)
                    kinds.add(name)
            assert kinds == set(names)
            frames = walks.frames(use_time_parameters=True)
            offsets = walks.frame_offsets(lengths)
            stride, D = int(offsets[:, -1].max()), walks._prims[0].n_dim
            with world.ctx.buffers() as bufs:
                d_f = bufs.malloc(8 * walks.n_walks * stride * D)
                rw.walks_frames_at_dev(walks._prims, walks.node_of, walks.n_steps, walks.parameters, walks.dtype, walks.ld, d_t, lengths, t_cap, offsets[:, :-1], d_f,
                                       stride)
                block = world.ctx.download(d_f, (walks.n_walks, stride, D), np.float64)
            for w in range(walks.n_walks):
                assert same_bits(frames[w], block[w, :int(offsets[w, -1])]), w
        finally:
            d_t.free()
        with pytest.raises(ValueError, match=r"walk \d, step \d: \d+ samples: If mode is 'interp', window_length"):
            walks.frames(use_time_parameters=True, speed=8.0)
        walks.close()
    finally:
        for mp in graph.nodes.values():
            mp._prim.close()


def _walk_rows_of(world, walks, P, t_cap):
    """mg_walks_time_functions (unsmoothed) for a RandomWalks population's own tables."""
    with world.ctx.buffers() as bufs:
        d_t, d_l = bufs.upload(np.full(walks.node_of.shape + (t_cap,), SENTINEL)), bufs.upload(np.zeros(walks.node_of.shape, dtype=np.int32))
        rw.walks_time_functions_dev(walks._prims, walks.node_of, walks.n_steps, bufs.upload(P), P.dtype, P.shape[2], 1.0, d_t, d_l, t_cap)
        return world.ctx.download(d_t, walks.node_of.shape + (t_cap,), np.float64), world.ctx.download(d_l, walks.node_of.shape, np.int32)


# ---- feature points -----------------------------------------------------------------------------------------------------------
POSITION_BOUND = 4e-12          # per position, times the scale: tests/test_gpu_feature_points_warped.py's, for what goes through FK
JOINTS = ["Spine", "Hips"]


def _fp_rows(world, n, seed):
    """n full rows of node c: 12 spatial latents, then its two time latents"""
    rng = np.random.default_rng(seed)
    return np.concatenate((0.7 * rng.standard_normal((n, 12)), 0.5 * rng.standard_normal((n, 2))), axis=1)


@pytest.fixture(scope="module")
def fp_case(world):
    """Node c's rows over more than one tile, the unsmoothed time rows (mg_time_function_sample) and their NumPy-smoothed form."""
    S = _fp_rows(world, _capi.MG_FEATURE_POINTS_TILE + 3, 61)
    plain_t, lens = world.prims[0].time_function_sample(np.ascontiguousarray(S[:, 12:]))
    assert lens.min() >= WINDOW and len(set(lens.tolist())) > 1
    return S, lens, [smooth_time_row_host(plain_t[b, :T]) for b, T in enumerate(lens)]


def _fp_item(prim, S, sk, frame_idx):
    return {"prim": prim, "S": S, "skeleton": sk, "joints": JOINTS, "frame_idx": frame_idx}


@pytest.mark.parametrize("which", ["0", "6", "7", "Tmin-8", "Tmin-7", "Tmin-1", "Tmin", "Tmax-8", "Tmax-7", "Tmax-1", "Tmax"])
def test_feature_points_take_all_three_times_from_the_smoothed_row(world, fp_case, which):
    S, lens, smoothed = fp_case
    prim, sk, n = world.prims[0], rc.skeleton(), len(S)
    frame_idx = int(eval(which, {"Tmin": int(lens.min()), "Tmax": int(lens.max())}))
    got, plain = _capi.feature_points_warped([_fp_item(prim, S, sk, frame_idx)] * 2, smooth=[1, 0])
    want_plain = _capi.feature_points_warped([_fp_item(prim, S, sk, frame_idx)])[0]
    for key in _capi.WARPED_FEATURE_POINT_OUTPUTS:                                # smooth = 0: mg_feature_points_warped's bits
        assert same_bits(plain[key], want_plain[key]) if plain[key].dtype == np.float64 else np.array_equal(plain[key], want_plain[key]), key
    assert np.array_equal(got["n_frames"], lens)
    has = lens > frame_idx
    assert (which == "Tmax") == (not has.any()) and (which != "Tmin" or (has.any() and not has.all()))
    want_mid = np.array([smoothed[b][frame_idx] if has[b] else np.nan for b in range(n)])
    assert same_bits(got["time_mid"], want_mid)
    # the frames at the three smoothed times through mg_back_project_frames_at: the first one below 0 or above, the last one off F - 1
    times = np.array([[smoothed[b][0], want_mid[b] if has[b] else smoothed[b][0], smoothed[b][-1]] for b in range(n)])
    assert (times[:, 0] != 0.0).all() and (times[:, 2] != 64.0).all() and (times[:, 0] < 0.0).any()
    frames = prim.back_project_frames_at(np.ascontiguousarray(S[:, :12]), times, None)
    assert same_bits(got["start_root"], frames[:, 0, :3]) and same_bits(got["root_end"], frames[:, 2][:, [0, 2]])
    scale = max(1.0, float(np.abs(frames[:, :, :3]).max()))
    for b in range(n):
        heading, length = fpm.heading_host(frames[b, 2])
        assert np.abs(got["heading_end"][b] - heading).max() <= POSITION_BOUND and abs(got["heading_len"][b] - length) <= POSITION_BOUND
    assert np.isnan(got["points"][~has]).all() and np.isfinite(got["points"][has]).all()      # frame_idx = T: NaN in points and time_mid only
    if has.any():
        pos = world.ctx.joint_positions(sk, JOINTS, np.ascontiguousarray(frames[has, 1]))
        want = (pos - frames[has, 0, :3][:, None, :]).reshape(int(has.sum()), -1)
        assert np.abs(got["points"][has] - want).max() <= POSITION_BOUND * scale
    # the existing kernel at its own (unsmoothed) times gives other features: the smoothing is not a no-op
    assert not same_bits(got["start_root"], plain["start_root"])


def test_a_candidate_below_the_window_is_nan_but_for_its_length(world):
    data = synthetic.make_primitive(seed=77, n_components=5, n_frames=12, n_basis=7, n_dim=3 + 4 * rc.N_ANIMATED, n_gmm=2, name="short", n_time_components=2)
    prim, sk = _capi.Primitive(world.ctx, data), rc.skeleton()
    try:
        rng = np.random.default_rng(5)
        S = np.concatenate((0.7 * rng.standard_normal((5, 5)), 0.3 * rng.standard_normal((5, 2))), axis=1)
        uploads = {name: world.ctx.table_uploads(name) for name in _capi.DEVICE_TABLES if name not in ("feature_points_smoothed", "savgol")}
        before = world.ctx.table_uploads("feature_points_smoothed")
        got, plain = _capi.feature_points_warped([_fp_item(prim, S, sk, 3)] * 2, smooth=[1, 0])
        assert {name: world.ctx.table_uploads(name) for name in uploads} == uploads and world.ctx.table_uploads("feature_points_smoothed") == before + 1
        assert np.array_equal(got["n_frames"], plain["n_frames"]) and (got["n_frames"] > 3).all() and (got["n_frames"] < WINDOW).all()
        for key in _capi.FEATURE_POINT_OUTPUTS + ("time_mid",):
            assert np.isnan(got[key]).all() and np.isfinite(plain[key]).all(), key
    finally:
        prim.close()


def test_the_feature_point_model_routes_a_smoothed_primitive_to_the_smoothed_call(world, fp_case):
    S, lens, smoothed = fp_case
    graph = HipPrimitiveSet([world.jsons[0]], context=world.ctx)
    mp = graph.nodes[world.jsons[0]["name"]]
    try:
        mp.smooth_time_parameters = True
        with pytest.raises(NotImplementedError, match="Savitzky-Golay"):
            fpm.HipFeaturePointModel(mp, rc.skeleton(), latents=S, time_warped=True).create_root_pos_ori(len(S))
        mp.smooth_on_device = True
        model = fpm.HipFeaturePointModel(mp, rc.skeleton(), latents=S, time_warped=True)
        model.create_root_pos_ori(len(S))
        want = _capi.feature_points_warped([_fp_item(mp._prim, S, rc.skeleton(), 0)], smooth=[1])[0]
        assert same_bits(np.array(model.root_pos), want["root_end"]) and same_bits(np.array(model.root_orientation), want["heading_end"])
    finally:
        mp._prim.close()
