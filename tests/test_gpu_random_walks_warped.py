"""Time-warped random walks on the device: mg_walks_time_functions, mg_walks_frames_at and RandomWalks.frames(use_time_parameters=True)
(tests/random_walk_cases.py: node c has two time latents, a and b have none; 31 / 33 / 65 canonical frames).

Both contracts are exact.  A time row of a node with a time model has the bits of mg_time_function_sample for that primitive and
gamma, one of a node without has numpy.linspace's; every walk of a mixed population has the bits mg_walk_frames gives for that walk
alone at the same times.  Only the comparison with the NumPy frames carries a tolerance, tests/test_graph_walk_host.py's
WALK_TOLERANCE.
"""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import random_walk_cases as rc
import timewarp_cases as tc
from morphablegraphs_amd import _capi, feature_point_model as fpm, graph_walk as gw, random_walks as rw
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraph, HipPrimitiveSet
from test_graph_walk_host import WALK_TOLERANCE, root_scale

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25
D = 3 + 4 * rc.N_ANIMATED
LD = 16                                     # wider than the widest mixture (14)
WIDTH = [L for L, _, _, _, _ in rc.SHAPES]
FRAMES = [F for _, F, _, _, _ in rc.SHAPES]
TIME_WIDTH = [Lt for _, _, _, _, Lt in rc.SHAPES]
SPEEDS = (1.0, 0.37, 1.6)
INVALID, UNSUPPORTED = _capi.MG_ERR_INVALID_ARGUMENT, _capi.MG_ERR_UNSUPPORTED


class _World(object):
    def __init__(self):
        self.ctx = _capi.Context(0)
        self.jsons = rc.primitive_jsons()
        self.prims = [_capi.Primitive(self.ctx, d) for d in self.jsons]
        self.sk = rc.skeleton()
        self.alignments = {name: (al, sk) for name, al, sk in rc.alignments(self.sk, self.jsons)}

    def close(self):
        for p in self.prims:
            p.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _rule_cap(speed):
    """graph_walk._sample_times' first t_cap for the three nodes."""
    return max(int(4 * FRAMES[2] / min(speed, 1.0)) + 8, int(FRAMES[1] * (1.0 / speed)))


def _time_rows(world, walks, P, speed, t_cap, prims=None):
    """mg_walks_time_functions into sentinel-filled buffers: (times (n, s_max, t_cap), lengths (n, s_max), 77 where not written)."""
    node_of, n_steps = rc.tables(walks)
    with world.ctx.buffers() as bufs:
        d_t = bufs.upload(np.full(node_of.shape + (t_cap,), SENTINEL))
        d_l = bufs.upload(np.full(node_of.shape, 77, dtype=np.int32))
        rw.walks_time_functions_dev(prims or world.prims, node_of, n_steps, bufs.upload(P), P.dtype, P.shape[2], speed, d_t, d_l, t_cap)
        return world.ctx.download(d_t, node_of.shape + (t_cap,), np.float64), world.ctx.download(d_l, node_of.shape, np.int32)


def _assert_time_rows(world, walks, P, speed, t_cap, times, lengths, skip=()):
    """Every row against mg_time_function_sample (node c, its gamma from the step's row) or numpy.linspace (a, b); what a walk
    does not have is untouched, its length 0."""
    node_of, n_steps = rc.tables(walks)
    timed = [(w, i) for w, seq in enumerate(walks) for i, k in enumerate(seq) if TIME_WIDTH[k] > 0]
    if timed:
        G = np.stack([P[w, i, WIDTH[2]:WIDTH[2] + TIME_WIDTH[2]] for w, i in timed])
        want_t, want_l = world.prims[2].time_function_sample(G, speed, t_cap=t_cap)
    for w in range(node_of.shape[0]):
        for i in range(node_of.shape[1]):
            if (w, i) in skip:
                continue
            if i >= n_steps[w]:
                assert lengths[w, i] == 0 and (times[w, i] == SENTINEL).all(), (w, i)
            elif (w, i) in timed:
                r = timed.index((w, i))
                T = int(want_l[r])
                assert lengths[w, i] == T, (w, i)
                if T > 0:
                    assert _same_bits(times[w, i, :T], want_t[r, :T]) and (times[w, i, T:] == SENTINEL).all(), (w, i)
                else:
                    assert (times[w, i] == SENTINEL).all(), (w, i)
            else:
                F = FRAMES[node_of[w, i]]
                want = np.linspace(0, F, int(F * (1.0 / speed)))
                assert lengths[w, i] == len(want) and _same_bits(times[w, i, :len(want)], want) and (times[w, i, len(want):] == SENTINEL).all(), (w, i)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("speed", SPEEDS)
def test_every_time_row_has_the_bits_of_its_own_statement(world, speed, dtype):
    walks = rc.CONTRACT_WALKS
    node_of, n_steps = rc.tables(walks)
    P = rc.latents(node_of, LD, dtype=dtype)
    t_cap = _rule_cap(speed)
    times, lengths = _time_rows(world, walks, P, speed, t_cap)
    _assert_time_rows(world, walks, P, speed, t_cap, times, lengths)
    assert lengths.max() <= t_cap and len({int(lengths[w, i]) for w, seq in enumerate(walks) for i, k in enumerate(seq) if k == 2}) > 1
    host_t, host_l = np.full(times.shape, SENTINEL), np.full(lengths.shape, 77, dtype=np.int32)
    rw.walks_time_functions_host(world.prims, node_of, n_steps, P, speed, host_t, host_l)
    assert _same_bits(host_t, times) and np.array_equal(host_l, lengths)


def test_a_row_that_does_not_fit_reports_its_length_and_is_not_written(world):
    walks = rc.CONTRACT_WALKS
    node_of, _ = rc.tables(walks)
    P = rc.latents(node_of, LD)
    full_t, full_l = _time_rows(world, walks, P, 1.0, _rule_cap(1.0))
    longest = int(full_l.max())
    t_cap = longest - 1
    times, lengths = _time_rows(world, walks, P, 1.0, t_cap)
    too_long = full_l == longest
    assert too_long.any() and not too_long.all()
    for w in range(node_of.shape[0]):
        for i in range(node_of.shape[1]):
            if too_long[w, i]:
                assert lengths[w, i] == -longest and (times[w, i] == SENTINEL).all(), (w, i)
            else:
                assert lengths[w, i] == full_l[w, i] and _same_bits(times[w, i], full_t[w, i, :t_cap]), (w, i)


def _primitive_set(world, jsons):
    return HipPrimitiveSet(jsons, context=world.ctx)


def _close_set(graph):
    for mp in graph.nodes.values():
        mp._prim.close()


def test_random_walks_time_functions_lays_the_table_out_again(world):
    """timewarp_cases' long_row needs about 281 samples of its 64 canonical frames, more than the 4 F + 8 the first table has."""
    long_json, _ = tc.model_of("long_row")
    graph = _primitive_set(world, [world.jsons[0], long_json])
    try:
        walks = rw.RandomWalks(graph, [["a", long_json["name"]], [long_json["name"]]], seed=3, ctx=world.ctx)
        d_t, lengths, t_cap = walks.time_functions()
        try:
            first_cap = 4 * 64 + 8
            assert lengths[0, 1] > first_cap and lengths[1, 0] > first_cap and t_cap >= lengths.max() and lengths[1, 1] == 0
            times = world.ctx.download(d_t, lengths.shape + (t_cap,), np.float64)
        finally:
            d_t.free()
        P = walks.parameters_host()
        want_t, want_l = graph.nodes[long_json["name"]]._prim.time_function_sample(np.stack([P[0, 1, 3:4], P[1, 0, 3:4]]), 1.0)
        for (w, i), r in (((0, 1), 0), ((1, 0), 1)):
            assert lengths[w, i] == want_l[r] and _same_bits(times[w, i, :want_l[r]], want_t[r, :want_l[r]])
        assert _same_bits(times[0, 0, :31], np.linspace(0, 31, 31)) and lengths[0, 0] == 31
        frames = walks.frames(use_time_parameters=True)
        assert [len(f) for f in frames] == [int(lengths[0].sum()), int(lengths[1].sum())] and all(np.isfinite(f).all() for f in frames)
        walks.close()
    finally:
        _close_set(graph)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_time_function_that_is_not_finite_has_length_zero(world, dtype):
    walks = rc.CONTRACT_WALKS
    node_of, n_steps = rc.tables(walks)
    P = rc.latents(node_of, LD, dtype=dtype)
    t_cap = _rule_cap(1.0)
    before_t, before_l = _time_rows(world, walks, P, 1.0, t_cap)
    wild = (3, 0)                                                      # a step of node c
    assert walks[wild[0]][wild[1]] == 2
    P[wild[0], wild[1], WIDTH[2]:WIDTH[2] + 2] = 1.0e6                 # exp() overflows: plain inf / NaN arithmetic
    with np.errstate(all="ignore"):
        assert not np.isfinite(fpm.canonical_time_function_host(fpm._time_model_host(world.jsons[2]), FRAMES[2], np.array([1.0e6, 1.0e6]))[-2])
    times, lengths = _time_rows(world, walks, P, 1.0, t_cap)
    assert lengths[wild] == 0 and (times[wild] == SENTINEL).all()
    keep = np.ones(node_of.shape, dtype=bool)
    keep[wild] = False
    assert np.array_equal(lengths[keep], before_l[keep]) and _same_bits(times[keep], before_t[keep])


def test_random_walks_raises_on_a_time_function_that_is_not_finite(world):
    graph = _primitive_set(world, world.jsons)
    try:
        walks = rw.RandomWalks(graph, [["a", "c"], ["b"]], seed=5, ctx=world.ctx)
        P = walks.parameters_host()
        P[0, 1, WIDTH[2]:WIDTH[2] + 2] = 1.0e6
        _capi._check(world.ctx.lib.mg_memcpy_h2d(world.ctx.handle, walks.parameters.ptr, P.ctypes.data_as(C.c_void_p), P.nbytes))
        with pytest.raises(ValueError, match="a time function is not finite"):
            walks.time_functions()
        with pytest.raises(ValueError, match="a time function is not finite"):
            walks.frames(use_time_parameters=True)
        walks.close()
    finally:
        _close_set(graph)


# ---- the frames ----------------------------------------------------------------------------------------------------------
def _back_to_back(lengths, n_steps):
    offsets = np.zeros(lengths.shape, dtype=np.int64)
    for w, ns in enumerate(n_steps):
        offsets[w, 1:ns] = np.cumsum(lengths[w, :ns - 1])
    return offsets


def _stride(lengths, offsets, n_steps):
    return int(max(offsets[w, i] + lengths[w, i] for w, ns in enumerate(n_steps) for i in range(ns)))


def _solo_at(world, seq, rows, dtype, times, lengths, offsets, stride, alignment, skeleton):
    """mg_walk_frames for one walk alone at its time rows, into sentinel-filled rows: (frames (stride, D), transforms (n_steps, 4))."""
    m = len(seq)
    S = np.concatenate([rows[i, :WIDTH[k]] for i, k in enumerate(seq)])[None, :].astype(dtype)
    offs = np.concatenate(([0], np.cumsum([WIDTH[k] for k in seq])[:-1]))
    with world.ctx.buffers() as bufs:
        d_f, d_x = bufs.upload(np.full((stride, D), SENTINEL)), bufs.malloc(8 * m * 4)
        gw.walk_frames_dev([world.prims[k] for k in seq], offs, bufs.upload(S), dtype, 1, S.shape[1], d_f, stride, bufs.upload(np.ascontiguousarray(times[:m])),
                           lengths[None, :m], times.shape[1], offsets[None, :m], alignment, skeleton, d_x)
        return world.ctx.download(d_f, (stride, D), np.float64), world.ctx.download(d_x, (m, 4), np.float64)


def _mixed_at(world, walks, P, times, lengths, offsets, stride, alignment=None, skeleton=None):
    """mg_walks_frames_at into buffers filled with the sentinel: (frames (n, stride, D), transforms (n, s_max, 4))."""
    node_of, n_steps = rc.tables(walks)
    with world.ctx.buffers() as bufs:
        d_f = bufs.upload(np.full((len(walks), stride, D), SENTINEL))
        d_x = bufs.upload(np.full(node_of.shape + (4,), SENTINEL))
        rw.walks_frames_at_dev(world.prims, node_of, n_steps, bufs.upload(P), P.dtype, P.shape[2], bufs.upload(times), lengths, times.shape[2], offsets, d_f, stride,
                               alignment, skeleton, d_x)
        return world.ctx.download(d_f, (len(walks), stride, D), np.float64), world.ctx.download(d_x, node_of.shape + (4,), np.float64)


def _assert_contract(world, walks, P, times, lengths, offsets, frames, transforms, alignment, skeleton, which=None):
    """Walk w's rows, sentinel rows included, and its transforms are the solo call's; what it does not have keeps the sentinel."""
    stride = frames.shape[1]
    for w in (range(len(walks)) if which is None else which):
        seq = walks[w]
        fr, tr = _solo_at(world, seq, P[w], P.dtype, times[w], lengths[w], offsets[w], stride, alignment, skeleton)
        assert _same_bits(frames[w], fr), w
        assert _same_bits(transforms[w, :len(seq)], tr) and (transforms[w, len(seq):] == SENTINEL).all(), w
        owned = np.zeros(stride, dtype=bool)
        for i in range(len(seq)):
            owned[offsets[w, i]:offsets[w, i] + lengths[w, i]] = True
        assert (frames[w, ~owned] == SENTINEL).all() and (frames[w, owned] != SENTINEL).all(), w


def _contract_population(world, dtype, speed=1.6):
    walks = rc.CONTRACT_WALKS
    node_of, n_steps = rc.tables(walks)
    P = rc.latents(node_of, LD, dtype=dtype)
    t_cap = _rule_cap(speed)
    times, lengths = _time_rows(world, walks, P, speed, t_cap)
    times[times == SENTINEL], lengths = 0.0, np.where(node_of >= 0, lengths, 0).astype(np.int32)
    return walks, node_of, n_steps, P, times, lengths


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["none", "previous", "start_pose", "previous_spine"])
def test_every_walk_of_a_warped_population_is_its_solo_call(world, kind, dtype):
    alignment, skeleton = world.alignments[kind]
    walks, node_of, n_steps, P, times, lengths = _contract_population(world, dtype)
    offsets = _back_to_back(lengths, n_steps)
    stride = _stride(lengths, offsets, n_steps)
    frames, transforms = _mixed_at(world, walks, P, times, lengths, offsets, stride, alignment, skeleton)
    _assert_contract(world, walks, P, times, lengths, offsets, frames, transforms, alignment, skeleton)
    assert np.isfinite(frames[frames != SENTINEL]).all()
    host_f, host_x = np.full(frames.shape, SENTINEL), np.full(transforms.shape, SENTINEL)
    rw.walks_frames_at_host(world.prims, node_of, n_steps, P, times, lengths, offsets, host_f, alignment, skeleton, host_x)
    assert _same_bits(host_f, frames) and _same_bits(host_x, transforms)


@pytest.mark.parametrize("kind", ["none", "previous_spine"])
def test_the_frames_against_the_numpy_statement(world, kind):
    alignment, skeleton = world.alignments[kind]
    walks, node_of, n_steps, P, times, lengths = _contract_population(world, np.float64, speed=0.37)
    offsets = _back_to_back(lengths, n_steps)
    frames, transforms = _mixed_at(world, walks, P, times, lengths, offsets, _stride(lengths, offsets, n_steps), alignment, skeleton)
    rows = [[times[w, i, :lengths[w, i]] for i in range(len(seq))] for w, seq in enumerate(walks)]
    ref, _, ref_x = rw.assemble_walks_mixed_host(world.jsons, node_of, n_steps, P, alignment, skeleton, times=rows, speed=0.37)
    for w, seq in enumerate(walks):
        T = int(lengths[w].sum())
        worst = float(np.max(np.abs(frames[w, :T] - ref[w]))) / root_scale(ref[w])
        worst_x = float(np.max(np.abs(transforms[w, :len(seq)] - ref_x[w, :len(seq)]))) / root_scale(ref[w])
        print("walk %d: frames %.3g, transforms %.3g of the root scale %.4g (bound %.3g)" % (w, worst, worst_x, root_scale(ref[w]), WALK_TOLERANCE))
        assert ref[w].shape == (T, D) and worst <= WALK_TOLERANCE and worst_x <= WALK_TOLERANCE


def test_tile_edges_with_hand_made_time_rows(world):
    """Lengths 1, 2, 31, 32, 33, 64, 65 and 97 over eight steps of three walks; a row shuffled inside its tiles (the control-point
    window spans the whole spline), a row that ends below F - 1 on a step another step follows (the exit pose follows the row),
    offsets with gaps."""
    walks = [[0, 1, 2], [2, 0], [1, 2, 1]]
    node_of, n_steps = rc.tables(walks)
    want = {(0, 0): 32, (0, 1): 1, (0, 2): 97, (1, 0): 64, (1, 1): 2, (2, 0): 33, (2, 1): 65, (2, 2): 31}
    t_cap = 97
    times, lengths = np.zeros(node_of.shape + (t_cap,)), np.zeros(node_of.shape, dtype=np.int32)
    rng = np.random.default_rng(41)
    for (w, i), T in want.items():
        F = FRAMES[walks[w][i]]
        lengths[w, i] = T
        times[w, i, :T] = np.linspace(0.0, F - 1.0, T) if T > 1 else 0.4 * (F - 1.0)
    times[0, 0, :32] *= 0.6                                            # ends at 0.6 (F - 1); step (0, 1) is aligned to that pose
    times[1, 0, :64] = rng.permutation(times[1, 0, :64])              # not monotone inside either tile
    assert times[0, 0, 31] < 0.7 * (FRAMES[0] - 1) and (np.diff(times[1, 0, :32]) < 0).any() and np.ptp(times[1, 0, :32]) > 0.8 * (FRAMES[2] - 1)
    assert sorted(want.values()) == [1, 2, 31, 32, 33, 64, 65, 97]
    offsets = np.zeros(node_of.shape, dtype=np.int64)
    for w, seq in enumerate(walks):
        row = 2
        for i in (reversed(range(len(seq))) if w == 1 else range(len(seq))):
            offsets[w, i] = row
            row += lengths[w, i] + 2 + i
    stride = _stride(lengths, offsets, n_steps) + 3
    P = rc.latents(node_of, LD, seed=12)
    alignment, skeleton = world.alignments["previous"]
    frames, transforms = _mixed_at(world, walks, P, times, lengths, offsets, stride, alignment, skeleton)
    _assert_contract(world, walks, P, times, lengths, offsets, frames, transforms, alignment, skeleton)
    assert (frames[:, :2] == SENTINEL).all() and (frames[:, -3:] == SENTINEL).all()
    # the exit pose follows the row: with the canonical end in its place step (0, 1) lands elsewhere
    other = times.copy()
    other[0, 0, 31] = FRAMES[0] - 1.0
    _, moved = _mixed_at(world, walks, P, other, lengths, offsets, stride, alignment, skeleton)
    assert not np.array_equal(moved[0, 1], transforms[0, 1]) and _same_bits(moved[0, 0], transforms[0, 0])


def test_a_warped_walk_does_not_depend_on_its_population(world):
    seq = rc.CONTRACT_WALKS[3]
    rows = rc.latents(np.zeros((1, 4), dtype=np.int32), LD, seed=8)[0]
    own_len, t_cap = [40, 33, 20, 31], 70
    own_times = np.zeros((4, t_cap))
    for i, (k, T) in enumerate(zip(seq, own_len)):
        own_times[i, :T] = np.linspace(0.0, FRAMES[k] - 1.0, T)
    alignment, skeleton = world.alignments["start_pose"]
    got = []
    for n, at, extra in ((1, 0, None), (6, 0, None), (6, 5, [0, 1, 2, 1, 0, 2]), (65, 64, None)):
        walks = [rc.CONTRACT_WALKS[(w + 1) % 6] for w in range(n)]
        if extra is not None:
            walks[1] = extra                                           # another s_max: six steps
        walks[at] = seq
        node_of, n_steps = rc.tables(walks)
        P = rc.latents(node_of, LD, seed=20 + n)
        times, lengths = np.zeros(node_of.shape + (t_cap,)), np.zeros(node_of.shape, dtype=np.int32)
        for w, s in enumerate(walks):
            for i, k in enumerate(s):
                lengths[w, i] = FRAMES[k]
                times[w, i, :FRAMES[k]] = np.linspace(0.0, FRAMES[k] - 1.0, FRAMES[k])
        P[at, :4], times[at, :4], lengths[at, :4] = rows, own_times, own_len
        offsets = _back_to_back(lengths, n_steps)
        frames, transforms = _mixed_at(world, walks, P, times, lengths, offsets, _stride(lengths, offsets, n_steps), alignment, skeleton)
        got.append((frames[at, :sum(own_len)], transforms[at, :4]))
    for fr, tr in got[1:]:
        assert _same_bits(fr, got[0][0]) and _same_bits(tr, got[0][1])
    lengths = np.array(own_len, dtype=np.int32)
    fr, tr = _solo_at(world, seq, rows, np.float64, own_times, lengths, _back_to_back(lengths[None], [4])[0], sum(own_len), alignment, skeleton)
    assert _same_bits(got[0][0], fr) and _same_bits(got[0][1], tr)


def test_past_65536_walks_the_prefix_search_finds_every_walk(world):
    """65 537 one-step walks of 1 .. 3 frames: one tile each, the tile prefix as long as the population."""
    n, t_cap = 65537, 3
    walks = [[w % 2] for w in range(n)]
    node_of, n_steps = rc.tables(walks)
    P = rc.latents(node_of, 12, seed=9)
    rng = np.random.default_rng(10)
    lengths = (1 + np.arange(n) % 3).astype(np.int32)[:, None]
    times = np.sort(rng.uniform(0.0, 30.0, size=(n, 1, t_cap)), axis=2)
    offsets = np.zeros((n, 1), dtype=np.int64)
    with world.ctx.buffers() as bufs:
        d_f = bufs.upload(np.full((n, t_cap, D), SENTINEL))
        rw.walks_frames_at_dev(world.prims, node_of, n_steps, bufs.upload(P), P.dtype, 12, bufs.upload(times), lengths, t_cap, offsets, d_f, t_cap)
        for w in (0, 65535, 65536):
            got = world.ctx.download(d_f.address + 8 * w * t_cap * D, (t_cap, D), np.float64)
            fr, _ = _solo_at(world, walks[w], P[w], np.float64, times[w], lengths[w], offsets[w], t_cap, None, None)
            assert _same_bits(got, fr) and (got[lengths[w, 0]:] == SENTINEL).all() and (got[:lengths[w, 0]] != SENTINEL).all(), w


@pytest.mark.parametrize("speed", SPEEDS)
def test_round_trip_through_the_graph(world, speed):
    graph = HipMotionStateGraph(context=world.ctx).build_from_graph_data(rc.graph_data(world.jsons))
    try:
        walks = graph.generate_random_walks("walk", 3, 6, seed=11, rng=random.Random(2))
        params = walks.parameters_host()
        frames, transforms = walks.frames(with_transforms=True, use_time_parameters=True, speed=speed)
        assert len({len(f) for f in frames}) > 1 and any(("walk", "c") in keys for keys in walks.node_keys)
        for w, keys in enumerate(walks.node_keys):
            prims = [walks._prims[k] for k in walks.node_of[w, :len(keys)]]
            S = np.concatenate([params[w, i, :p.n_components] for i, p in enumerate(prims)])[None, :]
            G = np.concatenate([params[w, i, p.n_components:p.n_gmm_dims] for i, p in enumerate(prims)] + [np.zeros(1)])[None, :]
            ref, offs, ref_x = gw.assemble_walks(graph, [tuple(k) for k in keys], S, time_parameters=G, speed=speed, with_transforms=True)
            assert _same_bits(frames[w], ref[0, :int(offs[0, -1])]) and _same_bits(transforms[w, :len(keys)], ref_x[0]), w
            assert np.isnan(transforms[w, len(keys):]).all()
        gwalks = walks.to_graph_walks(use_time_parameters=True)
        assert all(g.use_time_parameters for g in gwalks) and not walks.to_graph_walks()[0].use_time_parameters
        walks.close()
    finally:
        graph.close()


def test_frames_without_the_flag_are_mg_walks_frames(world):
    graph = _primitive_set(world, world.jsons)
    try:
        walks = rw.RandomWalks(graph, [["a", "c", "b"], ["c"], ["b", "b"]], seed=7, ctx=world.ctx)
        frames = walks.frames()
        offsets = walks.frame_offsets()
        canonical = np.array([FRAMES[rc.NAMES.index(name)] for name in walks.nodes])        # (the nodes in order of first occurrence)
        assert np.array_equal(offsets[:, 1:], np.cumsum(np.where(walks.node_of >= 0, canonical[np.maximum(walks.node_of, 0)], 0), axis=1))
        stride = int(offsets[:, -1].max())
        with world.ctx.buffers() as bufs:
            d_f = bufs.malloc(8 * 3 * stride * D)
            rw.walks_frames_dev(walks._prims, walks.node_of, walks.n_steps, walks.parameters, walks.dtype, walks.ld, d_f, stride)
            block = world.ctx.download(d_f, (3, stride, D), np.float64)
        for w in range(3):
            assert _same_bits(frames[w], block[w, :int(offsets[w, -1])]), w
        # the new entry points keep tables of their own
        counts = [world.ctx.table_uploads(name) for name in ("walks_mixed", "walks_sample")]
        warped = walks.frames(use_time_parameters=True, speed=1.6)
        assert [world.ctx.table_uploads(name) for name in ("walks_mixed", "walks_sample")] == counts
        assert [len(f) for f in warped] != [len(f) for f in frames]
        lengths = np.array([[31, 40, 33], [40, 0, 0], [33, 33, 0]])
        assert np.array_equal(walks.frame_offsets(lengths)[:, 1:], np.cumsum(lengths, axis=1))
        with pytest.raises(NotImplementedError):
            walks.frames(speed=1.6)
        graph.nodes["c"].smooth_time_parameters = True
        with pytest.raises(NotImplementedError):
            walks.time_functions()
        with pytest.raises(NotImplementedError):
            walks.frames(use_time_parameters=True)
        walks.close()
    finally:
        _close_set(graph)


def test_misuse_is_refused_before_anything_is_written(world):
    walks = rc.CONTRACT_WALKS
    _, node_of, n_steps, P, times, lengths = _contract_population(world, np.float64)
    n, s_max = node_of.shape
    t_cap = times.shape[2]
    offsets = _back_to_back(lengths, n_steps)
    stride = _stride(lengths, offsets, n_steps)
    long_json = tc.time_model(2049, 1, 20, 0.05, 77, name="too_long")
    too_long = _capi.Primitive(world.ctx, long_json)
    spine, _ = world.alignments["previous_spine"]
    bad_node, no_steps = node_of.copy(), n_steps.copy()
    bad_node[2, 1], no_steps[0] = 3, 0
    zero_len, long_len, absent_len = lengths.copy(), lengths.copy(), lengths.copy()
    zero_len[2, 1], long_len[4, 3], absent_len[0, 1] = 0, t_cap + 1, -5          # (absent: a step the walk does not have is not read)
    overlap = offsets.copy()
    overlap[:, 1:] = 5
    TA = dict(prims=world.prims, node_of=node_of, n_steps=n_steps, ld=LD, speed=1.0)
    time_cases = [("speed 0", dict(speed=0.0), INVALID), ("negative speed", dict(speed=-1.0), INVALID), ("infinite speed", dict(speed=np.inf), INVALID),
                  ("speed NaN", dict(speed=np.nan), INVALID), ("an untimed node without a sample", dict(speed=40.0), INVALID),
                  ("ld below n_components + n_time_components", dict(ld=13), INVALID), ("node index past the table", dict(node_of=bad_node), INVALID),
                  ("a walk without steps", dict(n_steps=no_steps), INVALID),
                  ("a timed node of more than MG_TW_MAX_F frames", dict(prims=[world.prims[0], world.prims[1], too_long]), UNSUPPORTED)]
    FA = dict(prims=world.prims, node_of=node_of, n_steps=n_steps, ld=LD, times=True, lengths=lengths, offsets=offsets, stride=stride, alignment=None)
    frame_cases = [("a length below 1", dict(lengths=zero_len), INVALID), ("a length above t_cap", dict(lengths=long_len), INVALID),
                   ("steps overlap", dict(offsets=overlap), INVALID), ("a walk passes walk_stride", dict(stride=stride - 1), INVALID),
                   ("a non-root aligning joint without a skeleton", dict(alignment=spine), INVALID), ("no times", dict(times=False), INVALID),
                   ("no lengths", dict(lengths=None), INVALID), ("no frame offsets", dict(offsets=None), INVALID),
                   ("ld below a node's latents", dict(ld=8), INVALID), ("node index past the table", dict(node_of=bad_node), INVALID)]
    try:
        with world.ctx.buffers() as bufs:
            d_P, d_times = bufs.upload(P), bufs.upload(times)
            d_f, d_x = bufs.upload(np.full((n, stride, D), SENTINEL)), bufs.upload(np.full((n, s_max, 4), SENTINEL))
            d_t, d_l = bufs.upload(np.full((n, s_max, t_cap), SENTINEL)), bufs.upload(np.full((n, s_max), 77, dtype=np.int32))

            def intact():
                world.ctx.synchronize()
                return (world.ctx.download(d_f, (n, stride, D), np.float64) == SENTINEL).all() and (world.ctx.download(d_x, (n, s_max, 4), np.float64) == SENTINEL).all() \
                    and (world.ctx.download(d_t, (n, s_max, t_cap), np.float64) == SENTINEL).all() and (world.ctx.download(d_l, (n, s_max), np.int32) == 77).all()

            for what, change, status in time_cases:
                a = dict(TA, **change)
                with pytest.raises(_capi.MGError) as e:
                    rw.walks_time_functions_dev(a["prims"], a["node_of"], a["n_steps"], d_P, np.float64, a["ld"], a["speed"], d_t, d_l, t_cap)
                assert e.value.status == status, what
                assert intact(), what
            for what, change, status in frame_cases:
                a = dict(FA, **change)
                with pytest.raises(_capi.MGError) as e:
                    rw.walks_frames_at_dev(a["prims"], a["node_of"], a["n_steps"], d_P, np.float64, a["ld"], d_times if a["times"] else None, a["lengths"], t_cap,
                                           a["offsets"], d_f, a["stride"], a["alignment"], None, d_x)
                assert e.value.status == status, what
                assert intact(), what
            # 2^31 (walk, step) pairs: refused before a table is read
            lib, handles = world.prims[0].lib, rw._handles(world.prims)
            assert lib.mg_walks_time_functions(3, handles, _capi._host_ptr(node_of), _capi._host_ptr(n_steps), d_P.ptr, _capi.MG_F64, 2 ** 31, 1, LD, 1.0, d_t.ptr,
                                               d_l.ptr, t_cap) == UNSUPPORTED
            assert lib.mg_walks_frames_at(3, handles, _capi._host_ptr(node_of), _capi._host_ptr(n_steps), d_P.ptr, _capi.MG_F64, 2 ** 30, 2, LD, d_times.ptr,
                                          _capi._host_ptr(lengths), t_cap, _capi._host_ptr(offsets), None, None, d_f.ptr, stride, d_x.ptr) == UNSUPPORTED
            assert intact()
            # valid calls afterwards succeed; the length of a step a walk does not have is not read
            rw.walks_time_functions_dev(world.prims, node_of, n_steps, d_P, np.float64, LD, 1.6, d_t, d_l, t_cap)
            got_l = world.ctx.download(d_l, (n, s_max), np.int32)
            assert np.array_equal(got_l, lengths)
            rw.walks_frames_at_dev(world.prims, node_of, n_steps, d_P, np.float64, LD, d_t, absent_len, t_cap, offsets, d_f, stride, None, None, d_x)
            frames, transforms = world.ctx.download(d_f, (n, stride, D), np.float64), world.ctx.download(d_x, (n, s_max, 4), np.float64)
            _assert_contract(world, walks, P, times, lengths, offsets, frames, transforms, None, None)
    finally:
        too_long.close()
