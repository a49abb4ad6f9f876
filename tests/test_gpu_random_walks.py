"""Random walks on the device: mg_walks_frames, mg_walks_sample_latents and the Python layer over them (tests/random_walk_cases.py).

The contract of mg_walks_frames is exact: every walk of a mixed population has the bits mg_walk_frames gives for that walk alone.
The sampler's is exact too: the component is the NumPy restatement's, the row is mg_gmm_sample_rows' at the row's global index.
Only the round trip against the NumPy frames carries a tolerance, tests/test_graph_walk_host.py's WALK_TOLERANCE, the bound every
device test of mg_walk_frames holds against assemble_walk_host.
"""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import random_walk_cases as rc
from morphablegraphs_amd import _capi, graph_walk as gw, random_walks as rw
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraph
from test_graph_walk_host import WALK_TOLERANCE, root_scale

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25
D = 3 + 4 * rc.N_ANIMATED
LD = 16                                     # wider than the widest mixture (14)
WIDTH = [L for L, _, _, _, _ in rc.SHAPES]
FRAMES = [F for _, F, _, _, _ in rc.SHAPES]


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


def _solo(world, seq, rows, dtype, alignment, skeleton):
    """mg_walk_frames for one walk alone: its latents packed into one row.  (frames (T, D), transforms (n_steps, 4))."""
    S = np.concatenate([rows[i, :WIDTH[k]] for i, k in enumerate(seq)])[None, :].astype(dtype)
    offs = np.concatenate(([0], np.cumsum([WIDTH[k] for k in seq])[:-1]))
    T = sum(FRAMES[k] for k in seq)
    with world.ctx.buffers() as bufs:
        d_f, d_x = bufs.malloc(8 * T * D), bufs.malloc(8 * len(seq) * 4)
        gw.walk_frames_dev([world.prims[k] for k in seq], offs, bufs.upload(S), dtype, 1, S.shape[1], d_f, T, alignment=alignment, skeleton=skeleton,
                           d_transforms=d_x)
        return world.ctx.download(d_f, (T, D), np.float64), world.ctx.download(d_x, (len(seq), 4), np.float64)


def _mixed(world, walks, P, alignment=None, skeleton=None, frame_offset=None, stride=None):
    """mg_walks_frames into buffers filled with the sentinel: (frames (n, stride, D), transforms (n, s_max, 4))."""
    node_of, n_steps = rc.tables(walks)
    stride = stride or max(sum(FRAMES[k] for k in seq) for seq in walks)
    with world.ctx.buffers() as bufs:
        d_f = bufs.upload(np.full((len(walks), stride, D), SENTINEL))
        d_x = bufs.upload(np.full(node_of.shape + (4,), SENTINEL))
        rw.walks_frames_dev(world.prims, node_of, n_steps, bufs.upload(P), P.dtype, P.shape[2], d_f, stride, frame_offset, alignment, skeleton, d_x)
        return world.ctx.download(d_f, (len(walks), stride, D), np.float64), world.ctx.download(d_x, node_of.shape + (4,), np.float64)


def _assert_contract(world, walks, P, frames, transforms, alignment, skeleton, offsets=None, which=None):
    for w in (range(len(walks)) if which is None else which):
        seq = walks[w]
        fr, tr = _solo(world, seq, P[w], P.dtype, alignment, skeleton)
        owned, row = np.zeros(frames.shape[1], dtype=bool), 0
        for i, k in enumerate(seq):
            at = row if offsets is None else int(offsets[w, i])
            assert _same_bits(frames[w, at:at + FRAMES[k]], fr[row:row + FRAMES[k]]), (w, i)
            owned[at:at + FRAMES[k]] = True
            row += FRAMES[k]
        assert _same_bits(transforms[w, :len(seq)], tr), w
        assert (frames[w, ~owned] == SENTINEL).all() and (transforms[w, len(seq):] == SENTINEL).all(), w       # what no step owns is not written


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["none", "previous", "start_pose", "previous_spine"])
def test_every_walk_of_a_mixed_population_is_its_solo_call(world, kind, dtype):
    """Alignment modes 0, 1 and 2, a non-root aligning joint with a skeleton, both latent dtypes; the _host twin gives the device's bits."""
    alignment, skeleton = world.alignments[kind]
    walks = rc.CONTRACT_WALKS
    node_of, n_steps = rc.tables(walks)
    assert n_steps.tolist() == [1, 2, 3, 4, 4, 2] and walks[1] == walks[5] and walks[3][1] == walks[3][2]
    P = rc.latents(node_of, LD, dtype=dtype)
    frames, transforms = _mixed(world, walks, P, alignment, skeleton)
    _assert_contract(world, walks, P, frames, transforms, alignment, skeleton)
    assert np.isfinite(frames[frames != SENTINEL]).all()
    host_f, host_x = np.full(frames.shape, SENTINEL), np.full(transforms.shape, SENTINEL)
    rw.walks_frames_host(world.prims, node_of, n_steps, P, host_f, None, alignment, skeleton, host_x)
    assert _same_bits(host_f, frames) and _same_bits(host_x, transforms)


def test_given_frame_offsets_with_gaps(world):
    """Steps out of order and apart: walk w's step i starts where the table says, the rows between them keep the sentinel."""
    walks = rc.CONTRACT_WALKS
    node_of, n_steps = rc.tables(walks)
    offsets = np.zeros(node_of.shape, dtype=np.int64)
    for w, seq in enumerate(walks):
        row = 3
        for i in (reversed(range(len(seq))) if w % 2 else range(len(seq))):      # odd walks: the last step first
            offsets[w, i] = row
            row += FRAMES[seq[i]] + 1 + i
    stride = int(max(offsets[w, i] + FRAMES[k] for w, seq in enumerate(walks) for i, k in enumerate(seq))) + 2
    P = rc.latents(node_of, LD, seed=6)
    alignment, skeleton = world.alignments["previous"]
    frames, transforms = _mixed(world, walks, P, alignment, skeleton, offsets, stride)
    _assert_contract(world, walks, P, frames, transforms, alignment, skeleton, offsets)
    assert (frames[:, :3] == SENTINEL).all() and (frames[:, -2:] == SENTINEL).all()


def test_a_walk_does_not_depend_on_its_population(world):
    seq = rc.CONTRACT_WALKS[3]
    rows = rc.latents(np.zeros((1, 4), dtype=np.int32), LD, seed=8)
    alignment, skeleton = world.alignments["start_pose"]
    got = []
    for n, at in ((1, 0), (6, 3), (65, 64)):
        walks = [rc.CONTRACT_WALKS[(w + 1) % 6] for w in range(n)]
        walks[at] = seq
        node_of, _ = rc.tables(walks)
        P = rc.latents(node_of, LD, seed=20 + n)
        P[at, :4] = rows[0]
        frames, transforms = _mixed(world, walks, P, alignment, skeleton)
        T = sum(FRAMES[k] for k in seq)
        got.append((frames[at, :T], transforms[at, :4]))
    for fr, tr in got[1:]:
        assert _same_bits(fr, got[0][0]) and _same_bits(tr, got[0][1])
    fr, tr = _solo(world, seq, rows[0], np.float64, alignment, skeleton)
    assert _same_bits(got[0][0], fr) and _same_bits(got[0][1], tr)


def test_past_65536_walks_the_prefix_search_finds_every_walk(world):
    """70 000 one-step walks of the 31-frame primitive with every 1000th a 65-frame one: one grid of 70 140 tiles, the walks'
    first tiles no longer their indices; three sampled walks and the last one against their solo calls."""
    n = 70000
    walks = [[2] if w % 1000 == 999 else [0] for w in range(n)]
    node_of, n_steps = rc.tables(walks)
    P = rc.latents(node_of, 12, seed=9)
    stride = 65
    with world.ctx.buffers() as bufs:
        d_f = bufs.malloc(8 * n * stride * D)
        rw.walks_frames_dev(world.prims, node_of, n_steps, bufs.upload(P), P.dtype, 12, d_f, stride)
        for w in (0, 999, 65536, n - 1):
            T = FRAMES[walks[w][0]]
            got = world.ctx.download(d_f.address + 8 * w * stride * D, (T, D), np.float64)
            fr, _ = _solo(world, walks[w], P[w], np.float64, None, None)
            assert _same_bits(got, fr), w


SAMPLE_WALKS = [[0, 1, 2], [2], [1, 1], [2, 0, 1], [0]]


def _sample(world, walks, seed, dtype, ld=LD):
    node_of, n_steps = rc.tables(walks)
    with world.ctx.buffers() as bufs:
        d_x = bufs.upload(np.full(node_of.shape + (ld,), SENTINEL, dtype=dtype))
        d_c = bufs.upload(np.full(node_of.shape, 77, dtype=np.int32))
        rw.sample_walk_latents_dev(world.prims, node_of, n_steps, seed, d_x, dtype, ld, d_c)
        return world.ctx.download(d_x, node_of.shape + (ld,), dtype), world.ctx.download(d_c, node_of.shape, np.int32)


def test_the_samplers_bits(world):
    node_of, n_steps = rc.tables(SAMPLE_WALKS)
    n, s_max = node_of.shape
    assert (n, s_max) == (5, 3)
    x, comp = _sample(world, SAMPLE_WALKS, 119, np.float64)
    want = rc.walk_components([d["gmm_weights"] for d in world.jsons], node_of, n_steps, 119)
    # (the seed is chosen so that the restatement draws every component of both mixtures that have more than one)
    assert set(want[node_of == 2].tolist()) == {0, 1, 2} and set(want[node_of == 1].tolist()) == {0, 1}
    assert np.array_equal(comp, want)
    for w in range(n):
        for i in range(s_max):
            if i >= n_steps[w]:
                assert (x[w, i] == 0.0).all() and comp[w, i] == -1
                continue
            prim = world.prims[node_of[w, i]]
            Lg = prim.n_gmm_dims
            counts = np.zeros(prim.n_gmm, dtype=np.int64)
            counts[comp[w, i]] = n * s_max                            # all rows of the draw in the row's component
            with world.ctx.buffers() as bufs:
                d_row = bufs.malloc(8 * Lg)
                prim.gmm_sample_dev(counts, 119, d_row, np.float64, Lg, rows=(w * s_max + i, 1))
                row = world.ctx.download(d_row, (Lg,), np.float64)
            assert _same_bits(x[w, i, :Lg], row), (w, i)
            assert (x[w, i, Lg:] == 0.0).all() and Lg < LD
    again, comp_again = _sample(world, SAMPLE_WALKS, 119, np.float64)
    assert _same_bits(again, x) and np.array_equal(comp_again, comp)
    other, _ = _sample(world, SAMPLE_WALKS, 120, np.float64)
    assert not np.array_equal(other, x)
    x32, comp32 = _sample(world, SAMPLE_WALKS, 119, np.float32)
    assert np.array_equal(x32.view(np.uint32), x.astype(np.float32).view(np.uint32)) and np.array_equal(comp32, comp)
    # a row depends on (seed, its global index, its node) only: the same rows inside a longer population
    longer, _ = _sample(world, SAMPLE_WALKS + [[1, 2, 0]], 119, np.float64)
    assert _same_bits(longer[:n], x)
    host_x, host_c = rw.sample_walk_latents(world.prims, node_of, n_steps, 119, np.float64, LD)
    assert _same_bits(host_x, x) and np.array_equal(host_c, comp)


def test_the_tables_are_uploaded_when_they_differ_and_only_then(world):
    node_of, _ = rc.tables(rc.CONTRACT_WALKS)
    P = rc.latents(node_of, LD)
    for name, call in (("walks_mixed", lambda walks: _mixed(world, walks, P[:len(walks)])), ("walks_sample", lambda walks: _sample(world, walks, 1, np.float64))):
        call(rc.CONTRACT_WALKS)
        u0 = world.ctx.table_uploads(name)
        first = call(rc.CONTRACT_WALKS)
        assert world.ctx.table_uploads(name) == u0
        call(rc.CONTRACT_WALKS[:4])
        assert world.ctx.table_uploads(name) == u0 + 1
        again = call(rc.CONTRACT_WALKS)
        assert world.ctx.table_uploads(name) == u0 + 2 and all(_same_bits(a, b) for a, b in zip(first[:1], again[:1]))


def test_round_trip_through_the_graph(world):
    graph = HipMotionStateGraph(context=world.ctx).build_from_graph_data(rc.graph_data(world.jsons))
    try:
        walks = graph.generate_random_walks("walk", 3, 6, seed=11, rng=random.Random(2))
        assert walks.node_keys == rw.choose_random_walks(graph, "walk", 3, 6, random.Random(2)) and len({tuple(k) for k in walks.node_keys}) > 1
        assert walks.n_steps.tolist() == [len(k) for k in walks.node_keys] and {len(k) for k in walks.node_keys} <= {4, 5}
        params, comp = walks.parameters_host(), walks.components_host()
        assert params.shape == (6, int(walks.n_steps.max()), 14) and ((comp >= 0) == (walks.node_of >= 0)).all()
        frames, transforms = walks.frames(with_transforms=True)
        ref, _, ref_x = rw.assemble_walks_mixed_host([graph.nodes[k] for k in walks.nodes], walks.node_of, walks.n_steps, params)
        graph_walks = walks.to_graph_walks()
        for w in range(walks.n_walks):
            worst = float(np.max(np.abs(frames[w] - ref[w]))) / root_scale(ref[w])
            worst_x = float(np.nanmax(np.abs(transforms[w] - ref_x[w]))) / root_scale(ref[w])
            print("walk %d: frames %.3g, transforms %.3g of the root scale %.4g (bound %.3g)" % (w, worst, worst_x, root_scale(ref[w]), WALK_TOLERANCE))
            assert frames[w].shape == ref[w].shape and worst <= WALK_TOLERANCE and worst_x <= WALK_TOLERANCE
            assert np.isnan(transforms[w, walks.n_steps[w]:]).all()
            gwalk = graph_walks[w]
            assert [s.node_key for s in gwalk.steps] == [tuple(k) for k in walks.node_keys[w]]
            gwalk.convert_graph_walk_to_quaternion_frames()
            assert _same_bits(gwalk.get_quat_frames(), frames[w]), w
            assert len(gwalk.to_json()["steps"]) == walks.n_steps[w]
            gwalk.close()
        walks.close()
        # the reference's method: a list of {"node_key", "parameters"}, the nodes from the global `random`
        random.seed(4)
        np.random.seed(4)
        entries = graph.generate_random_walk("walk", 2)
        random.seed(4)
        assert [e["node_key"] for e in entries] == rw.choose_random_walks(graph, "walk", 2)[0]
        for e in entries:
            p = e["parameters"]
            assert p.dtype == np.float64 and p.shape == (graph.nodes[e["node_key"]].motion_primitive._prim.n_gmm_dims,) and np.isfinite(p).all() and p.any()
        graph.nodes[("walk", "b")].outgoing_edges[("walk", "c")].transition_model = object()
        with pytest.raises(NotImplementedError):
            graph.generate_random_walk("walk", 2)
        assert len(graph.generate_random_walk("walk", 2, use_transition_model=False)) >= 3
    finally:
        graph.close()


def test_misuse_is_refused_before_anything_is_written(world):
    walks = rc.CONTRACT_WALKS
    node_of, n_steps = rc.tables(walks)
    n, s_max = node_of.shape
    P = rc.latents(node_of, LD)
    stride = max(sum(FRAMES[k] for k in seq) for seq in walks)
    other_ctx = _capi.Context(0)
    foreign = _capi.Primitive(other_ctx, world.jsons[1])
    narrow = _capi.Primitive(world.ctx, rc.synthetic.make_primitive(seed=3, n_components=4, n_frames=12, n_basis=6, n_dim=7, n_gmm=2, name="narrow"))
    spine, _ = world.alignments["previous_spine"]
    bad_node, neg_node, no_steps, many_steps = node_of.copy(), node_of.copy(), n_steps.copy(), n_steps.copy()
    bad_node[2, 1], neg_node[4, 3], no_steps[0], many_steps[5] = 3, -1, 0, s_max + 1
    overlap = np.zeros(node_of.shape, dtype=np.int64)
    overlap[:, 1:] = 20                                                   # every second step inside the first one's rows
    INVALID, UNSUPPORTED = _capi.MG_ERR_INVALID_ARGUMENT, _capi.MG_ERR_UNSUPPORTED
    IA = dict(prims=world.prims, node_of=node_of, n_steps=n_steps, ld=LD, frame_offset=None, alignment=None, skeleton=None, stride=stride)
    frame_cases = [("node index past the table", dict(node_of=bad_node), INVALID), ("negative node index", dict(node_of=neg_node), INVALID),
                   ("a walk without steps", dict(n_steps=no_steps), INVALID), ("more steps than s_max", dict(n_steps=many_steps), INVALID),
                   ("ld below a node's latents", dict(ld=8), INVALID), ("steps overlap", dict(frame_offset=overlap), INVALID),
                   ("a walk passes walk_stride", dict(stride=stride - 1), INVALID),
                   ("two contexts", dict(prims=[world.prims[0], foreign, world.prims[2]]), INVALID),
                   ("two widths", dict(prims=[world.prims[0], narrow, world.prims[2]]), INVALID),
                   ("a non-root aligning joint without a skeleton", dict(alignment=spine), INVALID)]
    sample_cases = [c for c in frame_cases[:4]] + [("ld below a node's mixture", dict(ld=13), INVALID), frame_cases[7], frame_cases[8]]
    try:
        with world.ctx.buffers() as bufs:
            d_P = bufs.upload(P)
            d_f, d_t = bufs.upload(np.full((n, stride, D), SENTINEL)), bufs.upload(np.full((n, s_max, 4), SENTINEL))
            d_x, d_c = bufs.upload(np.full((n, s_max, LD), SENTINEL)), bufs.upload(np.full((n, s_max), 77, dtype=np.int32))

            def intact():
                world.ctx.synchronize()
                return (world.ctx.download(d_f, (n, stride, D), np.float64) == SENTINEL).all() and (world.ctx.download(d_t, (n, s_max, 4), np.float64) == SENTINEL).all() \
                    and (world.ctx.download(d_x, (n, s_max, LD), np.float64) == SENTINEL).all() and (world.ctx.download(d_c, (n, s_max), np.int32) == 77).all()

            for what, change, status in frame_cases:
                a = dict(IA, **change)
                with pytest.raises(_capi.MGError) as e:
                    rw.walks_frames_dev(a["prims"], a["node_of"], a["n_steps"], d_P, np.float64, a["ld"], d_f, a["stride"], a["frame_offset"], a["alignment"],
                                        a["skeleton"], d_t)
                assert e.value.status == status, what
                assert intact(), what
            for what, change, status in sample_cases:
                a = dict(IA, **change)
                with pytest.raises(_capi.MGError) as e:
                    rw.sample_walk_latents_dev(a["prims"], a["node_of"], a["n_steps"], 5, d_x, np.float64, a["ld"], d_c)
                assert e.value.status == status, what
                assert intact(), what
            # the cap that remains: 2^31 (walk, step) pairs -- refused before a table is read
            lib, handles = world.prims[0].lib, rw._handles(world.prims)
            assert lib.mg_walks_frames(3, handles, _capi._host_ptr(node_of), _capi._host_ptr(n_steps), d_P.ptr, _capi.MG_F64, 2 ** 31, 1, LD, None, None, None,
                                       d_f.ptr, stride, d_t.ptr) == UNSUPPORTED
            assert lib.mg_walks_sample_latents(3, handles, _capi._host_ptr(node_of), _capi._host_ptr(n_steps), 2 ** 30, 2, C.c_uint64(5), d_x.ptr, _capi.MG_F64,
                                               LD, d_c.ptr) == UNSUPPORTED
            assert intact()
            # a valid call afterwards succeeds
            rw.walks_frames_dev(world.prims, node_of, n_steps, d_P, np.float64, LD, d_f, stride, d_transforms=d_t)
            rw.sample_walk_latents_dev(world.prims, node_of, n_steps, 5, d_x, np.float64, LD, d_c)
            frames, transforms = world.ctx.download(d_f, (n, stride, D), np.float64), world.ctx.download(d_t, (n, s_max, 4), np.float64)
            _assert_contract(world, walks, P, frames, transforms, None, None)
            assert np.array_equal(world.ctx.download(d_c, (n, s_max), np.int32), rc.walk_components([d["gmm_weights"] for d in world.jsons], node_of, n_steps, 5))
    finally:
        foreign.close()
        narrow.close()
        other_ctx.close()
