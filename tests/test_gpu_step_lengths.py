"""mg_step_lengths on the device (csrc/mg_step_length.hip): step lengths without frames in memory against the reference's own
frames, against the library's float64 frames, bit for bit across batch sizes, items, slices and latent dtypes, at the shape
edges, its errors, and through the graph and walk call sites."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conftest import GOLDEN_CASES, golden_model, load_golden
from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import graph_walk as gw
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraph, HipPrimitiveSet, step_lengths_host
from test_graph_walk_host import START_POSE, primitive_jsons, walk_case

pytestmark = pytest.mark.gpu

POSITION_BOUND = 4e-12          # per position, times the scale: what the float64 frames path is held to (test_gpu_parity.py:77)


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def prims(ctx):
    """The primitives of the batch tests: tiny_tm and odd_shape (their golden models), walk_32 (the 'walk' primitive)."""
    out = {name: _capi.Primitive(ctx, golden_model(name)[0]) for name in ("tiny_tm", "odd_shape")}
    out["walk_32"] = _capi.Primitive(ctx, synthetic.make_walk_primitive(seed=0))
    yield out
    for p in out.values():
        p.close()


def _scale(frames):
    return max(1.0, float(np.abs(frames).max()))


def _device_bound(F, scale):
    """positions that differ in the last bit at both ends of each segment, and a sqrt that is not correctly rounded"""
    return max(F - 1, 1) * 8 * 2.0 ** -53 * scale


def _eq(a, b):
    np.testing.assert_array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- against the reference's frames and the device's own -------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_step_lengths_against_the_reference_frames_and_the_float64_frames(ctx, name):
    """Observed on an MI355X: within 1.8e-12 (arc length) and 2.3e-13 (distance) of the reference's frames; no difference at all from
    the library's own float64 frames in any case."""
    data, g = golden_model(name)
    prim = _capi.Primitive(ctx, data)
    S, frames = g["S"], g["frames"]
    F, scale = frames.shape[1], _scale(frames)
    arc, dist = prim.step_lengths(S, "both")
    assert arc.shape == dist.shape == (len(S),) and arc.dtype == dist.dtype == np.float64
    ref_arc, ref_dist = step_lengths_host(frames[:, :, :3])
    print("%s: reference  arc %.3g (bound %.3g)  distance %.3g (bound %.3g)" % (
        name, np.abs(arc - ref_arc).max(), (F - 1) * 2 * np.sqrt(2) * POSITION_BOUND * scale, np.abs(dist - ref_dist).max(),
        2 * np.sqrt(3) * POSITION_BOUND * scale))
    np.testing.assert_allclose(arc, ref_arc, rtol=0, atol=(F - 1) * 2 * np.sqrt(2) * POSITION_BOUND * scale)
    np.testing.assert_allclose(dist, ref_dist, rtol=0, atol=2 * np.sqrt(3) * POSITION_BOUND * scale)
    own_arc, own_dist = step_lengths_host(prim.back_project_frames_f64(S)[:, :, :3])
    print("%s: own frames arc %.3g  distance %.3g (bound %.3g; ulp of the arc %.3g)" % (
        name, np.abs(arc - own_arc).max(), np.abs(dist - own_dist).max(), _device_bound(F, scale), np.spacing(np.abs(own_arc).max())))
    np.testing.assert_allclose(arc, own_arc, rtol=0, atol=_device_bound(F, scale))
    np.testing.assert_allclose(dist, own_dist, rtol=0, atol=_device_bound(F, scale))
    # each method alone: the same bits
    _eq(prim.step_lengths(S, "arc_length"), arc)
    _eq(prim.step_lengths(S, "distance"), dist)
    _eq(prim.step_lengths(S), arc)
    with pytest.raises(NotImplementedError):
        prim.step_lengths(S, "other")
    prim.close()


# ---- batch independence, bit for bit ---------------------------------------------------------------------------------------
def _rows(prim, n, seed):
    return 0.8 * np.random.default_rng(seed).standard_normal((n, prim.n_components))


def test_a_candidate_does_not_depend_on_the_batch_or_the_other_items(prims):
    walk, tiny, odd = prims["walk_32"], prims["tiny_tm"], prims["odd_shape"]
    g = load_golden("walk_32")
    S = np.concatenate((g["S"], 0.5 * g["S"], 1.5 * g["S"], _rows(walk, 257 - 96, 5)))      # 257 distinct rows; row 0 the fixture's
    alone = walk.step_lengths(S[:1], "both")
    for n in (63, 64, 65, 257):
        arc, dist = walk.step_lengths(S[:n], "both")
        _eq(arc[:1], alone[0])
        _eq(dist[:1], alone[1])
    full = walk.step_lengths(S, "both")
    for n in (63, 65):
        arc, dist = walk.step_lengths(S[:n], "both")
        _eq(arc, full[0][:n])
        _eq(dist, full[1][:n])
    # three items over ONE matrix, ld greater than the columns used, non-zero offsets: tiny_tm (5 rows), odd_shape (0), walk (65)
    Lw, Lt, Lo = walk.n_components, tiny.n_components, odd.n_components
    St = _rows(tiny, 5, 6)
    M = np.full((65, 3 + Lt + 2 + Lw + 4), 7.25)
    M[:5, 3:3 + Lt] = St
    M[:, 3 + Lt + 2:3 + Lt + 2 + Lw] = S[:65]
    table = (_capi.StepLengthItem * 3)()
    outs = [np.full((2, n), -1.0) for n in (5, 0, 65)]
    for rec, prim, off, n, out in zip(table, (tiny, odd, walk), (3, 1, 3 + Lt + 2), (5, 0, 65), outs):
        rec.prim, rec.latents, rec.latent_offset, rec.n_samples, rec.ld = prim.handle.value, M.ctypes.data, off, n, M.shape[1]
        rec.arc_length, rec.distance = out[0].ctypes.data, out[1].ctypes.data
    assert Lo + 1 <= M.shape[1]
    _capi.step_lengths_table(walk.lib, 3, table, np.float64)
    _eq(outs[2][0], full[0][:65])
    _eq(outs[2][1], full[1][:65])
    _eq(outs[2][0][:1], alone[0])
    want = tiny.step_lengths(St, "both")
    _eq(outs[0][0], want[0])
    _eq(outs[0][1], want[1])
    for i in range(5):                                    # ... and every row of the small item alone
        one = tiny.step_lengths(St[i:i + 1], "both")
        _eq(outs[0][0][i:i + 1], one[0])
        _eq(outs[0][1][i:i + 1], one[1])
    # the wrapper's form of the same call
    got = _capi.step_lengths([(tiny, M[:5], 3), (odd, M[:0], 1), (walk, M, 3 + Lt + 2)], "both")
    _eq(got[0][0], want[0])
    assert got[1][0].shape == (0,) and got[1][1].shape == (0,)
    _eq(got[2][1], full[1][:65])


def test_float32_latents_give_the_bits_of_their_float64_values(prims):
    for name, n in (("walk_32", 33), ("tiny_tm", 5)):
        prim = prims[name]
        S32 = _rows(prim, n, 8).astype(np.float32)
        a32, d32 = prim.step_lengths(S32, "both")
        a64, d64 = prim.step_lengths(S32.astype(np.float64), "both")
        _eq(a32, a64)
        _eq(d32, d64)
    with pytest.raises(TypeError):
        _capi.step_lengths([(prims["tiny_tm"], S32), (prims["tiny_tm"], S32.astype(np.float64))])


def test_a_call_with_more_items_than_a_launch_takes_goes_in_slices(prims):
    tiny = prims["tiny_tm"]
    n_items = _capi.MG_STEP_LENGTH_MAX_ITEMS + 1
    S = _rows(tiny, 3 * n_items, 9)
    parts = [np.ascontiguousarray(S[3 * i:3 * i + 3]) for i in range(n_items)]
    got = _capi.step_lengths([(tiny, part) for part in parts], "both")
    assert len(got) == n_items
    for part, (arc, dist) in zip(parts, got):
        one = tiny.step_lengths(part, "both")
        _eq(arc, one[0])
        _eq(dist, one[1])
    # the same through the device-pointer form: one latent matrix on the device, one item per three rows
    ctx = tiny.ctx
    with ctx.buffers() as bufs:
        d_S, d_out = bufs.upload(S), bufs.upload(np.full((2, 3 * n_items), -1.0))
        table = (_capi.StepLengthItem * n_items)()
        for i, rec in enumerate(table):
            rec.prim, rec.latents, rec.latent_offset, rec.n_samples, rec.ld = tiny.handle.value, d_S.address + 8 * 3 * i * S.shape[1], 0, 3, S.shape[1]
            rec.arc_length, rec.distance = d_out.address + 8 * 3 * i, d_out.address + 8 * 3 * (n_items + i)
        _capi.step_lengths_table(tiny.lib, n_items, table, np.float64, host=False)
        ctx.synchronize()
        out = ctx.download(d_out, (2, 3 * n_items), np.float64)
    _eq(out[0], np.concatenate([a for a, _ in got]))
    _eq(out[1], np.concatenate([d for _, d in got]))


# ---- shape edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3])
def test_the_fewest_canonical_frames(ctx, F):
    """Two canonical frames, one segment, are the fewest: the knot vector synthetic builds for one frame has an empty domain,
    which mg_primitive_create refuses."""
    if F == 2:
        with pytest.raises(_capi.MGError):
            _capi.Primitive(ctx, synthetic.make_primitive(seed=41, n_components=3, n_frames=1, n_basis=4, n_dim=7, n_gmm=2))
    data = synthetic.make_primitive(seed=40 + F, n_components=3, n_frames=F, n_basis=4, n_dim=7, n_gmm=2)
    prim = _capi.Primitive(ctx, data)
    S = _rows(prim, 17, F)
    arc, dist = prim.step_lengths(S, "both")
    frames = prim.back_project_frames_f64(S)
    assert frames.shape[1] == F
    own_arc, own_dist = step_lengths_host(frames[:, :, :3])
    assert (arc > 0).all() and (dist > 0).all()
    np.testing.assert_allclose(arc, own_arc, rtol=0, atol=_device_bound(F, _scale(frames)))
    np.testing.assert_allclose(dist, own_dist, rtol=0, atol=_device_bound(F, _scale(frames)))
    if F == 2:                                            # one segment: the arc length is the ground-plane part of the distance
        assert (arc <= dist).all()
    prim.close()


def test_translation_maxima_scale_the_root_path(ctx):
    data = synthetic.make_tiny_primitive(seed=3, translation_maxima=(1.5, 2.0, 0.5))
    plain = synthetic.make_tiny_primitive(seed=3)
    prim, prim1 = _capi.Primitive(ctx, data), _capi.Primitive(ctx, plain)
    S = _rows(prim, 19, 4)
    arc, dist = prim.step_lengths(S, "both")
    model = gw._HostModel(data)                        # NumPy: mean and eigenvectors scaled by the maxima, de Boor's recurrence
    root = np.stack([model.frames(s)[1][:, :3] for s in S])
    F, scale = root.shape[1], _scale(root)
    ref_arc, ref_dist = step_lengths_host(root)
    np.testing.assert_allclose(arc, ref_arc, rtol=0, atol=(F - 1) * 2 * np.sqrt(2) * POSITION_BOUND * scale)
    np.testing.assert_allclose(dist, ref_dist, rtol=0, atol=2 * np.sqrt(3) * POSITION_BOUND * scale)
    assert np.abs(arc - prim1.step_lengths(S)).max() > 1e-3 * scale      # the unscaled model walks another path
    prim.close()
    prim1.close()


def test_zero_root_eigenvectors_give_the_mean_path_for_every_candidate(ctx):
    data = synthetic.make_tiny_primitive(seed=5)
    NB, D = int(data["n_basis_spatial"]), int(data["n_dim_spatial"])
    eig = np.array(data["eigen_vectors_spatial"]).reshape(-1, NB, D)
    eig[:, :, :3] = 0.0
    data["eigen_vectors_spatial"] = eig.reshape(len(eig), -1).tolist()
    prim = _capi.Primitive(ctx, data)
    S = 3.0 * _rows(prim, 37, 6)
    arc, dist = prim.step_lengths(S, "both")
    mean_arc, mean_dist = prim.step_lengths(np.zeros((1, prim.n_components)), "both")
    assert mean_arc[0] > 0
    _eq(arc, np.repeat(mean_arc, 37))
    _eq(dist, np.repeat(mean_dist, 37))
    prim.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_latent_that_is_not_finite_gives_nan_for_its_candidate_alone(prims, bad):
    for name in ("tiny_tm", "walk_32"):
        prim = prims[name]
        S = _rows(prim, 3, 12)
        want = prim.step_lengths(S, "both")
        S[1, prim.n_components - 1] = bad
        arc, dist = prim.step_lengths(S, "both")
        assert np.isnan(arc[1]) and np.isnan(dist[1])
        _eq(arc[[0, 2]], want[0][[0, 2]])
        _eq(dist[[0, 2]], want[1][[0, 2]])


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_before_any_launch_and_leave_the_library_usable(ctx, prims):
    tiny = prims["tiny_tm"]
    L = tiny.n_components
    S = _rows(tiny, 4, 13)
    want = tiny.step_lengths(S, "both")
    other_ctx = _capi.Context(0)
    other = _capi.Primitive(other_ctx, synthetic.make_tiny_primitive(seed=2))

    def table(n=1, **fields):
        """n valid items over S; `fields` overwrite members of the LAST one"""
        t = (_capi.StepLengthItem * n)()
        keep = []
        for rec in t:
            arc, dist = np.full(4, -1.0), np.full(4, -1.0)
            keep.append((arc, dist))
            rec.prim, rec.latents, rec.latent_offset, rec.n_samples, rec.ld = tiny.handle.value, S.ctypes.data, 0, 4, L
            rec.arc_length, rec.distance = arc.ctypes.data, dist.ctypes.data
        for key, value in fields.items():
            setattr(t[n - 1], key, value)
        return t, keep

    cases = [("NULL item table", 1, None),
             ("negative item count", -1, table()[0]),
             ("NULL primitive", 2, table(2, prim=None)[0]),
             ("NULL latents", 1, table(latents=None)[0]),
             ("columns past ld", 1, table(latent_offset=1)[0]),
             ("negative offset", 1, table(latent_offset=-1)[0]),
             ("negative samples", 2, table(2, n_samples=-1)[0]),
             ("negative ld", 1, table(ld=-1, n_samples=0)[0]),
             ("both outputs NULL", 1, table(arc_length=None, distance=None)[0]),
             ("two contexts", 2, table(2, prim=other.handle.value)[0])]
    for what, n, t in cases:
        for host in (True, False):                         # the checks come before anything is copied or launched in either form
            with pytest.raises(_capi.MGError) as info:
                _capi.step_lengths_table(tiny.lib, n, t, np.float64, host=host)
            assert info.value.status == _capi.MG_ERR_INVALID_ARGUMENT, what
        got = tiny.step_lengths(S, "both")
        _eq(got[0], want[0])
        _eq(got[1], want[1])
    # a failing item behind valid ones: nothing of the call is written
    t, keep = table(3, latents=None)
    with pytest.raises(_capi.MGError):
        _capi.step_lengths_table(tiny.lib, 3, t, np.float64)
    assert all((arc == -1.0).all() and (dist == -1.0).all() for arc, dist in keep)
    # nothing to do: MG_OK
    _capi.step_lengths_table(tiny.lib, 0, None, np.float64)
    t, keep = table(2, n_samples=0)
    t[0].n_samples = 0
    _capi.step_lengths_table(tiny.lib, 2, t, np.float64)
    assert all((arc == -1.0).all() for arc, _ in keep)
    assert _capi.step_lengths([]) == []
    other.close()
    other_ctx.close()


# ---- the graph -------------------------------------------------------------------------------------------------------------
def _graph(ctx):
    """Four nodes of one action with different shapes; the statistics come from the file, so loading samples nothing."""
    shapes = [(5, 12, 7, 11), (8, 33, 9, 11), (3, 20, 6, 7), (40, 60, 12, 79)]
    mms = {"n%d" % i: synthetic.make_primitive(seed=60 + i, n_components=L, n_frames=F, n_basis=NB, n_dim=D, n_gmm=3, name="n%d" % i)
           for i, (L, F, NB, D) in enumerate(shapes)}
    stats = {name: {"average_step_length": -1.0, "n_standard_transitions": -1} for name in mms}
    data = {"subgraphs": {"walk": {"name": "walk", "info": {"stats": stats}, "nodes": {name: {"name": name, "mm": mm} for name, mm in mms.items()}}},
            "transitions": {"walk:n0": ["walk:n1", "walk:n2"], "walk:n1": ["walk:n0"], "walk:n3": ["walk:n0", "walk:n1", "walk:n2"]}}
    return HipMotionStateGraph(context=ctx).build_from_graph_data(data)


@pytest.mark.parametrize("method", ["median", "average"])
def test_update_all_motion_stats_is_the_per_node_update_in_one_call(ctx, method):
    graph = _graph(ctx)
    assert len(graph.nodes) == 4
    np.random.seed(9)
    graph.update_all_motion_stats(5, method)
    got = {key: (node.average_step_length, node.n_standard_transitions) for key, node in graph.nodes.items()}
    np.random.seed(9)
    for node in graph.nodes.values():
        node.update_motion_stats(5, method)
    for key, node in graph.nodes.items():
        value = node.average_step_length
        print("%s %s: %.17g against %.17g" % (key[1], method, got[key][0], value))
        assert value > 0 and abs(got[key][0] - value) <= 1e-9 * max(1.0, value)
        assert got[key][1] == node.n_standard_transitions
    assert sorted(n for _, n in got.values()) == [0, 1, 2, 3]
    # a subset, in the caller's order: the other nodes keep their values
    before = graph.nodes[("walk", "n1")].average_step_length
    np.random.seed(3)
    want = []
    for name in ("n2", "n0"):
        graph.nodes[("walk", name)].update_motion_stats(3, method)
        want.append(graph.nodes[("walk", name)].average_step_length)
    np.random.seed(3)
    graph.update_all_motion_stats(3, method, node_keys=[("walk", "n2"), ("walk", "n0")])
    for name, value in zip(("n2", "n0"), want):
        assert abs(graph.nodes[("walk", name)].average_step_length - value) <= 1e-9 * max(1.0, value)
    assert graph.nodes[("walk", "n1")].average_step_length == before


def test_step_lengths_on_device_of_a_node(ctx):
    graph = _graph(ctx)
    node = graph.nodes[("walk", "n3")]
    np.random.seed(2)
    S = node.sample_low_dimensional_vectors(21)
    for method in ("arc_length", "distance"):
        got = node.step_lengths_on_device(S, method)
        want = np.array([node.get_step_length_for_sample(s, method) for s in S[:4]])
        assert got.shape == (21,) and got.dtype == np.float64
        np.testing.assert_allclose(got[:4], want, rtol=0, atol=1e-9 * max(1.0, want.max()))


# ---- walks -----------------------------------------------------------------------------------------------------------------
class _Graph(object):
    def __init__(self, pset):
        self.nodes = {("walk", name): node for name, node in pset.nodes.items()}


def test_walk_step_lengths_are_the_lengths_of_the_aligned_steps(ctx):
    """Observed on an MI355X: arc length within 2.3e-13 and distance within 2.8e-14 of the aligned frames' (bounds 2.3e-11 and 6.7e-11)."""
    sequence = [0, 1, 0]                                   # three steps, the first primitive twice
    steps, S, alignment, hip_sk, _, _ = walk_case("start_pose", "Hips", n_walks=5, sequence=sequence)
    pset = HipPrimitiveSet(primitive_jsons(), context=ctx)
    keys = [("walk", "w%d" % k) for k in sequence]
    mps = [pset.nodes["w%d" % k] for k in sequence]
    frames, offsets = gw.assemble_walks(_Graph(pset), keys, S, alignment=alignment, skeleton=hip_sk)
    got = gw.walk_step_lengths(mps, S)
    dists = gw.walk_step_lengths(mps, S, method="distance")
    assert got.shape == dists.shape == (5, 3)
    scale = _scale(frames[:, :, :3])
    for i, mp in enumerate(mps):
        a, b = int(offsets[0, i]), int(offsets[0, i + 1])
        assert np.array_equal(offsets[:, i], np.full(5, a)) and b - a == mp.n_canonical_frames
        ref_arc, ref_dist = step_lengths_host(frames[:, a:b, :3])
        bound = 4 * _device_bound(b - a, scale)            # x 4: the alignment's rotation moves each position by a few ulps of the scale
        print("step %d: arc %.3g  distance %.3g (bound %.3g)" % (i, np.abs(got[:, i] - ref_arc).max(), np.abs(dists[:, i] - ref_dist).max(), bound))
        np.testing.assert_allclose(got[:, i], ref_arc, rtol=0, atol=bound)
        np.testing.assert_allclose(dists[:, i], ref_dist, rtol=0, atol=bound)
        # a step is its primitive's candidate whatever the walk around it
        off = sum(m.get_n_spatial_components() for m in mps[:i])
        _eq(got[:, i], mp._prim.step_lengths(np.ascontiguousarray(S[:, off:off + mp.get_n_spatial_components()])))
    _eq(got[:, 0], gw.walk_step_lengths(mps[:1], S)[:, 0])

    walk = gw.HipGraphWalk(_Graph(pset), start_pose=START_POSE, ctx=ctx)
    at = 0
    for key, mp in zip(keys, mps):
        L = mp.get_n_spatial_components()
        walk.steps.append(gw.HipGraphWalkStep(key, S[2, at:at + L], L, 0))
        at += L
    lengths = walk.update_arc_lengths()
    _eq(lengths, got[2])
    assert [st.arc_length for st in walk.steps] == [float(v) for v in np.cumsum(got[2])]
    assert gw.HipGraphWalk(_Graph(pset), ctx=ctx).update_arc_lengths().shape == (0,)
    walk.close()
