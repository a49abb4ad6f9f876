"""mg_walk_frames / graph_walk.py on the device: against assemble_walk_host (the arithmetic's NumPy statement, itself held to the
oracle's control-point chain in tests/test_graph_walk_host.py), against the chain of the existing entry points, across the batch,
at the shape boundaries of the kernels (tile = 32 frames, 64 steps per call), its errors, and HipGraphWalk end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import graph_walk as gw
from morphablegraphs_amd.frame_constraints import _Batch
from morphablegraphs_amd.motion_primitive_generator import HipMotionPrimitiveGenerator
from morphablegraphs_amd.motion_state_graph import HipPrimitiveSet
from test_graph_walk_host import CASES, SEQUENCE, SHAPES, START_POSE, WALK_TOLERANCE, primitive_jsons, root_scale, walk_case

pytestmark = pytest.mark.gpu

TILE = _capi.MG_WALK_TILE
D = 11


class _Graph(object):
    def __init__(self, pset, prefix="walk"):
        self.nodes = {(prefix, name): node for name, node in pset.nodes.items()}


@pytest.fixture(scope="module")
def pset():
    """The three primitives of the host test's cases plus: lengths at the tile's boundary (F = 31, 32), a time model (F = 16)."""
    extra = [synthetic.make_primitive(seed=80 + i, n_components=4, n_frames=F, n_basis=6, n_dim=D, n_gmm=2, name="t%d" % F) for i, F in enumerate((TILE - 1, TILE))]
    timed = synthetic.make_primitive(seed=90, n_components=4, n_frames=16, n_basis=6, n_dim=D, n_gmm=2, name="timed", n_time_components=2, n_basis_time=5)
    return HipPrimitiveSet(primitive_jsons() + extra + [timed])


def mps_of(pset, sequence):
    return [pset.nodes["w%d" % k if isinstance(k, int) else k] for k in sequence]


def run(mps, S, alignment=None, skeleton=None, times=None, lengths=None, frame_offset=None, stride=None, latent_offset=None):
    """One mg_walk_frames call: (frames (n, stride, D) over a NaN sentinel, transforms (n, n_steps, 4))."""
    S = _capi._latents(S)
    n, m = S.shape[0], len(mps)
    ctx = mps[0]._prim.ctx
    if latent_offset is None:
        latent_offset = np.concatenate(([0], np.cumsum([mp.get_n_spatial_components() for mp in mps])[:-1]))
    if stride is None:
        stride = (int(np.max(np.sum(lengths, axis=1))) if lengths is not None else sum(mp.n_canonical_frames for mp in mps)) + 3
    t_cap = 0 if times is None else times.shape[2]
    with ctx.buffers() as bufs:
        d_S, d_f, d_x = bufs.upload(S), bufs.upload(np.full((n, stride, D), np.nan)), bufs.malloc(8 * n * m * 4)
        d_t = bufs.upload(np.ascontiguousarray(times, dtype=np.float64)) if times is not None else None
        gw.walk_frames_dev([mp._prim for mp in mps], latent_offset, d_S, S.dtype, n, S.shape[1], d_f, stride, d_t, lengths, t_cap, frame_offset, alignment,
                           skeleton, d_x)
        return ctx.download(d_f, (n, stride, D), np.float64), ctx.download(d_x, (n, m, 4), np.float64)


def assert_close(got, ref):
    """within WALK_TOLERANCE of the largest |root coordinate| of the reference; NaN (unwritten rows) must coincide"""
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    worst = float(np.nanmax(np.abs(got - ref))) / root_scale(ref)
    print("disagreement %.3g of the root scale %.4g" % (worst, root_scale(ref)))
    assert worst <= WALK_TOLERANCE


# ---- 3. against the host statement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_walks", [1, 5])
@pytest.mark.parametrize("kind,node", CASES)
def test_walk_frames_match_the_host_statement(pset, kind, node, n_walks):
    steps, S, alignment, hip_sk, _, _ = walk_case(kind, node, n_walks=n_walks)
    ref, offsets, ref_x = gw.assemble_walk_host(steps, S, alignment=alignment, skeleton=hip_sk)
    got, got_x = run(mps_of(pset, SEQUENCE), S, alignment, hip_sk, stride=ref.shape[1])
    assert_close(got, ref)
    assert float(np.max(np.abs(got_x - ref_x))) / root_scale(ref) <= WALK_TOLERANCE
    # ... and through the package's batch entry point
    frames, offs = gw.assemble_walks(_Graph(pset), [("walk", "w%d" % k) for k in SEQUENCE], S, alignment=alignment, skeleton=hip_sk)
    assert np.array_equal(offs, offsets) and np.array_equal(frames, got)


# ---- 4. against the chain of the existing entry points ------------------------------------------------------------------
def test_an_unaligned_single_step_is_the_back_projection_bit_for_bit(pset):
    rng = np.random.default_rng(2)
    for name in ("w1", "t31", "t32"):                 # 33, 31 and 32 frames: two tiles, one short tile, one full tile
        mp = pset.nodes[name]
        S = 0.7 * rng.standard_normal((3, mp.get_n_spatial_components()))
        got, x = run([mp], S, stride=mp.n_canonical_frames)
        assert np.array_equal(got, mp._prim.back_project_frames_f64(S))
        assert np.array_equal(x, np.tile([1.0, 0.0, 0.0, 0.0], (3, 1, 1)))
    # given times: mg_back_project_frames_at's bits, ragged lengths
    mp = pset.nodes["w1"]
    S = 0.7 * rng.standard_normal((3, mp.get_n_spatial_components()))
    lengths = np.array([[TILE + 1], [1], [TILE - 1]], dtype=np.int32)
    times = np.sort(rng.uniform(0.0, mp.n_canonical_frames - 1.0, (3, 1, TILE + 2)), axis=2)
    got, _ = run([mp], S, times=times, lengths=lengths, frame_offset=np.zeros((3, 1), dtype=np.int64), stride=TILE + 2)
    ref = mp._prim.back_project_frames_at(S, times[:, 0], lengths[:, 0])
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(ref))


@pytest.mark.parametrize("kind,node", [("previous", "Spine"), ("start_pose", "Hips")])
def test_walk_frames_match_the_step_by_step_chain(pset, kind, node):
    """per step mg_back_project_frames_f64 -> mg_align_frames with the record built from the previous aligned last frame -> concatenate"""
    steps, S, alignment, hip_sk, _, _ = walk_case(kind, node, n_walks=1)
    mps = mps_of(pset, SEQUENCE)
    sk, joint = (hip_sk, node) if hip_sk is not None else (gw._ROOT_ONLY, 0)      # "Hips" is the root: joint 0 of any skeleton
    parts, off, al = [], 0, alignment
    for mp in mps:
        L = mp.get_n_spatial_components()
        batch = _Batch(mp._prim, S[:, off:off + L], hip_sk, al)
        try:
            d_f, T = batch.frames(None)
            parts.append(mp._prim.ctx.download(d_f, (T, D), np.float64))
        finally:
            batch.close()
        off += L
        al = sk.alignment_to(parts[-1][-1], joint)
    ref = np.concatenate(parts)[None]
    got, _ = run(mps, S, alignment, hip_sk, stride=ref.shape[1])
    assert_close(got, ref)


# ---- 5. batch invariance, determinism ---------------------------------------------------------------------------------
def test_a_walk_does_not_depend_on_the_batch_and_calls_repeat(pset):
    steps, S, alignment, hip_sk, _, _ = walk_case("previous", "Spine", n_walks=7)
    mps = mps_of(pset, SEQUENCE)
    all7, x7 = run(mps, S, alignment, hip_sk)
    again, xa = run(mps, S, alignment, hip_sk)
    assert np.array_equal(all7, again, equal_nan=True) and np.array_equal(x7, xa)
    for w in (0, 3, 6):
        alone, x1 = run(mps, S[w:w + 1], alignment, hip_sk)
        assert np.array_equal(alone[0], all7[w], equal_nan=True) and np.array_equal(x1[0], x7[w])


# ---- 6. shape boundaries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [1, 2, _capi.MG_WALK_MAX_STEPS])
def test_step_counts_up_to_the_call_limit(pset, n_steps):
    seq = [(0, 2)[i % 2] for i in range(n_steps)]      # 12 and 20 frames
    steps, S, alignment, _, _, _ = walk_case("previous", "Hips", n_walks=2, sequence=seq)
    ref, _, ref_x = gw.assemble_walk_host(steps, S, alignment=alignment)
    got, got_x = run(mps_of(pset, seq), S, alignment, stride=ref.shape[1])
    assert_close(got, ref)
    assert float(np.max(np.abs(got_x - ref_x))) / root_scale(ref) <= WALK_TOLERANCE


def test_a_walk_one_step_past_the_limit_is_joined_from_pieces(pset):
    seq = [(0, 2)[i % 2] for i in range(_capi.MG_WALK_MAX_STEPS + 1)]
    steps, S, _, _, _, _ = walk_case("start_pose", "Hips", n_walks=1, sequence=seq)
    graph = _Graph(pset)
    walk = gw.HipGraphWalk(graph, start_pose=START_POSE)
    off = 0
    for k in seq:
        L = SHAPES[k][0]
        walk.steps.append(gw.HipGraphWalkStep.from_graph(graph, ("walk", "w%d" % k), S[0, off:off + L]))
        off += L
    walk.convert_graph_walk_to_quaternion_frames()
    ref, offsets, _ = gw.assemble_walk_host(steps, S, alignment=gw.alignment_from_start_pose(START_POSE))
    assert_close(walk.get_quat_frames()[None], ref)
    assert [s.start_frame for s in walk.steps] == offsets[0, :-1].tolist() and walk.steps[-1].end_frame == offsets[0, -1] - 1
    # the batch form joins pieces the same way
    frames, offs = gw.assemble_walks(graph, [("walk", "w%d" % k) for k in seq], S, alignment=gw.alignment_from_start_pose(START_POSE))
    assert np.array_equal(offs, offsets) and np.array_equal(frames[0], walk.get_quat_frames())
    walk.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lengths_around_the_tile_and_a_primitive_used_twice(pset, dtype):
    seq = ["t31", "t32", 1, "t31", 0]                  # 31, 32, 33, 31, 12 frames
    mps = mps_of(pset, seq)
    rng = np.random.default_rng(21)
    S = (0.7 * rng.standard_normal((3, sum(mp.get_n_spatial_components() for mp in mps)))).astype(dtype)
    jsons = {d["name"]: d for d in primitive_jsons()}
    for mp in mps:
        jsons.setdefault(mp.name, mp)
    al = gw._ROOT_ONLY.alignment_to(np.concatenate(([10.0, 90.0, -30.0, 0.9, 0.1, 0.4, -0.1], np.tile([1.0, 0.0, 0.0, 0.0], 1))))
    ref, _, _ = gw.assemble_walk_host([jsons[mp.name] for mp in mps], S.astype(np.float64), alignment=al)
    got, _ = run(mps, S, al, stride=ref.shape[1] + 5)
    assert_close(got[:, :ref.shape[1]], ref)
    assert np.isnan(got[:, ref.shape[1]:]).all()        # the sentinel behind the walk's end is untouched


def test_given_times_lengths_of_one_and_ragged_rows(pset):
    """lengths tile - 1, tile, tile + 1 and 1 from given times; rows between a walk's end and walk_stride keep the NaN sentinel"""
    seq = [1, 0, 1, 2]
    mps = mps_of(pset, seq)
    rng = np.random.default_rng(8)
    steps, S, alignment, _, _, _ = walk_case("previous", "Hips", n_walks=3, sequence=seq)
    lengths = np.array([[TILE - 1, 1, TILE + 1, TILE], [TILE, TILE + 1, 1, 5], [1, 1, 1, 1]], dtype=np.int32)
    cap = TILE + 1
    times = np.zeros((3, 4, cap))
    for w in range(3):
        for i, mp in enumerate(mps):
            times[w, i, :lengths[w, i]] = np.sort(rng.uniform(0.0, mp.n_canonical_frames, lengths[w, i]))
    offsets = np.zeros((3, 4), dtype=np.int64)
    offsets[:, 1:] = np.cumsum(lengths, axis=1)[:, :-1]
    ref, _, _ = gw.assemble_walk_host(steps, S, times=[[times[w, i, :lengths[w, i]] for i in range(4)] for w in range(3)], alignment=alignment)
    got, _ = run(mps, S, alignment, times=times, lengths=lengths, frame_offset=offsets, stride=ref.shape[1] + 2)
    assert_close(got[:, :ref.shape[1]], ref)
    assert np.isnan(got[:, ref.shape[1]:]).all()


def test_time_parameters_give_ragged_walks(pset):
    """lengths from mg_time_function_sample on a primitive with a time model, mixed with a primitive without one"""
    graph = _Graph(pset)
    keys = [("walk", "timed"), ("walk", "w0"), ("walk", "timed")]
    mps = [graph.nodes[k] for k in keys]
    rng = np.random.default_rng(4)
    S = 0.7 * rng.standard_normal((4, 4 + 5 + 4))
    G = 3.0 * rng.standard_normal((4, 2 + 0 + 2))
    frames, offsets = gw.assemble_walks(graph, keys, S, time_parameters=G)
    timed = pset.nodes["timed"]
    times = []
    for w in range(4):
        rows = []
        for i, g in ((0, G[w, 0:2]), (2, G[w, 2:4])):
            t, ln = timed._prim.time_function_sample(g[None, :])
            rows.append(t[0, :ln[0]])
        times.append([rows[0], None, rows[1]])
    lengths = np.array([[len(t[0]), 12, len(t[2])] for t in times])
    assert len(set(lengths[:, 0])) > 1                 # ragged across the walks
    assert np.array_equal(np.diff(offsets, axis=1), lengths)
    jsons = {d["name"]: d for d in primitive_jsons()}
    ref, _, _ = gw.assemble_walk_host([timed, jsons["w0"], timed], S, latent_offset=[0, 4, 9], times=times)
    assert_close(frames, ref)


# ---- 7. errors before any launch --------------------------------------------------------------------------------------
def test_bad_calls_are_refused(pset):
    mps = mps_of(pset, [0, 1])
    S = np.zeros((2, 13))
    other = synthetic.make_primitive(seed=5, n_components=3, n_frames=12, n_basis=6, n_dim=15, n_gmm=2, name="wide")
    wide = HipPrimitiveSet([other]).nodes["wide"]
    cases = []
    cases.append(("has n_dim", dict(mps=[mps[0], wide], S=np.zeros((2, 8)))))                                            # mismatched n_dim
    t = np.zeros((2, 2, 40))
    ln = np.array([[12, 33], [12, 33]], dtype=np.int32)
    cases.append(("steps overlap", dict(mps=mps, S=S, times=t, lengths=ln, frame_offset=np.array([[0, 11], [0, 12]]), stride=50)))   # overlapping steps
    cases.append(("walk_stride is", dict(mps=mps, S=S, times=t, lengths=ln, frame_offset=np.array([[0, 12], [0, 18]]), stride=50)))   # past walk_stride
    cases.append(("has length 0", dict(mps=mps, S=S, times=t, lengths=np.array([[12, 0], [12, 33]], dtype=np.int32), frame_offset=np.array([[0, 12], [0, 12]]), stride=50)))
    cases.append(("walk_stride is 44", dict(mps=mps, S=S, stride=44)))                                                            # canonical grids need 45 rows
    other_ctx = HipPrimitiveSet(primitive_jsons()[:1], context=_capi.Context(0))
    cases.append(("another context", dict(mps=[mps[0], other_ctx.nodes["w0"]], S=np.zeros((2, 10)))))                           # two contexts
    joints, animated = synthetic.make_skeleton(2)
    al = _capi.Skeleton(joints, animated).alignment_to(np.concatenate(([0.0, 0.0, 0.0], np.tile([1.0, 0.0, 0.0, 0.0], 2))), "Spine")
    cases.append(("a skeleton is needed", dict(mps=mps, S=S, alignment=al)))                                                         # a non-root aligning joint, no skeleton
    for text, kw in cases:                            # the status and, in mg_last_error's text, the check that fired
        with pytest.raises(_capi.MGError) as e:
            run(**kw)
        assert e.value.status == _capi.MG_ERR_INVALID_ARGUMENT and text in str(e.value), (text, str(e.value))
    with pytest.raises(_capi.MGError, match="65 steps"):
        run(mps_of(pset, [0] * (_capi.MG_WALK_MAX_STEPS + 1)), np.zeros((1, 5 * (_capi.MG_WALK_MAX_STEPS + 1))))
    got, _ = run(mps, S)                              # the context still works
    assert not np.isnan(got[:, :45]).any()


# ---- 8. HipGraphWalk end to end -------------------------------------------------------------------------------------------
class _Constraints(object):
    def __init__(self, name):
        self.motion_primitive_name, self.constraints, self.min_error, self.evaluations = name, [], None, 0


def test_graph_walk_end_to_end(pset):
    graph = _Graph(pset)
    config = {"n_random_samples": 8, "use_constraints": False, "local_optimization_settings": {"start_error_threshold": 0.0, "error_scale_factor": 1.0,
              "quality_scale_factor": 1.0, "method": "leastsq", "max_iterations": 10}}
    gen = HipMotionPrimitiveGenerator(graph.nodes, config, "walk")
    np.random.seed(12)
    walk = gw.HipGraphWalk(graph, start_pose=START_POSE)
    for name in ("w0", "w1", "w2", "w1"):
        spline, parameters = gen.generate_constrained_motion_spline(_Constraints(name), walk)
        key = ("walk", name)
        start = walk.get_num_of_frames()
        walk.append_quat_frames(spline.get_motion_vector())
        walk.steps.append(gw.HipGraphWalkStep.from_graph(graph, key, np.ravel(parameters), start, walk.get_num_of_frames() - 1))
    appended = walk.get_quat_frames().copy()
    ranges = [(s.start_frame, s.end_frame) for s in walk.steps]
    walk.convert_graph_walk_to_quaternion_frames()
    assert [(s.start_frame, s.end_frame) for s in walk.steps] == ranges
    assert_close(walk.get_quat_frames()[None], appended[None])
    # new latents for the last two steps, rebuilt from step 2: the first two steps' rows keep their bits
    before = walk.get_quat_frames().copy()
    cut = walk.steps[2].start_frame
    new = np.array(walk.get_global_spatial_parameter_vector(2)) + 0.2
    walk.update_spatial_parameters(new, start_step=2)
    walk.convert_graph_walk_to_quaternion_frames(start_step=2)
    after = walk.get_quat_frames()
    assert np.array_equal(after[:cut], before[:cut]) and not np.allclose(after[cut:], before[cut:])
    fresh = gw.HipGraphWalk(graph, start_pose=START_POSE)
    fresh.steps = [gw.HipGraphWalkStep.from_graph(graph, s.node_key, s.parameters) for s in walk.steps]
    fresh.convert_graph_walk_to_quaternion_frames()
    assert_close(after[None], fresh.get_quat_frames()[None])
    walk.close()
    fresh.close()
