"""The device spatial alignment and frame preparation (mg_align_motions_spatially, mg_prepare_aligned_frames,
morphablegraphs_amd.spatial_alignment) against their host restatements, and HipMotionModelConstructor against the loose chain
of stage functions.

Root channels: within 4 ulp of the host restatement (a square root and a division may differ by one ulp each between libm and
the device); every other channel in bits.  The frame preparation is compared in bits."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_spatial_alignment_host import GOLDEN, PREPARE, align_set, prepare_case, random_motion, same_bits, turned_and_moved  # noqa: E402
from test_dtw_host import end_to_end  # noqa: E402

from morphablegraphs_amd import _capi, dtw, fpca, spatial_alignment as sa  # noqa: E402
from morphablegraphs_amd.motion_model_constructor import HipMotionModelConstructor  # noqa: E402

pytestmark = pytest.mark.gpu
WG = _capi.MG_SPATIAL_ALIGN_FRAMES_PER_WORKGROUP
ULPS = 4


@pytest.fixture(scope="module")
def ctx():
    from morphablegraphs_amd.motion_primitive import get_context
    return get_context(0)


def ulps_apart(a, b):
    """The largest |a - b| in units of the spacing of the larger magnitude (0 where both are equal)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.spacing(np.maximum(np.maximum(np.abs(a), np.abs(b)), np.finfo(np.float64).tiny))))


def check_against_host(ctx, motions, frame_idx, ref, what):
    """Device against host: root channels to 4 ulp, the rest in bits, the transforms to 4 ulp; two calls give identical bits,
    and a motion alone gives the bits it gives in the batch."""
    host, host_t = sa.align_motions_spatially_host(motions, frame_idx, ref, return_transforms=True)
    dev, dev_t = sa.align_motions_spatially(motions, frame_idx, ref, ctx=ctx, return_transforms=True)
    again = sa.align_motions_spatially(motions, frame_idx, ref, ctx=ctx)
    assert isinstance(dev, collections.OrderedDict) and list(dev.keys()) == list(motions.keys())
    worst = ulps_apart(dev_t, host_t)
    for key, m in motions.items():
        worst = max(worst, ulps_apart(dev[key][:, :7], host[key][:, :7]))
        assert same_bits(dev[key][:, 7:], np.asarray(m)[:, 7:]), (what, key)
        assert same_bits(again[key], dev[key]), (what, key)
        assert np.all(dev[key][frame_idx, :3] == 0.0)
    print("%s: root channels and transforms at most %.3g ulp from the host restatement" % (what, worst))
    assert worst <= ULPS, (what, worst)
    if len(motions) > 1:
        for i, key in enumerate(motions.keys()):
            alone, alone_t = sa.align_motions_spatially({key: motions[key]}, frame_idx, ref, ctx=ctx, return_transforms=True)
            assert same_bits(alone[key], dev[key]) and same_bits(alone_t[0], dev_t[i]), (what, key)
    return dev


@pytest.mark.parametrize("s", range(int(GOLDEN["a_n_sets"])))
def test_golden_inputs(ctx, s):
    motions, cases, ref = align_set(s)
    check_against_host(ctx, motions, 0, ref, str(GOLDEN["a%d_name" % s]))


SHAPES = [(1, [1]), (1, [2, WG - 1, WG + 1]), (19, [WG, 2, WG + 1]), (19, [WG - 1]), (63, [5, 2 * WG + 3, WG]), (64, [WG + 1, 1, 2 * WG])]


@pytest.mark.parametrize("n_joints,lengths", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_seeded_shapes(ctx, n_joints, lengths):
    rng = np.random.default_rng(100 * n_joints + len(lengths))
    motions = collections.OrderedDict(("k%d" % i, random_motion(rng, n, n_joints)) for i, n in enumerate(lengths))
    for frame_idx in sorted({0, min(lengths) - 1}):
        for ref in ((0.0, -1.0), (0.6, 1.7)):
            check_against_host(ctx, motions, frame_idx, ref, "J %d lengths %r frame %d ref %r" % (n_joints, lengths, frame_idx, ref))


def test_special_headings_and_a_quaternion_of_norm_three(ctx):
    """The heading already the reference, opposite to it (cos = -1), at +-90 degrees; the root quaternions have norm 3."""
    motions = collections.OrderedDict()
    for name, yaw in (("same", np.pi), ("opposite", 0.0), ("plus90", np.pi / 2), ("minus90", -np.pi / 2)):
        f = np.zeros((3, 11))
        f[:, :3] = [[1.0, 2.0, 3.0], [2.0, 2.5, 5.0], [-1.0, 0.0, 4.0]]
        f[:, 3:7] = 3.0 * np.array([np.cos(yaw / 2), 0.0, np.sin(yaw / 2), 0.0])
        f[:, 7:] = [0.5, -0.5, 0.5, 0.5]
        motions[name] = f
    dev = check_against_host(ctx, motions, 0, (0.0, -1.0), "special headings")
    _, t = sa.align_motions_spatially(motions, ctx=ctx, return_transforms=True)
    assert t[1, 0] == -1.0 and t[1, 1] == 0.0 and abs(t[0, 0] - 1.0) <= 1e-15 and abs(t[2, 0]) <= 1e-15 and abs(t[3, 0]) <= 1e-15
    for key in motions:
        assert np.all(np.isfinite(dev[key])) and np.max(np.abs(np.linalg.norm(dev[key][:, 3:7], axis=1) - 1.0)) <= 1e-12
        assert np.all(dev[key][:, 3] >= 0.0)


def status_of(call):
    with pytest.raises(_capi.MGError) as ei:
        call()
    return ei.value.status


def test_limits_and_misuse(ctx):
    """Each refusal by its status code, with nothing written and no HIP error left behind: the good call at the end succeeds."""
    rng = np.random.default_rng(9)
    good = random_motion(rng, 9, 2)
    sentinel = np.full((9 * 11,), -77.0)
    off = np.array([0, 4, 9], dtype=np.int64)
    ref = np.array([0.0, -1.0])
    with ctx.buffers() as bufs:
        out = bufs.upload(sentinel)
        t_dev = bufs.upload(np.full((10,), -77.0))

        def call(frames, n_dim=11, offsets=off, frame_idx=0):
            f_dev = bufs.upload(frames)
            _capi.align_motions_spatially(ctx, f_dev, offsets, n_dim, frame_idx, ref, out, t_dev)

        def untouched():
            return np.all(ctx.download(out, sentinel.shape, np.float64) == -77.0) and np.all(ctx.download(t_dev, (10,), np.float64) == -77.0)

        assert status_of(lambda: call(good, n_dim=8)) == _capi.MG_ERR_UNSUPPORTED
        assert status_of(lambda: call(good, n_dim=3 + 4 * 65)) == _capi.MG_ERR_UNSUPPORTED
        assert status_of(lambda: call(good, n_dim=3)) == _capi.MG_ERR_UNSUPPORTED
        assert status_of(lambda: call(good, offsets=np.array([1, 4, 9], dtype=np.int64))) == _capi.MG_ERR_INVALID_ARGUMENT
        assert status_of(lambda: call(good, offsets=np.array([0, 4, 4], dtype=np.int64))) == _capi.MG_ERR_INVALID_ARGUMENT
        assert status_of(lambda: call(good, frame_idx=4)) == _capi.MG_ERR_INVALID_ARGUMENT       # motion 0 has 4 frames
        assert status_of(lambda: call(good, frame_idx=-1)) == _capi.MG_ERR_INVALID_ARGUMENT
        nan = good.copy()
        nan[8, 10] = np.nan
        assert status_of(lambda: call(nan)) == _capi.MG_ERR_INVALID_ARGUMENT
        zero = good.copy()
        zero[6, 3:7] = 0.0
        assert status_of(lambda: call(zero)) == _capi.MG_ERR_INVALID_ARGUMENT
        up = good.copy()
        up[4, 3:7] = [1.0, 1.0, 1.0, -1.0]       # frame 0 of motion 1: z goes onto y, every statement exact
        with pytest.raises(_capi.MGError, match="motion 1") as ei:
            call(up)
        assert ei.value.status == _capi.MG_ERR_INVALID_ARGUMENT
        with pytest.raises(ValueError):
            _capi.align_motions_spatially(ctx, out, off, 11, 0, [0.0, -1.0, 0.0], out, None)
        assert status_of(lambda: _capi.align_motions_spatially(ctx, out, off, 11, 0, [0.0, 0.0], t_dev, None)) == _capi.MG_ERR_INVALID_ARGUMENT
        assert untouched()
        _capi.align_motions_spatially(ctx, out, np.array([0], dtype=np.int64), 11, 0, ref, out, None)       # no motions: MG_OK, nothing to do
        assert untouched()
        call(good)
        got = ctx.download(out, (9, 11), np.float64)
    host = sa.align_motions_spatially_host({"a": good[:4], "b": good[4:]})
    assert ulps_apart(got[:, :7], np.concatenate([host["a"], host["b"]])[:, :7]) <= ULPS
    with pytest.raises(ValueError):
        sa.align_motions_spatially({"m": np.zeros((3, 8))}, ctx=ctx)
    assert sa.align_motions_spatially({}, ctx=ctx) == collections.OrderedDict()


# ---- mg_prepare_aligned_frames -------------------------------------------------------------------------------------------------
def check_prepare(ctx, table, n_joints=None, what=""):
    motions = collections.OrderedDict(("m%d" % i, table[i]) for i in range(len(table)))
    host, host_scale = sa.prepare_aligned_frames_host(motions, n_joints)
    dev, dev_scale = sa.prepare_aligned_frames(motions, n_joints, ctx=ctx)
    again, _ = sa.prepare_aligned_frames(motions, n_joints, ctx=ctx)
    assert list(dev.keys()) == list(motions.keys())
    for key in motions:
        assert same_bits(dev[key], host[key]), (what, key)
        assert same_bits(again[key], dev[key]), (what, key)
    assert same_bits(dev_scale, host_scale), (what, dev_scale, host_scale)
    return dev, dev_scale


def prepare_table(rng, shape):
    x = rng.standard_normal(shape)
    q = x[:, :, 3:].reshape(shape[0], shape[1], -1, 4)
    q /= np.linalg.norm(q, axis=3, keepdims=True)
    return x


@pytest.mark.parametrize("s", PREPARE)
def test_prepare_golden_inputs(ctx, s):
    c = prepare_case(s)
    dev, scale = check_prepare(ctx, c["in"], c["n_joints"], c["name"])
    assert same_bits(np.array(list(dev.values())), c["out"]) and same_bits(scale, c["scale"])


@pytest.mark.parametrize("shape", [(1, 1, 7), (3, 17, 79), (2, 257, 259)], ids=str)
def test_prepare_seeded_shapes(ctx, shape):
    rng = np.random.default_rng(sum(shape))
    x = prepare_table(rng, shape)
    check_prepare(ctx, x, what="plain %r" % (shape,))
    # the maximum in the last frame of the last motion, with a negative sign
    y = x.copy()
    y[-1, -1, 2] = -9.25
    _, scale = check_prepare(ctx, y, what="negative maximum %r" % (shape,))
    assert scale[2] == 9.25
    # one root channel zero everywhere: nothing scaled, scale = ones
    z = x.copy()
    z[:, :, 1] = 0.0
    dev, scale = check_prepare(ctx, z, what="zero channel %r" % (shape,))
    assert np.all(scale == 1.0) and same_bits(np.array(list(dev.values()))[:, :, :3], z[:, :, :3])
    # a joint whose quaternion is the exact negative of the reference frame's
    w = x.copy()
    w[-1, -1, 3:7] = -w[0, 0, 3:7]
    dev, _ = check_prepare(ctx, w, what="exact negative %r" % (shape,))
    assert same_bits(dev["m%d" % (shape[0] - 1)][-1, 3:7], w[0, 0, 3:7])
    # fewer animated joints than quaternion slots: the rest is copied
    if shape[2] > 7:
        dev, _ = check_prepare(ctx, x, n_joints=1, what="one joint %r" % (shape,))
        assert same_bits(np.array(list(dev.values()))[:, :, 7:], x[:, :, 7:])


def test_prepare_misuse(ctx):
    with ctx.buffers() as bufs:
        x = np.ones((2, 3, 11))
        f_dev, o_dev = bufs.upload(x), bufs.upload(np.full(x.shape, -77.0))
        assert status_of(lambda: _capi.prepare_aligned_frames(ctx, f_dev, 2, 3, 11, 3, o_dev)) == _capi.MG_ERR_INVALID_ARGUMENT
        assert status_of(lambda: _capi.prepare_aligned_frames(ctx, f_dev, 2, 0, 11, 2, o_dev)) == _capi.MG_ERR_INVALID_ARGUMENT
        x[1, 2, 5] = np.inf
        b_dev = bufs.upload(x)
        assert status_of(lambda: _capi.prepare_aligned_frames(ctx, b_dev, 2, 3, 11, 2, o_dev)) == _capi.MG_ERR_INVALID_ARGUMENT
        assert np.all(ctx.download(o_dev, x.shape, np.float64) == -77.0)
        assert np.all(_capi.prepare_aligned_frames(ctx, f_dev, 0, 3, 11, 2, o_dev) == 1.0)
        _capi.prepare_aligned_frames(ctx, f_dev, 2, 3, 11, 2, o_dev)
        assert np.all(ctx.download(o_dev, x.shape, np.float64) == 1.0)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
CONFIG = {"n_spatial_basis_factor": 0.25, "n_components": None, "fraction": 0.95, "n_basis_functions_temporal": 8, "npc_temporal": None,
          "precision_temporal": 0.99}


class _OneGaussian(object):
    """A stand-in trainer (six motions are too few for the AIC sweep): one component with a diagonal covariance."""

    def fit(self, data):
        self.data = np.array(data)

    def convert_model_to_json(self):
        return {'gmm_weights': [1.0], 'gmm_means': [self.data.mean(axis=0).tolist()], 'gmm_covars': [np.diag(self.data.var(axis=0) + 1e-6).tolist()]}


@pytest.fixture(scope="module")
def captures():
    """The six motions of dtw.npz's end-to-end case (30 to 44 frames, a 7-joint skeleton), each turned about y and moved by a
    seeded transform: captures as they come, not yet aligned."""
    joints, animated, keys, motions = end_to_end()
    rng = np.random.default_rng(31)
    moved = collections.OrderedDict((k, turned_and_moved(m, rng.uniform(-np.pi, np.pi), rng.uniform(-4.0, 4.0, 3))) for k, m in motions.items())
    assert sorted(len(m) for m in moved.values())[0] >= 30 and sorted(len(m) for m in moved.values())[-1] <= 44 and len(moved) == 6
    return _capi.Skeleton(joints, animated), [j[0] for j in joints], animated, moved


def same_model(a, b):
    """Two model dicts, equal in every entry; arrays (nested lists of floats) in bits."""
    assert type(a) is type(b), (type(a), type(b))
    if isinstance(a, dict):
        assert list(a.keys()) == list(b.keys())
        for k in a:
            same_model(a[k], b[k])
    elif isinstance(a, (list, tuple, np.ndarray)) and len(a) and not isinstance(a[0], str):
        assert same_bits(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    else:
        assert a == b, (a, b)


def loose_chain(ctx, sk, names, animated, motions, version, sections=None, keyframes=None):
    aligned = sa.align_motions_spatially(motions, ctx=ctx)
    warped, warps = dtw.align_frames_temporally(sk, names, aligned, sections=sections, ctx=ctx)
    data = fpca.construct_motion_primitive_model(warped, warps, CONFIG, animated_joints=animated, name="walk", version=version, keyframes=keyframes,
                                                 frame_time=1.0 / 30, gmm_trainer=_OneGaussian(), ctx=ctx)
    return data, warped, warps


def constructor_for(ctx, sk, names):
    return HipMotionModelConstructor(sk, CONFIG, joints=names, ctx=ctx, frame_time=1.0 / 30, gmm_trainer=_OneGaussian())


def test_construct_model_equals_the_loose_chain(ctx, captures):
    from morphablegraphs_amd.motion_primitive import HipMotionPrimitive
    sk, names, animated, motions = captures
    expected, warped, warps = loose_chain(ctx, sk, names, animated, motions, 1)
    c = constructor_for(ctx, sk, names)
    c.set_motions(motions)
    data = c.construct_model("walk", version=1)
    same_model(data, expected)
    assert list(c._aligned_frames.keys()) == list(motions.keys()) and c._aligned_dev is None
    for k in motions:
        assert same_bits(c._aligned_frames[k], warped[k]) and c._temporal_data[k] == warps[k]
    prim = HipMotionPrimitive(context=ctx)
    prim._initialize_from_json(data)
    assert data["n_canonical_frames"] == len(warped[list(motions.keys())[0]]) and prim.get_n_spatial_components() == len(data["eigen_vectors_spatial"])
    assert c.back_project_sample(np.zeros(len(data["eigen_vectors_spatial"]))).shape == (data["n_basis_spatial"], 11)
    # the aligned data handed over instead of the captures
    again = constructor_for(ctx, sk, names)
    again.set_aligned_frames(warped)
    again.set_timewarping(warps)
    same_model(again.construct_model("walk", version=1, align_frames=False), expected)
    # the reference motion by the least mean cost
    picked = HipMotionModelConstructor(sk, CONFIG, joints=names, ctx=ctx, frame_time=1.0 / 30, gmm_trainer=_OneGaussian(), reference_selection="least_mean_cost")
    picked.set_motions(motions)
    aligned = sa.align_motions_spatially(motions, ctx=ctx)
    w2, f2 = dtw.align_frames_temporally(sk, names, aligned, ctx=ctx, reference_selection="least_mean_cost")
    same_model(picked.construct_model("walk"), fpca.construct_motion_primitive_model(w2, f2, CONFIG, animated_joints=animated, name="walk", frame_time=1.0 / 30,
                                                                                     gmm_trainer=_OneGaussian(), ctx=ctx))


def test_construct_model_with_sections_and_version_3(ctx, captures):
    sk, names, animated, motions = captures
    sections = {k: [{"start_idx": 0, "end_idx": len(m) // 2}, {"start_idx": len(m) // 2, "end_idx": len(m)}] for k, m in motions.items()}
    mean_key = dtw.get_average_time_line(motions)
    keyframes = {"contact%d" % i: s["end_idx"] for i, s in enumerate(sections[mean_key])}
    for version in (1, 3):
        expected, _, _ = loose_chain(ctx, sk, names, animated, motions, version, sections=sections, keyframes=keyframes)
        c = constructor_for(ctx, sk, names)
        c.set_motions(motions)
        c.set_dtw_sections(sections)
        data = c.construct_model("walk", version=version)
        same_model(data, expected)
        assert data["keyframes"] == keyframes and len(keyframes) == 2
    assert data["sspm"]["animated_joints"] == animated and data["tspm"]["frame_time"] == 1.0 / 30
    with_skeleton = HipMotionModelConstructor(sk, CONFIG, joints=names, ctx=ctx, gmm_trainer=_OneGaussian(), skeleton_json={"root": "Hips"})
    with_skeleton.set_motions(motions)
    assert with_skeleton.construct_model("walk", version=3, save_skeleton=True)["skeleton"] == {"root": "Hips"}
