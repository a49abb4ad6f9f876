"""mg_point_cloud_features (csrc/mg_point_clouds.hip) bit for bit against the host route of the "euclidean_pca" features --
back_project_frames_f64, then ctx.joint_positions, then HipClusterTreeSampler.map_motions_to_euclidean_space -- across the joint counts
around the eight-joints-per-request boundary of mg_joint_tracks and the cap, the root and the longest chain, the channel counts, the
frame counts and steps, the batch sizes around a workgroup's candidates, both latent dtypes, a shape behind the large-LDS opt-in, and
every misuse with its code and no launch."""
import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd.cluster_tree_sampling import HipClusterTreeSampler, point_clouds_host

pytestmark = pytest.mark.gpu

MG_MAX_CHAIN = 32
MAX_JOINTS = _capi.MG_FEATURE_POINTS_MAX_JOINTS if hasattr(_capi, "MG_FEATURE_POINTS_MAX_JOINTS") else 32


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


class _MP(object):
    """What the sampler reads of a motion primitive, around a _capi.Primitive."""

    def __init__(self, prim):
        self._prim = prim

    def get_n_canonical_frames(self):
        return self._prim.n_canonical_frames


def chain_skeleton(n_animated, length=MG_MAX_CHAIN + 2):
    """j0 - j1 - ... one chain of `length` joints with seeded offsets, the first n_animated animated: joint k sits k links from the root."""
    rng = np.random.default_rng(2)
    joints = [("j%d" % k, None if k == 0 else "j%d" % (k - 1), tuple(float(v) for v in (rng.standard_normal(3) * 5.0 if k else np.zeros(3)))) for k in range(length)]
    return _capi.Skeleton(joints, ["j%d" % k for k in range(n_animated)])


_PRIMS = {}


def primitive(ctx, F, D, NB=None, L=5):
    key = (id(ctx), F, D, NB, L)
    if key not in _PRIMS:
        nb = NB if NB is not None else max(4, int(0.2 * F))
        data = synthetic.make_primitive(seed=F + D, n_components=L, n_frames=F, n_basis=nb, n_dim=D, n_gmm=2, name="pc_%d_%d_%d" % (F, D, nb))
        _PRIMS[key] = _capi.Primitive(ctx, data)
    return _PRIMS[key]


def latents(prim, n, dtype=np.float64, pad=0, seed=1):
    S = 0.7 * np.random.default_rng(seed).standard_normal((n, prim.n_components + pad))
    return S.astype(dtype)


def host_route(prim, S, sk, joints, step):
    """_back_project (the integer canonical frames), then map_motions_to_euclidean_space."""
    sampler = HipClusterTreeSampler()
    return sampler.map_motions_to_euclidean_space(_MP(prim), sampler._back_project(_MP(prim), S), sk, joints, step)


def device_route(prim, S, sk, joints, step):
    n, F, idx = len(S), prim.n_canonical_frames, sk.indices(joints)
    grid = prim.time_grid(np.arange(F, dtype=np.float64))
    try:
        with prim.ctx.buffers() as bufs:
            d_S, d_o = bufs.upload(S), bufs.malloc(8 * n * F * len(idx) * 3)
            _capi.point_cloud_features_dev(prim, grid, sk, idx, step, d_S, S.dtype, n, S.shape[1], d_o)
            return prim.ctx.download(d_o, (n, F * len(idx) * 3), np.float64)
    finally:
        grid.close()


def same_bits(prim, S, sk, joints, step):
    got, want = device_route(prim, S, sk, joints, step), host_route(prim, S, sk, joints, step)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "largest difference %.3g" % float(np.abs(got - want).max())
    return got


@pytest.mark.parametrize("J", [1, 8, 9, 10, MAX_JOINTS])
def test_joint_counts_around_the_request_boundary_and_the_cap(ctx, J):
    prim, sk = primitive(ctx, 5, 79), chain_skeleton(19)
    joints = ["j%d" % (J - 1 - k) for k in range(J)]                             # chains of J - 1 .. 0 links, the longest first
    same_bits(prim, latents(prim, 17), sk, joints, 1)


def test_the_root_and_the_end_of_the_longest_chain(ctx):
    prim, sk = primitive(ctx, 5, 79), chain_skeleton(19)
    got = same_bits(prim, latents(prim, 3), sk, ["j0", "j%d" % MG_MAX_CHAIN], 2)
    frames = HipClusterTreeSampler()._back_project(_MP(prim), latents(prim, 3))
    np.testing.assert_array_equal(got.reshape(3, 5, 2, 3)[:, 0, 0], frames[:, 0, :3])   # the root's position is the root translation


@pytest.mark.parametrize("D", [7, 79])
def test_channel_counts(ctx, D):
    prim, sk = primitive(ctx, 5, D), chain_skeleton((D - 3) // 4)
    same_bits(prim, latents(prim, 6), sk, ["j0", "j1", "j7"], 1)


@pytest.mark.parametrize("F", [4, 5, 64, 65])
def test_frame_counts_and_steps(ctx, F):
    prim, sk = primitive(ctx, F, 79), _capi.Skeleton(*synthetic.make_skeleton(19))
    S = latents(prim, 5)
    for step in (1, 3, 4, F + 1):
        got = same_bits(prim, S, sk, ["LeftHand_EndSite", "Hips", "RightFoot"], step)
        every = device_route(prim, S, sk, ["LeftHand_EndSite", "Hips", "RightFoot"], 1)
        np.testing.assert_array_equal(got, point_clouds_host(every.reshape(5, F, 3, 3), step))    # the layout rule, stated in NumPy


@pytest.mark.parametrize("n", [1, 15, 16, 17, 257])
def test_batch_sizes(ctx, n):
    prim, sk = primitive(ctx, 5, 79), _capi.Skeleton(*synthetic.make_skeleton(19))
    same_bits(prim, latents(prim, n), sk, ["LeftHand", "RightFoot"], 3)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_latent_dtypes_with_a_wider_row(ctx, dtype):
    prim, sk = primitive(ctx, 5, 79), _capi.Skeleton(*synthetic.make_skeleton(19))
    same_bits(prim, latents(prim, 9, dtype, pad=3), sk, ["LeftHand", "Head_EndSite"], 1)


def test_a_shape_that_needs_the_large_lds_opt_in(ctx):
    """32 basis functions x 79 channels x 4 candidates: 81 KB of control points, past the 64 KB a kernel gets without the opt-in."""
    prim, sk = primitive(ctx, 40, 79, NB=32), _capi.Skeleton(*synthetic.make_skeleton(19))
    ends = ["LeftHand_EndSite", "RightHand_EndSite", "Head_EndSite", "LeftFoot", "RightFoot"]      # their chains read every channel
    same_bits(prim, latents(prim, 6), sk, ends, 4)


def test_the_sampler_returns_the_host_routes_array_on_the_device(ctx):
    prim, sk = primitive(ctx, 5, 79), _capi.Skeleton(*synthetic.make_skeleton(19))
    S, names = latents(prim, 10), ["LeftHand", "Hips"]
    buf = HipClusterTreeSampler().point_clouds_on_device(_MP(prim), S, sk, names, step=2)
    try:
        got = ctx.download(buf, (10, 5 * 2 * 3), np.float64)
    finally:
        buf.free()
    np.testing.assert_array_equal(got, host_route(prim, S, sk, names, 2))


def test_misuse_returns_its_code_and_launches_nothing(ctx):
    prim, sk, chain = primitive(ctx, 5, 79), _capi.Skeleton(*synthetic.make_skeleton(19)), chain_skeleton(19)
    S = latents(prim, 4)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        with ctx.buffers() as bufs:
            d_S, d_o = bufs.upload(S), bufs.malloc(8 * 4 * 5 * 2 * 3)

            def call(p=prim, skel=sk, idx=sk.indices(["LeftHand", "Hips"]), step=1, lat=d_S, n=4, ld=S.shape[1], out=d_o):
                _capi.point_cloud_features_dev(p, None, skel, idx, step, lat, np.float64, n, ld, out)      # (the canonical grid)

            def status(**kw):
                with pytest.raises(_capi.MGError) as e:
                    call(**kw)
                return e.value.status

            bad, unsupported = _capi.MG_ERR_INVALID_ARGUMENT, _capi.MG_ERR_UNSUPPORTED
            assert status(idx=np.array([99], dtype=np.int32)) == bad
            assert status(idx=np.array([-1], dtype=np.int32)) == bad
            assert status(idx=np.zeros(MAX_JOINTS + 1, dtype=np.int32)) == bad
            assert status(idx=np.zeros(0, dtype=np.int32)) == bad
            assert status(idx=None) == bad
            assert status(skel=None) == bad
            assert status(step=0) == bad
            assert status(step=-3) == bad
            assert status(out=None) == bad
            assert status(lat=None) == bad
            assert status(n=-1) == bad
            assert status(ld=prim.n_components - 1) == bad
            assert status(skel=chain, idx=chain.indices(["j%d" % (MG_MAX_CHAIN + 1)])) == unsupported      # a chain of 33 links
            assert status(p=primitive(ctx, 5, 6), skel=chain_skeleton(0), idx=np.zeros(1, dtype=np.int32)) == unsupported   # no root pose
            ends = sk.indices(["LeftHand_EndSite", "RightHand_EndSite", "Head_EndSite", "LeftFoot", "RightFoot"])
            assert status(p=primitive(ctx, 120, 79, NB=104), idx=ends) == unsupported                       # 263 KB of control points
            call(n=0)                                                                                        # MG_OK, no launch
            assert ctx.profile_get("point_clouds")[1] == 0
            call()
            ctx.synchronize()
            assert ctx.profile_get("point_clouds")[1] == 1
    finally:
        ctx.profile_enable(False)
