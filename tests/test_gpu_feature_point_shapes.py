"""mg_feature_points at the smallest shapes at which the kernel can go wrong, on seeded synthetic primitives against
feature_points_host (and, where two device paths exist, bit for bit against the composed one), and its argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from morphablegraphs_amd import _capi, synthetic
from test_gpu_feature_points import against_host, composed, ctx, eq, item  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu

TILE = _capi.MG_FEATURE_POINTS_TILE
OUTPUTS = _capi.FEATURE_POINT_OUTPUTS


def skeleton_of(n_animated):
    return _capi.Skeleton(*synthetic.make_skeleton(n_animated))


@pytest.fixture(scope="module")
def world(ctx):
    """name -> (model dict, primitive, skeleton): small (L 5, F 14, D 23), one (L 1), walk (L 40, F 156, D 79), root (D 7)."""
    models = {"small": (synthetic.make_primitive(seed=301, n_components=5, n_frames=14, n_basis=8, n_dim=23, n_gmm=2), skeleton_of(5)),
              "one": (synthetic.make_primitive(seed=302, n_components=1, n_frames=9, n_basis=6, n_dim=11, n_gmm=2), skeleton_of(2)),
              "walk": (synthetic.make_walk_primitive(seed=3), skeleton_of(19)),
              "root": (synthetic.make_primitive(seed=303, n_components=3, n_frames=12, n_basis=7, n_dim=7, n_gmm=2),
                       _capi.Skeleton([("Hips", None, (0.0, 0.0, 0.0))], ["Hips"]))}
    out = {name: (data, _capi.Primitive(ctx, data), sk) for name, (data, sk) in models.items()}
    yield out
    for _, prim, _ in out.values():
        prim.close()


def rows(prim, n, seed, width=None):
    return 0.8 * np.random.default_rng(seed).standard_normal((n, width or prim.n_components))


def check(world, name, S, joints, frame_idx, latent_offset=0, bitwise=True):
    data, prim, sk = world[name]
    got = _capi.feature_points([item(prim, S, sk, joints, frame_idx, latent_offset)])[0]
    L = prim.n_components
    own = np.ascontiguousarray(np.asarray(S, dtype=np.float64)[:, latent_offset:latent_offset + L])
    worst = against_host(data, got, own, sk, joints, frame_idx)
    if bitwise:
        want = composed(prim, np.ascontiguousarray(np.asarray(S)[:, latent_offset:latent_offset + L]), sk, joints, frame_idx)
        for key in want:
            eq(got[key], want[key])
    return got, worst


@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1])
def test_sample_counts_around_the_tile(world, n):
    check(world, "small", rows(world["small"][1], n, n), ["Head_EndSite", "LeftHand"], 6)


@pytest.mark.parametrize("name,joints", [("one", ["Spine1"]), ("small", ["Head"]), ("walk", ["LeftHand", "RightFoot"])])
def test_latent_widths(world, name, joints):
    check(world, name, rows(world[name][1], 5, 21), joints, 4)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_an_offset_into_wider_rows_and_both_latent_dtypes(world, dtype):
    prim = world["small"][1]
    M = np.full((TILE + 3, prim.n_components + 5), 9.5, dtype=dtype)
    M[:, 2:2 + prim.n_components] = rows(prim, TILE + 3, 22).astype(dtype)
    got, _ = check(world, "small", M, ["Neck"], 3, latent_offset=2)
    # float32 latents are converted first: the bits of their float64 values
    again = _capi.feature_points([item(prim, M.astype(np.float64), world["small"][2], ["Neck"], 3, 2)])[0]
    for key in OUTPUTS:
        eq(got[key], again[key])


def test_joint_counts_zero_one_and_the_cap(world):
    data, prim, sk = world["small"]
    S = rows(prim, 3, 23)
    got, _ = check(world, "small", S, [], 10)
    assert "points" not in got
    check(world, "small", S, ["RightHand"], 10)
    cap = (sk.names + sk.names)[:_capi.MG_FEATURE_POINTS_MAX_JOINTS]       # every joint of the skeleton, rigid limbs included
    assert len(cap) == 32
    check(world, "small", S, cap, 10)
    with pytest.raises(_capi.MGError) as info:
        _capi.feature_points([item(prim, S, sk, cap + ["Hips"], 10)])
    assert info.value.status == _capi.MG_ERR_INVALID_ARGUMENT


def test_the_root_as_listed_joint_and_the_deepest_chain(world):
    data, prim, sk = world["walk"]
    S = rows(prim, 4, 24)
    deepest = max(sk.names, key=lambda n: len(sk.chain(n)))
    assert len(sk.chain(deepest)) == 8
    got, _ = check(world, "walk", S, ["Hips", deepest], 77)
    frames = prim.back_project_frames_f64(S)
    eq(got["points"][:, :3], frames[:, 77, :3] - frames[:, 0, :3])


@pytest.mark.parametrize("name", ["small", "walk"])
def test_frames_at_both_ends_and_where_the_tap_windows_overlap(world, name):
    data, prim, sk = world[name]
    F = prim.n_canonical_frames
    S = rows(prim, 3, 25)
    for frame_idx in (0, 1, 2, F // 2, F - 3, F - 2, F - 1):
        got, _ = check(world, name, S, ["Head", "Hips"], frame_idx)
        if frame_idx == 0:
            assert np.array_equal(got["points"][:, 3:], np.zeros((3, 3)))       # the root against itself
    for bad in (-1, F):
        with pytest.raises(_capi.MGError) as info:
            _capi.feature_points([item(prim, S, sk, ["Head"], bad)])
        assert info.value.status == _capi.MG_ERR_INVALID_ARGUMENT


def test_seven_channels_with_the_root_as_only_joint(world):
    prim = world["root"][1]
    for frame_idx in (0, 5, 11):
        check(world, "root", rows(prim, TILE + 1, 26), ["Hips"], frame_idx)
    check(world, "root", rows(prim, 2, 27), [], 0)


def test_two_primitives_a_primitive_twice_an_empty_item_and_the_slices(world):
    (ds, small, sks), (dw, walk, skw) = world["small"], world["walk"]
    Ss, Sw = rows(small, TILE + 2, 28), rows(walk, 3, 29)
    items = [item(small, Ss, sks, ["LeftHand"], 2), item(walk, Sw, skw, ["Head", "LeftFoot"], 100), item(small, Ss[:0], sks, ["Neck"], 1),
             item(small, Ss[:5], sks, ["Neck", "Hips"], 13)]
    got = _capi.feature_points(items)
    assert got[2]["start_root"].shape == (0, 3) and got[2]["points"].shape == (0, 3)
    for i in (0, 1, 3):
        alone = _capi.feature_points([items[i]])[0]
        for key in OUTPUTS:
            eq(got[i][key], alone[key])
    against_host(ds, got[0], Ss, sks, ["LeftHand"], 2)
    against_host(dw, got[1], Sw, skw, ["Head", "LeftFoot"], 100)
    # more one-row items than a launch takes
    n_items = _capi.MG_FEATURE_POINTS_MAX_ITEMS + 1
    S = rows(small, n_items, 30)
    parts = _capi.feature_points([item(small, np.ascontiguousarray(S[i:i + 1]), sks, ["Head"], i % 14) for i in range(n_items)])
    for frame_idx in (0, 5, 13):
        whole = _capi.feature_points([item(small, S, sks, ["Head"], frame_idx)])[0]
        for i in range(frame_idx, n_items, 14):
            for key in OUTPUTS:
                eq(parts[i][key], whole[key][i:i + 1])
    eq(parts[256]["root_end"], _capi.feature_points([item(small, S, sks, ["Head"], 256 % 14)])[0]["root_end"][256:])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_latent_that_is_not_finite_gives_nan_for_its_candidate_alone(world, bad):
    data, prim, sk = world["small"]
    S = rows(prim, TILE + 1, 31)
    want = _capi.feature_points([item(prim, S, sk, ["Head", "LeftHand"], 9)])[0]
    S[TILE - 1, prim.n_components - 1] = bad
    got = _capi.feature_points([item(prim, S, sk, ["Head", "LeftHand"], 9)])[0]
    keep = [i for i in range(len(S)) if i != TILE - 1]
    for key in OUTPUTS:
        assert np.isnan(got[key][TILE - 1]).all()
        eq(got[key][keep], want[key][keep])


def test_tables_beyond_64_kib_take_the_large_lds_opt_in_and_beyond_150_kib_are_refused(ctx, world):
    data, prim, sk = world["walk"]
    S = rows(prim, TILE + 1, 32)
    # the chains of both hands, both feet and the head: 14 quaternions and the root position, 59 channels of frame_idx;
    # 4 x 59 + 12 + 28 = 276 rows of 40 latents are 88 KB of E', 136 KB with the tile's control points
    joints = ["LeftHand", "RightHand", "Head", "LeftFoot", "RightFoot"]
    check(world, "walk", S, joints, 78)
    check(world, "walk", S.astype(np.float32), joints, 78)
    # every joint's chain: all 79 channels, 356 rows, 173 KB
    with pytest.raises(_capi.MGError) as info:
        _capi.feature_points([item(prim, S, sk, sk.names, 78)])
    assert info.value.status == _capi.MG_ERR_UNSUPPORTED


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_every_argument_check_returns_its_code_and_writes_nothing(ctx, world):
    data, prim, sk = world["small"]
    L = prim.n_components
    S = rows(prim, 4, 34)
    idx, desc = sk.indices(["Head", "LeftHand"]), sk.desc()
    other_ctx = _capi.Context(0)
    other = _capi.Primitive(other_ctx, synthetic.make_tiny_primitive(seed=2))
    few = _capi.Primitive(ctx, synthetic.make_primitive(seed=305, n_components=2, n_frames=8, n_basis=5, n_dim=6, n_gmm=2))
    narrow = _capi.Primitive(ctx, synthetic.make_primitive(seed=306, n_components=2, n_frames=8, n_basis=5, n_dim=11, n_gmm=2))
    outside = np.array([len(sk.names)], dtype=np.int32)
    widths = _capi.feature_point_widths(2)

    def table(n=1, **fields):
        """n valid items over S; `fields` overwrite members of the LAST one"""
        t = (_capi.FeaturePointItem * n)()
        keep = []
        for rec in t:
            outs = {name: np.full(4 * widths[name], -1.0) for name in OUTPUTS}
            keep.append(outs)
            rec.prim, rec.latents, rec.latent_offset, rec.n_samples, rec.ld = prim.handle.value, S.ctypes.data, 0, 4, L
            rec.skeleton, rec.joints, rec.n_joints, rec.frame_idx = C.addressof(desc), idx.ctypes.data, 2, 3
            for name in OUTPUTS:
                setattr(rec, name, outs[name].ctypes.data)
        for key, value in fields.items():
            setattr(t[n - 1], key, value)
        return t, keep

    invalid, unsupported = _capi.MG_ERR_INVALID_ARGUMENT, _capi.MG_ERR_UNSUPPORTED
    nothing = {name: None for name in OUTPUTS}
    cases = [("NULL item table", 1, (None, []), invalid),
             ("NULL primitive", 2, table(2, prim=None), invalid),
             ("NULL latents", 1, table(latents=None), invalid),
             ("columns past ld", 1, table(latent_offset=1), invalid),
             ("negative offset", 1, table(latent_offset=-1), invalid),
             ("ld below the latents", 1, table(ld=L - 1), invalid),
             ("frame below 0", 1, table(frame_idx=-1), invalid),
             ("frame past the last", 2, table(2, frame_idx=prim.n_canonical_frames), invalid),
             ("joint outside the skeleton", 1, table(joints=outside.ctypes.data, n_joints=1), invalid),
             ("joints without points", 1, table(points=None), invalid),
             ("points without joints", 1, table(n_joints=0), invalid),
             ("all outputs NULL", 1, table(n_joints=0, **nothing), invalid),
             ("two contexts", 2, table(2, prim=other.handle.value, ld=max(L, other.n_components)), invalid),
             ("fewer than 7 channels", 1, table(prim=few.handle.value, n_joints=0, points=None), unsupported),
             ("skeleton channels beyond the primitive's", 1, table(prim=narrow.handle.value), unsupported)]
    want = _capi.feature_points([item(prim, S, sk, ["Head", "LeftHand"], 3)])[0]
    for what, n, (t, keep), code in cases:
        for host in (True, False):                         # the checks come before anything is copied or launched in either form
            with pytest.raises(_capi.MGError) as info:
                _capi.feature_points_table(prim.lib, n, t, np.float64, host=host)
            assert info.value.status == code, what
        assert all((a == -1.0).all() for outs in keep for a in outs.values()), what
    got = _capi.feature_points([item(prim, S, sk, ["Head", "LeftHand"], 3)])[0]      # the library is usable afterwards
    for key in OUTPUTS:
        eq(got[key], want[key])
    # a failing item behind valid ones: nothing of the call is written
    t, keep = table(3, latents=None)
    with pytest.raises(_capi.MGError):
        _capi.feature_points_table(prim.lib, 3, t, np.float64)
    assert all((a == -1.0).all() for outs in keep for a in outs.values())
    # nothing to do: MG_OK
    _capi.feature_points_table(prim.lib, 0, None, np.float64)
    t, keep = table(2, n_samples=0)
    t[0].n_samples = 0
    _capi.feature_points_table(prim.lib, 2, t, np.float64)
    assert all((a == -1.0).all() for outs in keep for a in outs.values())
    assert _capi.feature_points([]) == []
    # a valid table writes every output
    t, keep = table(1)
    _capi.feature_points_table(prim.lib, 1, t, np.float64)
    for name in OUTPUTS:
        eq(keep[0][name], want[name].ravel())
    for p in (other, few, narrow):
        p.close()
    other_ctx.close()
