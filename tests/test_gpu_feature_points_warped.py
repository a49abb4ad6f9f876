"""mg_feature_points_warped on the device (csrc/mg_feature_points.hip), in two separated steps: (a) time_mid and n_frames against
mg_time_function_sample's row -- equal lengths, the same bits (csrc/mg_timewarp_device.h states the warp for both kernels) --
and against scipy's FITPACK within timewarp_cases' tolerance; (b) every feature output against feature_points_warped_host at
the DEVICE's time_mid and against the composed device route (mg_time_function_sample, mg_back_project_frames_at, rows 0 /
frame_idx / last, mg_joint_positions) within the float64 bound.  Then the shape edges, the NaN rules, the argument checks and
the classes end to end."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import timewarp_cases as twc
from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import feature_point_model as fpm
from morphablegraphs_amd.motion_primitive import HipMotionPrimitive
from feature_points_warped_cases import case_ids, golden_cases, time_tolerance_of

CASES, IDS = golden_cases(), case_ids()

pytestmark = pytest.mark.gpu

POSITION_BOUND = 4e-12          # per position, times the scale
TILE = _capi.MG_FEATURE_POINTS_TILE
OUTPUTS = _capi.WARPED_FEATURE_POINT_OUTPUTS
FEATURES = _capi.FEATURE_POINT_OUTPUTS
L = twc.N_SPATIAL


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def skeleton_of(n_animated):
    return _capi.Skeleton(*synthetic.make_skeleton(n_animated))


# name -> the reference's JSON: timewarp_cases' models (D 11, 6 control points, 3 spatial components) and two of the generator's
MODELS = {
    "F4": lambda: twc.model_of((4, 1))[0],                                   # the two-row system
    "F5": lambda: twc.time_model(5, 3, 4, 0.05, 511),
    "F24": lambda: twc.time_model(24, 3, 8, 0.3, 2411),                      # lengths that differ within a tile
    "F200": lambda: twc.time_model(200, 1, 8, 0.05, 20011),                  # 3 x 200 x 16 doubles: beyond 64 KiB
    "F2048": lambda: twc.model_of((2048, 1))[0],                             # beyond MG_FEATURE_POINTS_WARPED_MAX_F
    "walk": lambda: synthetic.make_walk_primitive(seed=3, n_time_components=3),
}


@pytest.fixture(scope="module")
def world(ctx):
    """name -> (model dict, primitive, skeleton)"""
    out = {}
    for name, make in MODELS.items():
        data = make()
        sk = skeleton_of(19 if name == "walk" else 2)
        out[name] = (data, _capi.Primitive(ctx, data), sk)
    yield out
    for _, prim, _ in out.values():
        prim.close()


def eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    np.testing.assert_array_equal(a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32), b.view(np.uint64 if b.dtype.itemsize == 8 else np.uint32))


def item(prim, S, skeleton=None, joints=(), frame_idx=0, latent_offset=0, time_offset=None):
    return {"prim": prim, "S": S, "skeleton": skeleton, "joints": list(joints), "frame_idx": frame_idx, "latent_offset": latent_offset,
            "time_offset": time_offset}


def rows(prim, n, seed, scale=0.8):
    """n full latent rows (spatial, then time) whose sample count is not near a tie"""
    return scale * np.random.default_rng(seed).standard_normal((n, prim.n_components + prim.n_time_components))


def composed(prim, own, skeleton, joints, frame_idx):
    """The composed device route on rows `own` (spatial then time latents): the time function's row, every frame of it, rows 0 /
    frame_idx / last, mg_joint_positions; the heading is fpm.heading_host on the route's last frame.  Returns times (the row's
    value at frame_idx), lengths, start_root, points, root_end, heading_end, heading_len; rows without the frame have NaN points."""
    n_s = prim.n_components
    times, lens = prim.time_function_sample(np.ascontiguousarray(own[:, n_s:]))
    frames = prim.back_project_frames_at(np.ascontiguousarray(own[:, :n_s]), times, lens)
    n = len(own)
    has = (lens > 0) & np.isfinite(own[:, :n_s]).all(axis=1)
    start = np.where(has[:, None], frames[:, 0, :3], np.nan)
    last = np.array([frames[b, lens[b] - 1] if has[b] else np.full(prim.n_dim, np.nan) for b in range(n)])
    out = {"times": np.array([times[b, frame_idx] if frame_idx < lens[b] else np.nan for b in range(n)]), "lengths": lens,
           "start_root": start, "root_end": last[:, [0, 2]], "heading_end": np.full((n, 2), np.nan), "heading_len": np.full(n, np.nan)}
    for b in np.flatnonzero(has):
        out["heading_end"][b], out["heading_len"][b] = fpm.heading_host(last[b])
    if len(joints):
        mid = np.array([frames[b, frame_idx] if has[b] and frame_idx < lens[b] else np.full(prim.n_dim, np.nan) for b in range(n)])
        ok = np.isfinite(mid).all(axis=1)
        pos = np.full((n, len(joints), 3), np.nan)
        if ok.any():
            pos[ok] = prim.ctx.joint_positions(skeleton, joints, np.ascontiguousarray(mid[ok]))
        out["points"] = (pos - start[:, None, :]).reshape(n, -1)
    return out


WORST = {"time_mid": 0.0, "host": 0.0, "composed": 0.0}


def check(world, name, S, joints, frame_idx, latent_offset=0, time_offset=None, fitpack=True):
    """Both steps for one item; returns the device's outputs."""
    data, prim, sk = world[name]
    n_s, n_t = prim.n_components, prim.n_time_components
    t_off = latent_offset + n_s if time_offset is None else time_offset
    got = _capi.feature_points_warped([item(prim, S, sk, joints, frame_idx, latent_offset, time_offset)])[0]
    S64 = np.asarray(S, dtype=np.float64)
    own = np.ascontiguousarray(np.concatenate((S64[:, latent_offset:latent_offset + n_s], S64[:, t_off:t_off + n_t]), axis=1))
    assert set(got) == set(OUTPUTS) - (set() if joints else {"points"})
    assert got["n_frames"].dtype == np.int32 and got["time_mid"].dtype == np.float64
    # (a) the warp against mg_time_function_sample: equal lengths, equal bits; against FITPACK to timewarp_cases' tolerance
    want = composed(prim, own.astype(np.asarray(S).dtype), sk, joints, frame_idx)
    assert np.array_equal(got["n_frames"], want["lengths"])
    eq(got["time_mid"], want["times"])
    has_frame = got["n_frames"] > frame_idx
    assert np.isnan(got["time_mid"][~has_frame]).all() and np.isfinite(got["time_mid"][has_frame]).all()
    host = fpm.feature_points_warped_host(data, own, sk, joints, frame_idx, time_mid=got["time_mid"])
    if fitpack:
        with np.errstate(all="ignore"):
            safe = np.array([np.isfinite(g).all() and twc.count_margins(twc.canonical_time_function(data, g), 1.0)[0] >= twc.MARGIN for g in own[:, n_s:]])
        assert np.array_equal(got["n_frames"][safe], host["n_frames"][safe])
        both = safe & has_frame
        if both.any():
            # e_fit from the first three rows only (the 50-digit twin is slow): the bound grows with the rows it sees, so every
            # row is held to a bound that is at most the one all rows would give
            tol = time_tolerance_of(data, own[both, n_s:][:3])
            WORST["time_mid"] = max(WORST["time_mid"], float(np.abs(got["time_mid"][both] - host["time_mid"][both]).max()))
            np.testing.assert_allclose(got["time_mid"][both], host["time_mid"][both], rtol=0, atol=tol)
    # (b) the features at the device's time_mid: the host statement and the composed device route
    finite = [host[k][np.isfinite(host[k])] for k in ("start_root", "root_end") + (("points",) if joints else ())]
    bound = POSITION_BOUND * max([1.0] + [float(np.abs(a).max()) for a in finite if a.size])
    for key in FEATURES:
        if key in got:
            assert np.array_equal(np.isnan(got[key]), np.isnan(host[key])), key
            if np.isfinite(host[key]).any():
                WORST["host"] = max(WORST["host"], float(np.nanmax(np.abs(got[key] - host[key]))))
            np.testing.assert_allclose(got[key], host[key], rtol=0, atol=bound, err_msg=key)
    for key in FEATURES:
        if key in got:
            assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
            if np.isfinite(want[key]).any():
                WORST["composed"] = max(WORST["composed"], float(np.nanmax(np.abs(got[key] - want[key]))))
            np.testing.assert_allclose(got[key], want[key], rtol=0, atol=bound, err_msg=key)
    return got


# ---- F and the time components ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,joints", [("F4", ["Spine1"]), ("F5", ["Spine1", "Hips"]), ("F24", ["Spine1"])])
def test_frame_counts_time_components_and_every_frame_of_the_warped_motion(world, name, joints):
    data, prim, sk = world[name]
    S = rows(prim, TILE + 1, 41)
    S[2, L:] = 0.0                                                            # gamma = 0: the mean time function
    lens = _capi.feature_points_warped([item(prim, S)], ("n_frames",))[0]["n_frames"]
    assert lens.min() >= 2
    for frame_idx in sorted({0, 1, int(lens.min()) - 2, int(lens.min()) - 1, int(lens.max()) - 1, int(lens.max())}):
        if frame_idx < 0:
            continue
        got = check(world, name, S, joints, frame_idx)
        short = lens <= frame_idx
        assert np.isnan(got["points"][short]).all() and np.isnan(got["time_mid"][short]).all()
        assert np.isfinite(got["points"][~short]).all()
        for key in ("start_root", "root_end", "heading_end", "heading_len"):
            assert np.isfinite(got[key]).all(), key                          # a short row keeps its root outputs
        if frame_idx == 0:
            assert np.array_equal(got["time_mid"], np.zeros(len(S)))
        last = lens == frame_idx + 1
        assert np.array_equal(got["time_mid"][last], np.full(last.sum(), prim.n_canonical_frames - 1.0))
    print("%s: time_mid against FITPACK %.3g, features against the host %.3g, against the composed route %.3g" % (
        name, WORST["time_mid"], WORST["host"], WORST["composed"]))


def test_lengths_differ_within_a_tile_and_so_do_the_knot_intervals(world):
    data, prim, sk = world["F24"]
    S = rows(prim, TILE, 42, scale=1.5)
    got = check(world, "F24", S, ["Spine1"], 9)
    assert len(set(got["n_frames"])) > 1
    knots = np.asarray(data["b_spline_knots_spatial"])
    spans = set(np.searchsorted(knots, got["time_mid"], side="right"))
    assert len(spans) > 1, spans                                             # one tile, tap windows of its own per candidate
    # mid times in the first and in the last knot interval of the spatial spline
    first = check(world, "F24", S, ["Spine1"], 1)["time_mid"]
    lens = got["n_frames"]
    last = check(world, "F24", S, ["Spine1"], int(lens.min()) - 2)["time_mid"]
    inner = np.unique(knots)
    assert (first < inner[1]).all() and (last[lens == lens.min()] > inner[-2]).all()


def test_a_primitive_with_too_many_canonical_frames_is_refused(ctx, world):
    data, prim, sk = world["F2048"]
    assert prim.n_canonical_frames > _capi.MG_FEATURE_POINTS_WARPED_MAX_F
    uploads = ctx.table_uploads("feature_points_warped")
    with pytest.raises(_capi.MGError) as info:
        _capi.feature_points_warped([item(prim, rows(prim, 3, 43), sk, ["Spine1"], 1)])
    assert info.value.status == _capi.MG_ERR_UNSUPPORTED
    assert ctx.table_uploads("feature_points_warped") == uploads


# ---- batch and layout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 257])
def test_sample_counts_around_the_tile(world, n):
    check(world, "F24", rows(world["F24"][1], n, n), ["Spine1", "Head_EndSite"], 7, fitpack=n <= TILE + 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_offsets_into_wider_rows_and_both_latent_dtypes(world, dtype):
    data, prim, sk = world["F24"]
    n_t = prim.n_time_components
    own = rows(prim, TILE + 3, 44).astype(dtype)
    M = np.full((TILE + 3, L + n_t + 6), 9.5, dtype=dtype)
    M[:, 1:1 + n_t], M[:, 6:6 + L] = own[:, L:], own[:, :L]                  # the time latents IN FRONT of the spatial ones
    got = check(world, "F24", M, ["Spine1"], 5, latent_offset=6, time_offset=1, fitpack=dtype == np.float64)
    # float32 latents are converted first: the bits of their float64 values
    again = _capi.feature_points_warped([item(prim, M.astype(np.float64), sk, ["Spine1"], 5, 6, 1)])[0]
    packed = _capi.feature_points_warped([item(prim, own, sk, ["Spine1"], 5)])[0]
    for key in OUTPUTS:
        eq(got[key], again[key])
        eq(got[key], packed[key])


def test_joint_counts_and_an_item_that_needs_the_large_lds_opt_in_beside_one_that_does_not(ctx, world):
    (dw, walk, skw), (ds, small, sks), (dl, long_, skl) = world["walk"], world["F24"], world["F200"]
    Sw, Ss, Sl = rows(walk, TILE + 1, 45, 0.5), rows(small, 3, 46), rows(long_, 2, 47)
    cap = (skw.names + skw.names)[:_capi.MG_FEATURE_POINTS_MAX_JOINTS]
    assert len(cap) == 32
    check(world, "walk", Sw, cap, 77, fitpack=False)                         # J = 32, 75 KB of LDS
    check(world, "walk", Sw[:3], ["LeftHand"], 150, fitpack=False)
    root_only = check(world, "walk", Sw[:3], [], 0, fitpack=False)
    assert "points" not in root_only
    check(world, "F200", Sl, ["Spine1"], 100)                                 # 77 KB for the inversion alone
    # several items in one call: different primitives and joint lists, one of them root-only, an empty one
    items = [item(walk, Sw, skw, ["LeftHand", "RightFoot"], 77), item(small, Ss, sks, ["Spine1"], 7), item(small, Ss[:0], sks, ["Hips"], 1),
             item(small, Ss), item(long_, Sl, skl, ["Head_EndSite"], 150)]
    uploads = ctx.table_uploads("feature_points_warped")
    got = _capi.feature_points_warped(items)
    assert ctx.table_uploads("feature_points_warped") == uploads + 1
    assert got[2]["n_frames"].shape == (0,) and got[2]["points"].shape == (0, 3)
    for i in (0, 1, 3, 4):
        alone = _capi.feature_points_warped([items[i]])[0]
        assert set(alone) == set(got[i])
        for key in alone:
            eq(got[i][key], alone[key])
    with pytest.raises(_capi.MGError) as info:
        _capi.feature_points_warped([item(walk, Sw, skw, cap + ["Hips"], 10)])
    assert info.value.status == _capi.MG_ERR_INVALID_ARGUMENT


def test_more_items_than_a_launch_takes(world):
    data, prim, sk = world["F5"]
    n_items = _capi.MG_FEATURE_POINTS_MAX_ITEMS + 1
    S = rows(prim, n_items, 48)
    parts = _capi.feature_points_warped([item(prim, np.ascontiguousarray(S[i:i + 1]), sk, ["Spine1"], i % 3) for i in range(n_items)])
    for frame_idx in range(3):
        whole = _capi.feature_points_warped([item(prim, S, sk, ["Spine1"], frame_idx)])[0]
        for i in range(frame_idx, n_items, 3):
            for key in OUTPUTS:
                eq(parts[i][key], whole[key][i:i + 1])


# ---- NaN and independence ---------------------------------------------------------------------------------------------------
def test_what_is_not_finite_stays_with_its_candidate_and_a_permuted_batch_gives_permuted_rows(world):
    data, prim, sk = world["F24"]
    S = rows(prim, TILE + 2, 49)
    clean = _capi.feature_points_warped([item(prim, S, sk, ["Spine1"], 6)])[0]
    bad = S.copy()
    bad[3, 1] = np.nan                                                        # a spatial latent
    bad[TILE - 1, L] = np.nan                                                 # a time latent
    bad[TILE, L + 1] = 1.0e5                                                  # exp() overflows
    bad[7, 0] = np.inf
    got = check(world, "F24", bad, ["Spine1"], 6)
    assert got["n_frames"][TILE - 1] == 0 and got["n_frames"][TILE] == 0
    for b in (TILE - 1, TILE):
        for key in FEATURES + ("time_mid",):
            assert np.isnan(got[key][b]).all(), key
    for b in (3, 7):
        assert got["n_frames"][b] == clean["n_frames"][b] and got["time_mid"][b] == clean["time_mid"][b]
        for key in FEATURES:
            assert np.isnan(got[key][b]).all(), key
    keep = [i for i in range(len(S)) if i not in (3, 7, TILE - 1, TILE)]
    for key in OUTPUTS:
        eq(got[key][keep], clean[key][keep])                                  # the neighbours' bits
        eq(_capi.feature_points_warped([item(prim, S[5:6], sk, ["Spine1"], 6)])[0][key], clean[key][5:6])
    perm = np.random.default_rng(50).permutation(len(S))
    moved = _capi.feature_points_warped([item(prim, np.ascontiguousarray(S[perm]), sk, ["Spine1"], 6)])[0]
    for key in OUTPUTS:
        eq(moved[key], clean[key][perm])


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_every_argument_check_returns_its_code_and_launches_nothing(ctx, world):
    data, prim, sk = world["F24"]
    n_t = prim.n_time_components
    S = rows(prim, 4, 51)
    ld = L + n_t
    idx, desc = sk.indices(["Spine1", "Hips"]), sk.desc()
    other_ctx = _capi.Context(0)
    other = _capi.Primitive(other_ctx, twc.model_of((5, 1))[0])
    untimed = _capi.Primitive(ctx, synthetic.make_primitive(seed=307, n_components=L, n_frames=8, n_basis=5, n_dim=11, n_gmm=2))
    few = _capi.Primitive(ctx, synthetic.make_primitive(seed=308, n_components=L, n_frames=8, n_basis=5, n_dim=6, n_gmm=2, n_time_components=n_t, n_basis_time=4))
    outside = np.array([len(sk.names)], dtype=np.int32)
    widths = dict(_capi.feature_point_widths(2), time_mid=1, n_frames=1)

    def table(n=1, **fields):
        """n valid items over S; `fields` overwrite members of the LAST one"""
        t = (_capi.WarpedFeaturePointItem * n)()
        keep = []
        for rec in t:
            outs = {name: np.full(4 * widths[name], -1.0) if name != "n_frames" else np.full(4, -1, dtype=np.int32) for name in OUTPUTS}
            keep.append(outs)
            rec.prim, rec.latents, rec.latent_offset, rec.n_samples, rec.ld, rec.time_offset = prim.handle.value, S.ctypes.data, 0, 4, ld, L
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
             ("spatial columns past ld", 1, table(latent_offset=n_t + 1, time_offset=0), invalid),
             ("negative offset", 1, table(latent_offset=-1), invalid),
             ("ld below the latents", 1, table(ld=L - 1), invalid),
             ("negative time offset", 1, table(time_offset=-1), invalid),
             ("time columns past ld", 2, table(2, time_offset=L + 1), invalid),
             ("time columns inside the spatial ones", 1, table(time_offset=L - 1, ld=ld + 4), invalid),
             ("spatial columns inside the time ones", 1, table(latent_offset=n_t - 1, time_offset=0, ld=ld + 4), invalid),
             ("frame below 0", 1, table(frame_idx=-1), invalid),
             ("no time model", 1, table(prim=untimed.handle.value), invalid),
             ("joint outside the skeleton", 1, table(joints=outside.ctypes.data, n_joints=1), invalid),
             ("joints without points", 1, table(points=None), invalid),
             ("points without joints", 1, table(n_joints=0), invalid),
             ("all outputs NULL", 1, table(n_joints=0, **nothing), invalid),
             ("two contexts", 2, table(2, prim=other.handle.value), invalid),
             ("fewer than 7 channels", 1, table(prim=few.handle.value, n_joints=0, points=None), unsupported)]
    want = _capi.feature_points_warped([item(prim, S, sk, ["Spine1", "Hips"], 3)])[0]
    uploads = ctx.table_uploads("feature_points_warped")
    for what, n, (t, keep), code in cases:
        for host in (True, False):                         # the checks come before anything is copied or launched in either form
            with pytest.raises(_capi.MGError) as info:
                _capi.feature_points_warped_table(prim.lib, n, t, np.float64, host=host)
            assert info.value.status == code, what
        assert all((a == -1).all() for outs in keep for a in outs.values()), what
    assert ctx.table_uploads("feature_points_warped") == uploads
    # frame_idx has no upper bound on the host: the warped length is the candidate's
    t, keep = table(frame_idx=10 ** 6)
    _capi.feature_points_warped_table(prim.lib, 1, t, np.float64)
    assert np.isnan(keep[0]["points"]).all() and np.isnan(keep[0]["time_mid"]).all()
    eq(keep[0]["root_end"], want["root_end"].ravel())
    eq(keep[0]["n_frames"], want["n_frames"])
    # nothing to do: MG_OK
    _capi.feature_points_warped_table(prim.lib, 0, None, np.float64)
    t, keep = table(2, n_samples=0)
    t[0].n_samples = 0
    _capi.feature_points_warped_table(prim.lib, 2, t, np.float64)
    assert all((a == -1).all() for outs in keep for a in outs.values())
    assert _capi.feature_points_warped([]) == []
    # a valid table writes every output
    t, keep = table(1)
    _capi.feature_points_warped_table(prim.lib, 1, t, np.float64)
    for name in OUTPUTS:
        eq(keep[0][name], want[name].ravel())
    for p in (other, untimed, few):
        p.close()
    other_ctx.close()


# ---- the fixture and the classes ---------------------------------------------------------------------------------------------
def _primitive(ctx, data):
    mp = HipMotionPrimitive(None, context=ctx)
    mp._initialize_from_json(data)
    return mp


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_model_end_to_end_on_the_fixture(ctx, case):
    """Observed on an MI355X: see DESIGN 4.25 (the figures are printed)."""
    data, skeleton, rec = case
    mp = _primitive(ctx, data)
    joints, frame_idx = [str(j) for j in rec["feature_joints"]], int(rec["frame_idx"])
    bound = POSITION_BOUND * max(1.0, float(np.abs(rec["root_pos"]).max()), float(np.abs(rec["feature_points"]).max()))
    model = fpm.HipFeaturePointModel(mp, skeleton, latents=rec["root_latents"], time_warped=True, ctx=ctx)
    model.create_root_pos_ori(len(rec["root_latents"]))
    model.convert_ori_to_angle_deg()
    np.testing.assert_allclose(np.array(model.root_pos), rec["root_pos"], rtol=0, atol=bound)
    np.testing.assert_allclose(np.array(model.root_orientation), rec["root_orientation"], rtol=0, atol=bound)
    np.testing.assert_allclose(np.array(model.root_rot_angles), rec["root_rot_angles"], rtol=0, atol=1e-11)
    model.latents = rec["low_dimension_vectors"]
    model.create_feature_points(joints, len(rec["low_dimension_vectors"]), frame_idx)
    print("%s: points %.3g, orientations %.3g against the fixture (bound %.3g)" % (
        data["name"], np.abs(np.array(model.feature_points) - rec["feature_points"]).max(), np.abs(np.array(model.orientations) - rec["orientations"]).max(), bound))
    np.testing.assert_allclose(np.array(model.feature_points), rec["feature_points"], rtol=0, atol=bound)
    np.testing.assert_allclose(np.array(model.orientations), rec["orientations"], rtol=0, atol=bound)
    assert model.low_dimension_vectors == rec["low_dimension_vectors"].tolist()
    # the warp itself against what the reference recorded
    got = _capi.feature_points_warped([item(mp._prim, rec["low_dimension_vectors"], frame_idx=frame_idx)], ("time_mid", "n_frames"))[0]
    assert np.array_equal(got["n_frames"], rec["n_frames"])
    n_s = mp._prim.n_components
    np.testing.assert_allclose(got["time_mid"], rec["time_mid"], rtol=0, atol=time_tolerance_of(data, rec["low_dimension_vectors"][:, n_s:]))
    with pytest.raises(IndexError):
        model.create_feature_points(joints, len(rec["low_dimension_vectors"]), int(rec["n_frames"].min()))
    with pytest.raises(NotImplementedError):
        fpm.HipFeaturePointModel(mp, skeleton, latents=rec["root_latents"], ctx=ctx).create_root_pos_ori(len(rec["root_latents"]))


def test_the_builder_over_two_timed_nodes_and_one_without_a_time_model(ctx, tmp_path):
    nodes = {("walk", "leftStance"): _primitive(ctx, CASES[0][0]), ("carry", "turn"): _primitive(ctx, CASES[1][0]),
             ("walk", "plain"): _primitive(ctx, synthetic.make_primitive(seed=71, n_components=5, n_frames=12, n_basis=7, n_dim=11, n_gmm=3, name="walk_plain"))}
    builder = fpm.HipFeaturePointModelBuilder(context=ctx, device=True, max_components=2, seed=1, time_warped=True)
    builder.morphable_model_directory, builder.n_samples = str(tmp_path), 96
    np.random.seed(2)
    warped, plain = ctx.table_uploads("feature_points_warped"), ctx.table_uploads("feature_points")
    result = builder.build(nodes)
    assert ctx.table_uploads("feature_points_warped") == warped + 1          # one warped call for the two timed nodes
    assert ctx.table_uploads("feature_points") == plain + 1                  # ... and one call for the rest
    assert set(result) == set(nodes)
    for (key, node), case in zip(list(nodes.items())[:2], CASES):
        saved = json.load(open(str(tmp_path / ("%s_%s_root_dist_angle.json" % key))))
        assert saved == result[key] and saved["feature_type"] == "angle"
        model = builder.models[key]
        assert len(model.root_pos) == 96
        S = np.asarray(model.root_low_dimension_vectors[:4])
        assert S.shape[1] == node._prim.n_components + node._prim.n_time_components     # full rows
        want = fpm.feature_points_warped_host(case[0], S)
        np.testing.assert_allclose(np.array(model.root_pos[:4]), want["root_end"], rtol=0, atol=POSITION_BOUND * max(1.0, np.abs(want["root_end"]).max()))
