"""mg_feature_points on the device (csrc/mg_feature_points.hip): against feature_points_host on the golden models, bit for bit
against the composed device path (mg_back_project_frames_f64 of the three frames, then mg_joint_positions), bit for bit across
batches and items, and through HipFeaturePointModel and HipFeaturePointModelBuilder."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import feature_point_model as fpm
from morphablegraphs_amd.motion_primitive import HipMotionPrimitive
from test_feature_points_host import CASES, IDS

pytestmark = pytest.mark.gpu

POSITION_BOUND = 4e-12          # per position, times the scale: what the float64 frames path is held to (test_gpu_parity.py:77)
OUTPUTS = _capi.FEATURE_POINT_OUTPUTS


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def eq(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def item(prim, S, skeleton=None, joints=(), frame_idx=0, latent_offset=0):
    return {"prim": prim, "S": S, "skeleton": skeleton, "joints": list(joints), "frame_idx": frame_idx, "latent_offset": latent_offset}


def composed(prim, S, skeleton, joints, frame_idx):
    """The same quantities through whole float64 frames on the device and mg_joint_positions: start_root, points, root_end."""
    frames = prim.back_project_frames_f64(S)
    out = {"start_root": frames[:, 0, :3].copy(), "root_end": frames[:, -1, [0, 2]].copy()}
    if len(joints):
        pos = prim.ctx.joint_positions(skeleton, joints, np.ascontiguousarray(frames[:, frame_idx]))
        out["points"] = (pos - frames[:, None, 0, :3]).reshape(len(S), -1)
    return out


def against_host(data, got, S, skeleton, joints, frame_idx, scale=None):
    """The device's outputs within the float64 bound of the NumPy statement; returns the largest difference."""
    want = fpm.feature_points_host(data, S, skeleton, joints, frame_idx)
    scale = scale or max(1.0, float(np.abs(want["start_root"]).max()), float(np.abs(want["root_end"]).max()),
                         float(np.abs(want["points"]).max()) if "points" in want else 0.0)
    worst = 0.0
    assert set(got) == set(want)
    for key in want:
        assert got[key].shape == want[key].shape and got[key].dtype == np.float64, key
        worst = max(worst, float(np.abs(got[key] - want[key]).max()) if want[key].size else 0.0)
        np.testing.assert_allclose(got[key], want[key], rtol=0, atol=POSITION_BOUND * scale, err_msg=key)
    return worst


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_against_the_host_statement_on_the_golden_models(ctx, case):
    """Observed on an MI355X: see DESIGN 4.24 (the figures are printed)."""
    data, skeleton, rec = case
    prim = _capi.Primitive(ctx, data)
    joints, frame_idx = [str(j) for j in rec["feature_joints"]], int(rec["frame_idx"])
    got = _capi.feature_points([item(prim, rec["low_dimension_vectors"], skeleton, joints, frame_idx)])[0]
    worst = against_host(data, got, rec["low_dimension_vectors"], skeleton, joints, frame_idx)
    root = _capi.feature_points([item(prim, rec["root_latents"])])[0]
    worst = max(worst, against_host(data, root, rec["root_latents"], None, [], 0))
    print("%s: device against host %.3g" % (data["name"], worst))
    # ... and what the reference recorded, to the same bound
    scale = max(1.0, float(np.abs(rec["root_pos"]).max()), float(np.abs(rec["feature_points"]).max()))
    np.testing.assert_allclose(got["points"], rec["feature_points"], rtol=0, atol=POSITION_BOUND * scale)
    np.testing.assert_allclose(got["heading_end"], rec["orientations"], rtol=0, atol=POSITION_BOUND * scale)
    np.testing.assert_allclose(root["root_end"], rec["root_pos"], rtol=0, atol=POSITION_BOUND * scale)
    np.testing.assert_allclose(root["heading_end"], rec["root_orientation"], rtol=0, atol=POSITION_BOUND * scale)
    prim.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bit_for_bit_against_the_composed_device_path(ctx, case, dtype):
    data, skeleton, rec = case
    prim = _capi.Primitive(ctx, data)
    joints = [str(j) for j in rec["feature_joints"]]
    S = np.tile(rec["low_dimension_vectors"], (3, 1)).astype(dtype)
    S[len(S) // 3:] *= 0.7
    for frame_idx in (0, int(rec["frame_idx"]), prim.n_canonical_frames - 1):
        got = _capi.feature_points([item(prim, S, skeleton, joints, frame_idx)])[0]
        want = composed(prim, S, skeleton, joints, frame_idx)
        for key in ("start_root", "points", "root_end"):
            eq(got[key], want[key])
    prim.close()


def test_a_candidate_does_not_depend_on_the_batch_or_the_other_items(ctx):
    (d0, sk0, r0), (d1, sk1, r1) = CASES
    p0, p1 = _capi.Primitive(ctx, d0), _capi.Primitive(ctx, d1)
    j1 = [str(j) for j in r1["feature_joints"]]
    rng = np.random.default_rng(11)
    S = np.concatenate((r1["low_dimension_vectors"], 0.8 * rng.standard_normal((40, p1.n_components))))
    alone = _capi.feature_points([item(p1, S[:1], sk1, j1, 7)])[0]
    full = _capi.feature_points([item(p1, S, sk1, j1, 7)])[0]
    second = _capi.feature_points([item(p0, r0["low_dimension_vectors"], sk0, ["Hips_EndSite"], 2), item(p1, S[:17], sk1, j1, 7)])
    assert set(alone) == set(OUTPUTS)
    for key in OUTPUTS:
        eq(full[key][:1], alone[key])
        eq(second[1][key], full[key][:17])
        for n in (15, 16, 17):
            eq(_capi.feature_points([item(p1, S[:n], sk1, j1, 7)])[0][key], full[key][:n])
    first = _capi.feature_points([item(p0, r0["low_dimension_vectors"], sk0, ["Hips_EndSite"], 2)])[0]
    for key in OUTPUTS:
        eq(second[0][key], first[key])
    p0.close()
    p1.close()


def _primitive(ctx, data):
    mp = HipMotionPrimitive(None, context=ctx)
    mp._initialize_from_json(data)
    return mp


def test_the_model_end_to_end_on_512_samples(ctx, tmp_path):
    data, skeleton, rec = CASES[0]
    mp = _primitive(ctx, data)
    joints = [str(j) for j in rec["feature_joints"]]
    np.random.seed(5)
    model = fpm.HipFeaturePointModel(mp, skeleton, device=True, max_components=2, seed=3, ctx=ctx)
    model.create_feature_points(joints, 512, int(rec["frame_idx"]))
    assert len(model.low_dimension_vectors) == len(model.feature_points) == len(model.orientations) == 512
    want = fpm.feature_points_host(data, np.array(model.low_dimension_vectors[:8]), skeleton, joints, int(rec["frame_idx"]))
    np.testing.assert_allclose(np.array(model.feature_points[:8]), want["points"], rtol=0, atol=POSITION_BOUND * max(1.0, np.abs(want["points"]).max()))
    model.feature_point = joints[-1]
    model.model_feature_points()
    assert 1 <= model.feature_point_dist.n_components <= 2
    scores = model.score_targets(np.array(model.feature_points))
    assert abs(scores.mean() - 5 - model.threshold) <= 1e-9 * max(1.0, abs(model.threshold))      # averageScore - 5, as written
    model.save_feature_distribution(str(tmp_path / "points.json"))
    saved = json.load(open(str(tmp_path / "points.json")))
    assert set(saved) == {"name", "feature_point", "gmm_weights", "gmm_means", "gmm_covars", "threshold"}
    assert saved["name"] == data["name"] and np.shape(saved["gmm_means"])[1] == 3 * len(joints)
    best = int(np.argmax(scores))
    assert model.check_reachability(model.feature_points[best]) is True
    assert model.check_reachability(np.asarray(model.feature_points[best]) + 1e4) is False
    # the root features of the same model, host-drawn latents: the reference's stream
    np.random.seed(6)
    model.device = False
    model.create_root_pos_ori(64)
    model.convert_ori_to_angle_deg()
    model.model_root_dist()
    assert model.root_feature_dist_type == "angle" and np.shape(model.root_feature_dist.means_)[1] == 3
    assert np.isfinite(model.score_trajectory_target([model.root_pos[0][0], model.root_pos[0][1], model.root_rot_angles[0]]))
    assert min(model.heading_lengths) > 0.0


def test_the_builder_over_a_three_node_graph(ctx, tmp_path):
    shapes = {("walk", "leftStance"): (5, 12, 7, 11), ("walk", "rightStance"): (8, 33, 9, 23), ("carry", "turn"): (3, 20, 6, 7)}
    nodes = {key: _primitive(ctx, synthetic.make_primitive(seed=70 + i, n_components=L, n_frames=F, n_basis=NB, n_dim=D, n_gmm=3, name="_".join(key)))
             for i, (key, (L, F, NB, D)) in enumerate(shapes.items())}
    config = {"model_data_dir": str(tmp_path), "skeleton_file_dir": "unused.bvh", "n_samples": 96}
    with open(str(tmp_path / "config.json"), "w") as f:
        json.dump(config, f)
    builder = fpm.HipFeaturePointModelBuilder(context=ctx, device=True, max_components=2, seed=1)
    assert builder.n_samples == 10000
    builder.set_config(str(tmp_path / "config.json"))
    assert builder.n_samples == 96 and builder.morphable_model_directory == str(tmp_path)
    np.random.seed(2)
    uploads = ctx.table_uploads("feature_points")
    result = builder.build(nodes)
    assert ctx.table_uploads("feature_points") == uploads + 1          # one call for all nodes
    assert set(result) == set(shapes)
    for key in shapes:
        path = tmp_path / ("%s_%s_root_dist_angle.json" % key)
        saved = json.load(open(str(path)))
        assert saved == result[key]
        assert set(saved) == {"name", "feature_point", "gmm_weights", "gmm_means", "gmm_covars", "threshold", "feature_type"}
        assert saved["feature_type"] == "angle" and saved["feature_point"] == "Hips" and np.shape(saved["gmm_means"])[1] == 3
        model = builder.models[key]
        assert len(model.root_pos) == 96
        want = fpm.feature_points_host(nodes[key], np.asarray(model.root_low_dimension_vectors[:4]))
        np.testing.assert_allclose(np.array(model.root_pos[:4]), want["root_end"], rtol=0, atol=POSITION_BOUND * max(1.0, np.abs(want["root_end"]).max()))
