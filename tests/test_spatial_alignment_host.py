"""The host restatements of morphablegraphs_amd.spatial_alignment against tests/golden/spatial_alignment.npz
(tools/gen_spatial_alignment_golden.py: _align_frames_spatially compiled from the reference's own lines, construction/utils.py
imported unmodified, the absent anim_utils / transformations helpers restated in the tool), properties that need no golden,
and HipMotionModelConstructor's control flow on stub stages.

The reference goes through degrees, Euler angles, a rotation matrix and an eigenvector; the restatement goes from two unit
vectors to (cos, sin).  Measured on the fixture: the largest |host - golden| over every channel of every motion is 1.33e-15
(max |v| 1.87).  The test asserts 10 x that, with a floor of 1e-13 * max |v| (the pattern of the DTW grids).
"""
import collections
import os

import numpy as np
import pytest

from morphablegraphs_amd import _capi, spatial_alignment as sa
from morphablegraphs_amd.motion_model_constructor import HipMotionModelConstructor

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spatial_alignment.npz"))
ALIGN = [(s, k) for s in range(int(GOLDEN["a_n_sets"])) for k in range(int(GOLDEN["a%d_n" % s]))]
PREPARE = list(range(int(GOLDEN["q_n_sets"])))
MEASURED, MARGIN, FLOOR = 1.33e-15, 10.0, 1e-13
REL = 1e-12


def align_case(s, k):
    q = "a%d_m%d_" % (s, k)
    return {"in": GOLDEN[q + "in"], "out": GOLDEN[q + "out"], "heading_len": float(GOLDEN[q + "heading_len"]), "min_w": float(GOLDEN[q + "min_w"]),
            "ref": GOLDEN["a%d_ref_orientation" % s], "name": "%s motion %d" % (str(GOLDEN["a%d_name" % s]), k)}


def align_set(s):
    cases = [align_case(s, k) for k in range(int(GOLDEN["a%d_n" % s]))]
    return collections.OrderedDict(("m%d" % k, c["in"]) for k, c in enumerate(cases)), cases, cases[0]["ref"]


def prepare_case(s):
    x = GOLDEN["q%d_in" % s]
    return {"motions": collections.OrderedDict(("m%d" % i, x[i]) for i in range(len(x))), "in": x, "out": GOLDEN["q%d_out" % s],
            "scale": GOLDEN["q%d_scale" % s], "n_joints": int(GOLDEN["q%d_n_joints" % s]), "min_dot": float(GOLDEN["q%d_min_dot" % s]),
            "name": str(GOLDEN["q%d_name" % s])}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def heading_of(frame):
    """Independent of the restatement's statements: the root's rotation matrix column, from rotate_by_quaternion."""
    v = _capi.rotate_by_quaternion(frame[3:7], (0.0, 0.0, 1.0))
    return np.array([v[0], v[2]]) / np.hypot(v[0], v[2])


def random_motion(rng, n_frames, n_joints):
    f = rng.standard_normal((n_frames, 3 + 4 * n_joints))
    yaw = rng.uniform(-np.pi, np.pi) + 0.3 * rng.standard_normal(n_frames)
    tilt = 0.3 * rng.standard_normal((n_frames, 2))
    for i in range(n_frames):
        q = _capi._quat_mul(np.array([np.cos(yaw[i] / 2), 0.0, np.sin(yaw[i] / 2), 0.0]),
                            _capi._quat_mul(np.array([np.cos(tilt[i, 0] / 2), np.sin(tilt[i, 0] / 2), 0.0, 0.0]),
                                            np.array([np.cos(tilt[i, 1] / 2), 0.0, 0.0, np.sin(tilt[i, 1] / 2)])))
        f[i, 3:7] = q * rng.uniform(0.5, 3.0)
    return f


def turned_and_moved(frames, angle, offset):
    """The same motion seen from a frame of reference turned about y by `angle` and moved by `offset`."""
    out = np.array(frames)
    c, s = np.cos(angle), np.sin(angle)
    out[:, 0] = c * frames[:, 0] + s * frames[:, 2] + offset[0]
    out[:, 1] = frames[:, 1] + offset[1]
    out[:, 2] = -s * frames[:, 0] + c * frames[:, 2] + offset[2]
    qy = np.array([np.cos(angle / 2), 0.0, np.sin(angle / 2), 0.0])
    for i in range(len(frames)):
        out[i, 3:7] = _capi._quat_mul(qy, frames[i, 3:7])
    return out


# ---- the golden ----------------------------------------------------------------------------------------------------------------
def test_the_golden_file_keeps_the_generators_conditions():
    assert 4 * int(GOLDEN["redraws"]) <= int(GOLDEN["draws"])
    for s, k in ALIGN:
        c = align_case(s, k)
        assert c["heading_len"] >= 1e-3 and c["min_w"] >= 1e-3, c["name"]
        assert np.min(np.abs(c["out"][:, 3])) >= 1e-3
    for s in PREPARE:
        assert prepare_case(s)["min_dot"] >= 1e-6
    lengths = [len(align_case(s, k)["in"]) for s, k in ALIGN]
    assert 1 in lengths and 2 in lengths
    assert {align_case(s, 0)["in"].shape[1] for s in range(int(GOLDEN["a_n_sets"]))} >= {7, 11, 79}
    assert any(np.all(prepare_case(s)["scale"] == 1.0) and np.any(np.all(prepare_case(s)["in"][:, :, :3] == 0.0, axis=(0, 1))) for s in PREPARE)
    assert any(abs(prepare_case(s)["in"][-1, -1, 0]) == prepare_case(s)["scale"][0] and prepare_case(s)["in"][-1, -1, 0] < 0 for s in PREPARE)


@pytest.mark.parametrize("s", range(int(GOLDEN["a_n_sets"])))
def test_align_host_against_the_references_lines(s):
    """|host - golden| <= max(10 * 1.33e-15, 1e-13 * max |v|); measured worst 1.33e-15 (see the module docstring)."""
    motions, cases, ref = align_set(s)
    out = sa.align_motions_spatially_host(motions, 0, ref)
    assert isinstance(out, collections.OrderedDict) and list(out.keys()) == list(motions.keys())
    for (key, ours), c in zip(out.items(), cases):
        err, bound = float(np.max(np.abs(ours - c["out"]))), max(MARGIN * MEASURED, FLOOR * float(np.max(np.abs(c["out"]))))
        print("%s: max |host - golden| %.3g, bound %.3g" % (c["name"], err, bound))
        assert ours.shape == c["out"].shape and err <= bound, (c["name"], err, bound)


@pytest.mark.parametrize("s", PREPARE)
def test_prepare_host_is_the_references_two_functions_bit_for_bit(s):
    c = prepare_case(s)
    out, scale = sa.prepare_aligned_frames_host(c["motions"], c["n_joints"])
    assert list(out.keys()) == list(c["motions"].keys())
    assert same_bits(np.array(list(out.values())), c["out"]) and same_bits(scale, c["scale"]), c["name"]
    assert same_bits(np.array(list(c["motions"].values())), c["in"])       # the input is not written to


# ---- properties ----------------------------------------------------------------------------------------------------------------
PROPERTY_CASES = [(0, (0.0, -1.0)), (0, (0.0, 1.0)), (3, (2.0, 1.0)), (6, (-0.3, -0.1))]


def property_motions(seed=17):
    rng = np.random.default_rng(seed)
    return collections.OrderedDict(("c%d" % i, random_motion(rng, n, j)) for i, (n, j) in enumerate([(7, 1), (12, 3), (9, 19)]))


@pytest.mark.parametrize("frame_idx,ref", PROPERTY_CASES)
def test_aligned_frame_faces_the_reference_at_the_origin(frame_idx, ref):
    out, transforms = sa.align_motions_spatially_host({"a": property_motions()["c1"]}, frame_idx, ref, return_transforms=True)
    frame = out["a"][frame_idx]
    r = np.asarray(ref) / np.linalg.norm(ref)
    assert np.max(np.abs(heading_of(frame) - r)) <= REL
    assert np.all(frame[:3] == 0.0)
    assert abs(transforms[0, 0] ** 2 + transforms[0, 1] ** 2 - 1.0) <= REL


@pytest.mark.parametrize("frame_idx,ref", PROPERTY_CASES)
def test_alignment_does_not_depend_on_where_the_capture_stood(frame_idx, ref):
    rng = np.random.default_rng(23)
    for key, m in property_motions().items():
        if frame_idx >= len(m):
            continue
        base = sa.align_motions_spatially_host({key: m}, frame_idx, ref)[key]
        for angle in (0.4, -2.9, np.pi, rng.uniform(-np.pi, np.pi)):
            moved = turned_and_moved(m, angle, rng.uniform(-5.0, 5.0, 3))
            again = sa.align_motions_spatially_host({key: moved}, frame_idx, ref)[key]
            scale = max(1.0, float(np.max(np.abs(base))), float(np.max(np.abs(moved))))
            assert np.max(np.abs(again - base)) <= REL * scale, (key, angle)


def test_root_quaternions_are_unit_with_w_not_negative_and_other_channels_untouched():
    motions = property_motions()
    out = {key: sa.align_motions_spatially_host({key: m})[key] for key, m in motions.items()}      # one D per call
    for key, m in motions.items():
        q = out[key][:, 3:7]
        assert np.max(np.abs(np.linalg.norm(q, axis=1) - 1.0)) <= REL and np.all(q[:, 0] >= 0.0)
        assert same_bits(out[key][:, 7:], m[:, 7:])


def test_special_headings_and_a_quaternion_of_norm_three():
    """A heading equal to the reference (the identity: cos = 1, sin = 0), opposite to it (cos = -1: no special case), at +-90
    degrees; a root quaternion of norm 3 comes back with norm 1."""
    for yaw, cos, sin in ((np.pi, 1.0, 0.0), (0.0, -1.0, 0.0), (np.pi / 2, 0.0, 1.0), (-np.pi / 2, 0.0, -1.0)):
        f = np.zeros((2, 7))
        f[:, :3] = [[1.0, 2.0, 3.0], [2.0, 2.5, 5.0]]
        f[:, 3:7] = 3.0 * np.array([np.cos(yaw / 2), 0.0, np.sin(yaw / 2), 0.0])
        out, t = sa.align_motions_spatially_host({"m": f}, return_transforms=True)
        assert abs(t[0, 0] - cos) <= 1e-15 and abs(abs(t[0, 1]) - abs(sin)) <= 1e-15
        assert np.all(np.isfinite(out["m"])) and np.max(np.abs(np.linalg.norm(out["m"][:, 3:7], axis=1) - 1.0)) <= REL
        assert np.max(np.abs(heading_of(out["m"][0]) - [0.0, -1.0])) <= REL and np.all(out["m"][0, :3] == 0.0)
        assert abs(np.linalg.norm(out["m"][1, :3]) - np.linalg.norm(f[1, :3] - f[0, :3])) <= REL * 10


def test_host_refuses_what_the_device_refuses():
    good = property_motions()["c0"]
    for bad in (np.zeros((3, 8)), np.zeros((3, 3 + 4 * 65))):
        with pytest.raises(ValueError):
            sa.align_motions_spatially_host({"m": bad})
    with pytest.raises(ValueError):
        sa.align_motions_spatially_host({"m": good}, frame_idx=len(good))
    nan = good.copy()
    nan[2, 9 % good.shape[1]] = np.nan
    with pytest.raises(ValueError):
        sa.align_motions_spatially_host({"m": nan})
    up = good.copy()
    up[0, 3:7] = [1.0, 1.0, 1.0, -1.0]       # a third of a turn about (1, 1, -1): z goes onto y, and every statement is exact
    with pytest.raises(ValueError, match="'m'"):
        sa.align_motions_spatially_host({"m": up})


# ---- the constructor's control flow, on stub stages ----------------------------------------------------------------------------
CONFIG = {"n_spatial_basis_factor": 0.25, "n_components": None, "fraction": 0.95, "n_basis_functions_temporal": 8, "npc_temporal": None,
          "precision_temporal": 0.99}


class _Stub(HipMotionModelConstructor):
    """The stages replaced by recorders: what _align_frames decides is all that runs."""

    def __init__(self, **kw):
        sk = _capi.Skeleton([("Hips", None, (0.0, 0.0, 0.0)), ("Spine", "Hips", (0.0, 0.2, 0.0))], ["Hips", "Spine"])
        HipMotionModelConstructor.__init__(self, sk, CONFIG, ctx="no device", **kw)
        self.calls = []

    def _align_frames_spatially(self, input_motions):
        self.calls.append(("spatial", list(input_motions.keys())))
        return collections.OrderedDict((k, np.asarray(m) + 1.0) for k, m in input_motions.items() if k != "dropped")

    def _align_frames_temporally(self, input_motions, mean_key=None):
        self.calls.append(("temporal", mean_key))
        return input_motions, collections.OrderedDict((k, list(range(len(m)))) for k, m in input_motions.items())

    def run_dimension_reduction(self):
        self.calls.append(("fpca",))

    def learn_statistical_model(self):
        self.calls.append(("gmm",))

    def convert_motion_model_to_json(self, name="", version=1, save_skeleton=False):
        return {"name": name, "keyframes": self._keyframes}


def stub_motions():
    return collections.OrderedDict([("a", np.zeros((6, 11))), ("dropped", np.zeros((5, 11))), ("b", np.zeros((8, 11))), ("c", np.zeros((7, 11)))])


def test_align_frames_plain_branch():
    c = _Stub()
    c.set_motions(stub_motions())
    assert c.construct_model("walk", mean_key="b") == {"name": "walk", "keyframes": {}}
    assert c.calls == [("spatial", ["a", "dropped", "b", "c"]), ("temporal", "b"), ("fpca",), ("gmm",)]
    assert list(c._aligned_frames.keys()) == ["a", "b", "c"] and c._temporal_data["b"] == list(range(8))
    assert np.all(c._aligned_frames["a"] == 1.0)
    # aligned data that is already there is used as it is
    c.calls = []
    c.construct_model("walk", align_frames=False)
    assert c.calls == [("fpca",), ("gmm",)]
    # ... unless a part of it is missing
    fresh = _Stub()
    fresh.set_motions(stub_motions())
    fresh.set_aligned_frames(stub_motions())
    fresh.construct_model("walk", align_frames=False)
    assert [call[0] for call in fresh.calls] == ["spatial", "temporal", "fpca", "gmm"]


def test_align_frames_filters_preset_temporal_data_to_the_surviving_keys():
    c = _Stub()
    c.set_motions(stub_motions())
    c.set_timewarping({"c": [3], "dropped": [2], "a": [1], "unknown": [0]})
    c.construct_model("walk")
    assert [call[0] for call in c.calls] == ["spatial", "fpca", "gmm"]
    assert isinstance(c._temporal_data, collections.OrderedDict) and list(c._temporal_data.items()) == [("a", [1]), ("c", [3])]
    assert list(c._aligned_frames.keys()) == ["a", "b", "c"]


def test_align_frames_with_sections_sets_the_contact_keyframes(monkeypatch):
    from morphablegraphs_amd import dtw
    seen = {}

    def fake(skeleton, joints, motions, mean_key=None, sections=None, ctx=None, reference_selection="average_time_line"):
        seen.update({"keys": list(motions.keys()), "mean_key": mean_key, "sections": sections, "joints": list(joints)})
        return motions, collections.OrderedDict((k, [0]) for k in motions)
    monkeypatch.setattr(dtw, "align_frames_temporally", fake)
    c = _Stub()
    c.set_motions(stub_motions())
    c.set_aligned_frames(None, keyframes={"old": 1})
    sections = {k: [{"start_idx": 0, "end_idx": len(m) // 2}, {"start_idx": len(m) // 2, "end_idx": len(m)}] for k, m in stub_motions().items()}
    c.set_dtw_sections(sections)
    assert c._keyframes == {}
    data = c.construct_model("walk")
    # lengths 6, 8, 7: the mean is 7, the motion closest to it is "c"
    assert seen["mean_key"] == "c" and seen["keys"] == ["a", "b", "c"] and seen["sections"] is sections and seen["joints"] == ["Hips", "Spine"]
    assert data["keyframes"] == {"contact0": 3, "contact1": 7}
    assert [call[0] for call in c.calls] == ["spatial", "fpca", "gmm"]
    c.set_timewarping(None)      # as in the reference, temporal data that is there (now: the first run's) takes the first branch
    c.construct_model("walk", mean_key="a")
    assert c._keyframes == {"contact0": 3, "contact1": 6} and seen["mean_key"] == "a"


def test_save_skeleton_without_a_skeleton_raises():
    c = _Stub()
    c.set_motions(stub_motions())
    with pytest.raises(ValueError):
        c.construct_model("walk", save_skeleton=True)
    assert c.calls == []
    with pytest.raises(ValueError):
        HipMotionModelConstructor.convert_motion_model_to_json(c, "walk", 1, True)
    with pytest.raises(ValueError):
        _Stub(reference_selection="shortest")
    assert _Stub(skeleton_json={"root": "Hips"}).skeleton_json == {"root": "Hips"}
