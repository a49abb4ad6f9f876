"""graph_walk.py without a device: assemble_walk_host (the NumPy statement of mg_walk_frames' arithmetic, which transforms
FRAMES) against the oracle's control-point chain (back_project_spatial_coeffs -> align_coeffs_to_previous_frame /
align_coeffs_to_start_pose -> spline_frames, the exit frame handed to the next step), and HipGraphWalk's bookkeeping against a
stub graph.  The cases and the tolerance are shared with tests/test_gpu_graph_walk.py."""
import copy
import json

import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import graph_walk as gw
from morphablegraphs_amd.candidate_scoring import alignment_from_start_pose
from oracle import mg_oracle as orc

# The two sides are algebraically equal float64 formulations (control points transformed, then the spline -- frames of the spline,
# then transformed); their largest disagreement over the four cases below, measured on the CPU as max |difference| over every channel
# relative to the largest |root coordinate| of the case, is 1.23e-15.  The tolerance is 10 x that, the rule gmm_train
# uses (10 x the reference's own spread); it is relative to the largest |root coordinate| too.
MEASURED_DISAGREEMENT = 1.23e-15
WALK_TOLERANCE = 10.0 * MEASURED_DISAGREEMENT

N_ANIMATED = 2                      # Hips and Spine: n_dim = 3 + 4 * 2 = 11
SHAPES = [(5, 12, 7), (8, 33, 9), (3, 20, 6)]     # (n_components, n_canonical_frames, n_basis): three primitives of one n_dim
SEQUENCE = [0, 1, 2, 1, 0, 2]       # six steps; two primitives are used twice
CASES = [("previous", "Hips"), ("previous", "Spine"), ("start_pose", "Hips"), ("none", "Hips")]
START_POSE = {"position": [35.0, 7.0, -12.0], "orientation": [0.0, 40.0, 0.0]}


def primitive_jsons():
    return [synthetic.make_primitive(seed=70 + i, n_components=L, n_frames=F, n_basis=NB, n_dim=3 + 4 * N_ANIMATED, n_gmm=2, name="w%d" % i)
            for i, (L, F, NB) in enumerate(SHAPES)]


def walk_case(kind, node, n_walks=1, seed=11, sequence=SEQUENCE):
    """(jsons per step, S (n_walks, sum L), alignment record, hip skeleton or None, (joints, animated), previous frame or None)."""
    datas = primitive_jsons()
    joints, animated = synthetic.make_skeleton(N_ANIMATED)
    hip_sk = _capi.Skeleton(joints, animated)
    steps = [datas[k] for k in sequence]
    rng = np.random.default_rng(seed)
    S = 0.7 * rng.standard_normal((n_walks, sum(len(d["eigen_vectors_spatial"]) for d in steps)))
    prev, alignment = None, None
    if kind == "previous":
        prev = orc.OraclePrimitive(datas[1]).back_project_frames(rng.standard_normal(SHAPES[1][0]))[-1].copy()
        prev[0] += 120.0
        prev[2] -= 40.0
        alignment = hip_sk.alignment_to(prev, node)
    elif kind == "start_pose":
        alignment = alignment_from_start_pose(START_POSE)
    return steps, S, alignment, (hip_sk if node != "Hips" else None), (joints, animated), prev


def oracle_walk(steps, row, kind, node, skel, prev):
    """The oracle's chain for one walk: (frames, smallest xz norm of any heading before normalisation)."""
    joints, animated = skel
    parts, off, least = [], 0, np.inf
    start_pose = copy.deepcopy(START_POSE)
    ref = np.array([0.0, 0.0, 1.0])

    def xz_norm(pose):
        p = orc.joint_global_orientation(pose, joints, animated, node) @ ref
        return float(np.hypot(p[0], p[2]))
    if prev is not None:
        least = xz_norm(prev)
    for i, data in enumerate(steps):
        op = orc.OraclePrimitive(data)
        coeffs = op.back_project_spatial_coeffs(row[off:off + op.n_components])
        off += op.n_components
        least = min(least, xz_norm(coeffs[0]))
        if prev is not None:
            coeffs = orc.align_coeffs_to_previous_frame(coeffs, prev, joints, animated, node)
        elif i == 0 and kind == "start_pose":
            coeffs = orc.align_coeffs_to_start_pose(coeffs, start_pose)
        fr = orc.spline_frames(op.knots, coeffs, op.canonical_time_function())
        prev = fr[-1]
        least = min(least, xz_norm(prev))
        parts.append(fr)
    return np.concatenate(parts), least


def root_scale(frames):
    return float(np.nanmax(np.abs(frames[..., :3])))


@pytest.mark.parametrize("kind,node", CASES)
def test_assemble_walk_host_is_the_oracles_control_point_chain(kind, node):
    steps, S, alignment, hip_sk, skel, prev = walk_case(kind, node, n_walks=2)
    frames, offsets, transforms = gw.assemble_walk_host(steps, S, alignment=alignment, skeleton=hip_sk)
    assert frames.shape == (2, sum(d["n_canonical_frames"] for d in steps), 3 + 4 * N_ANIMATED)
    assert np.array_equal(offsets[0], np.concatenate(([0], np.cumsum([d["n_canonical_frames"] for d in steps]))))
    for w in range(2):
        ref, least = oracle_walk(steps, S[w], kind, node, skel, prev)
        assert least >= 0.1, "a heading of the case is badly conditioned: %g" % least
        worst = float(np.max(np.abs(frames[w] - ref))) / root_scale(ref)
        print("case %s/%s walk %d: disagreement %.3g of the root scale %.4g" % (kind, node, w, worst, root_scale(ref)))
        assert worst <= WALK_TOLERANCE
    if kind == "none":
        assert np.array_equal(transforms[:, 0], np.tile([1.0, 0.0, 0.0, 0.0], (2, 1)))
    assert np.allclose(transforms[..., 0] ** 2 + transforms[..., 1] ** 2, 1.0, atol=1e-12)


# ---- bookkeeping against a stub graph ----------------------------------------------------------------------------------
class StubNode(object):
    """What HipGraphWalk(host=True) reads of a node: the spatial model's arrays and, with n_time > 0, a time function whose
    length follows the first time latent."""

    def __init__(self, data, n_time=0):
        self.s_pca = {"eigen_vectors": np.asarray(data["eigen_vectors_spatial"]).T, "mean_vector": np.asarray(data["mean_spatial_vector"]),
                      "n_basis": data["n_basis_spatial"], "n_dim": data["n_dim_spatial"], "knots": np.asarray(data["b_spline_knots_spatial"]),
                      "n_components": len(data["eigen_vectors_spatial"])}
        self.translation_maxima = np.asarray(data["translation_maxima"])
        self.n_canonical_frames = data["n_canonical_frames"]
        self.n_time, self.has_time_parameters, self.smooth_time_parameters = n_time, n_time > 0, False

    def get_n_spatial_components(self):
        return self.s_pca["n_components"]

    def get_n_time_components(self):
        return self.n_time

    def back_project_time_function(self, gamma, speed=1.0):
        return np.linspace(0.0, self.n_canonical_frames - 1.0, self.n_canonical_frames + int(gamma[0]))


class StubGraph(object):
    def __init__(self, n_time=0):
        self.nodes = {("walk", d["name"]): StubNode(d, n_time) for d in primitive_jsons()}


def stub_walk(n_time=0, start_pose=None, sequence=SEQUENCE, seed=3):
    graph = StubGraph(n_time)
    walk = gw.HipGraphWalk(graph, start_pose=start_pose, host=True)
    rng = np.random.default_rng(seed)
    for k in sequence:
        key = ("walk", "w%d" % k)
        par = np.concatenate((0.7 * rng.standard_normal(SHAPES[k][0]), rng.integers(-3, 4, n_time).astype(np.float64)))
        walk.steps.append(gw.HipGraphWalkStep.from_graph(graph, key, par))
    return graph, walk


def test_steps_get_their_frame_ranges_on_the_canonical_grid():
    _, walk = stub_walk()
    walk.convert_graph_walk_to_quaternion_frames()
    F = [SHAPES[k][1] for k in SEQUENCE]
    starts = np.concatenate(([0], np.cumsum(F)[:-1]))
    assert [s.start_frame for s in walk.steps] == starts.tolist()
    assert [s.end_frame for s in walk.steps] == (starts + np.array(F) - 1).tolist()
    assert walk.get_num_of_frames() == sum(F) and walk.get_quat_frames().shape == (sum(F), 11)
    assert walk.get_quat_frames() is walk.get_quat_frames()          # one copy until the next change
    steps = [walk.motion_state_graph.nodes[s.node_key] for s in walk.steps]
    S = np.array(walk.get_global_spatial_parameter_vector())[None, :]
    ref, _, _ = gw.assemble_walk_host(steps, S)
    assert np.array_equal(walk.get_quat_frames(), ref[0])


def test_steps_get_their_frame_ranges_with_given_lengths():
    _, walk = stub_walk(n_time=1)
    walk.convert_graph_walk_to_quaternion_frames(use_time_parameters=True)
    lengths = [SHAPES[k][1] + int(s.parameters[-1]) for k, s in zip(SEQUENCE, walk.steps)]
    assert len(set(np.array(lengths) - np.array([SHAPES[k][1] for k in SEQUENCE]))) > 1     # the lengths really differ from the grids'
    starts = np.concatenate(([0], np.cumsum(lengths)[:-1]))
    assert [s.start_frame for s in walk.steps] == starts.tolist()
    assert [s.end_frame for s in walk.steps] == (starts + np.array(lengths) - 1).tolist()
    assert walk.get_num_of_frames() == sum(lengths)
    assert not np.isnan(walk.get_quat_frames()).any()


def test_rebuilding_from_a_later_step_keeps_the_prefix():
    _, walk = stub_walk(start_pose=START_POSE)
    walk.convert_graph_walk_to_quaternion_frames()
    before = walk.get_quat_frames().copy()
    ranges = [(s.start_frame, s.end_frame) for s in walk.steps]
    new = np.array(walk.get_global_spatial_parameter_vector(2)) + 0.25
    walk.update_spatial_parameters(new, start_step=2)
    walk.convert_graph_walk_to_quaternion_frames(start_step=2)
    after = walk.get_quat_frames()
    cut = walk.steps[2].start_frame
    assert [(s.start_frame, s.end_frame) for s in walk.steps] == ranges
    assert np.array_equal(after[:cut], before[:cut]) and not np.allclose(after[cut:], before[cut:])
    # the rebuilt part is a walk of its own aligned to the last kept frame
    nodes = [walk.motion_state_graph.nodes[s.node_key] for s in walk.steps[2:]]
    al = gw._ROOT_ONLY.alignment_to(before[cut - 1])
    ref, _, _ = gw.assemble_walk_host(nodes, new[None, :], alignment=al)
    assert np.array_equal(after[cut:], ref[0])


def test_parameter_vectors_round_trip():
    _, walk = stub_walk(n_time=2)
    spatial, time = walk.get_global_spatial_parameter_vector(), walk.get_global_time_parameter_vector()
    assert len(spatial) == sum(SHAPES[k][0] for k in SEQUENCE) and len(time) == 2 * len(SEQUENCE)
    walk.update_spatial_parameters(np.arange(len(spatial), dtype=np.float64))
    walk.update_time_parameters(-np.arange(len(time), dtype=np.float64), 0, len(walk.steps))
    assert walk.get_global_spatial_parameter_vector() == list(range(len(spatial)))
    assert walk.get_global_time_parameter_vector() == [-float(v) for v in range(len(time))]
    tail = walk.get_global_spatial_parameter_vector(4)
    walk.update_spatial_parameters(np.array(tail) + 1.0, start_step=4)
    assert walk.get_global_spatial_parameter_vector(4) == [v + 1.0 for v in tail]
    assert walk.get_global_spatial_parameter_vector()[:len(spatial) - len(tail)] == list(range(len(spatial) - len(tail)))


def test_step_from_keyframe_is_the_last_match():
    _, walk = stub_walk()
    walk.convert_graph_walk_to_quaternion_frames()
    assert walk.get_step_from_keyframe(0) == 0
    assert walk.get_step_from_keyframe(walk.steps[3].start_frame) == 3
    assert walk.get_step_from_keyframe(walk.get_num_of_frames()) == -1
    walk.steps[1].start_frame = walk.steps[0].end_frame          # two steps hold the keyframe: the reference's loop keeps the last
    assert walk.get_step_from_keyframe(walk.steps[0].end_frame) == 1


def test_json_round_trip():
    graph, walk = stub_walk(n_time=1, start_pose=START_POSE)
    walk.convert_graph_walk_to_quaternion_frames()
    data = json.loads(json.dumps(walk.to_json()))
    back = gw.HipGraphWalk.from_json(graph, data, host=True)
    assert back.start_pose == START_POSE and len(back.steps) == len(walk.steps)
    for a, b in zip(walk.steps, back.steps):
        assert a.node_key == b.node_key and np.array_equal(a.parameters, b.parameters)
        assert (a.start_frame, a.end_frame, a.n_spatial_components, a.n_time_components) == (b.start_frame, b.end_frame, b.n_spatial_components, b.n_time_components)
    back.convert_graph_walk_to_quaternion_frames()
    assert np.array_equal(back.get_quat_frames(), walk.get_quat_frames())
