"""motion_state_graph.step_lengths_host: the NumPy statement of mg_step_lengths' two reductions (sequential arc length on the
ground plane, distance between the first and the last root position), against the existing host formulas on the reference's own
frames.  No device."""
import numpy as np
import pytest

from conftest import GOLDEN_CASES, load_golden
from morphablegraphs_amd.motion_state_graph import arc_length_xz, step_lengths_host


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_step_lengths_host_agrees_with_the_existing_formulas_on_the_reference_frames(name):
    frames = load_golden(name)["frames"]
    root = frames[:, :, :3]
    F = root.shape[1]
    arc, dist = step_lengths_host(root)
    assert arc.shape == dist.shape == (len(root),) and arc.dtype == dist.dtype == np.float64
    # the summation order is the only difference: F terms, each within an ulp of the running sum
    rtol = F * 2.0 ** -52
    np.testing.assert_allclose(arc, arc_length_xz(root), rtol=rtol, atol=0)
    np.testing.assert_allclose(dist, np.linalg.norm(frames[:, -1, :3] - frames[:, 0, :3], axis=1), rtol=rtol, atol=0)
    # one path alone: the same bits as inside the batch
    a0, d0 = step_lengths_host(root[0])
    assert a0 == arc[0] and d0 == dist[0]


def test_the_arc_length_is_added_in_frame_order():
    """One segment of length 1, then 64 of 2^-58 along z: added one after the other from d_1 every small one is lost
    (1 + 2^-58 rounds to 1), although together they are an ulp of the total, which a pairwise sum keeps."""
    root = np.zeros((66, 3))
    root[1:, 0] = 1.0
    root[1:, 2] = 2.0 ** -58 * np.arange(65)
    arc, dist = step_lengths_host(root)
    assert arc == 1.0
    assert dist == np.sqrt(1.0 + (2.0 ** -52) ** 2)


def test_a_constant_path_has_length_zero_and_a_nan_position_gives_nan():
    root = np.tile(np.array([3.5, -1.25, 7.0]), (4, 9, 1))
    arc, dist = step_lengths_host(root)
    assert np.array_equal(arc, np.zeros(4)) and np.array_equal(dist, np.zeros(4))
    root[2, 5, 2] = np.nan
    arc, dist = step_lengths_host(root)
    assert np.isnan(arc[2]) and not np.isnan(arc[[0, 1, 3]]).any()
    root[2, 0, 1] = np.nan
    assert np.isnan(step_lengths_host(root)[1][2])
    # a single frame: no segment, no displacement
    arc, dist = step_lengths_host(np.ones((2, 1, 3)))
    assert np.array_equal(arc, np.zeros(2)) and np.array_equal(dist, np.zeros(2))
