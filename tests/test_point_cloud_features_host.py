"""The NumPy statements beside the device route of the "euclidean_pca" features (cluster_tree_sampling.py): point_clouds_host against the
reference's repeat rule written out (space_partitioning/features.py:139-150), pca_leading_host against sklearn's PCA with a float
n_components."""
import numpy as np
import pytest

from morphablegraphs_amd.cluster_tree_sampling import pca_leading_host, point_clouds_host

FRACTIONS = (0.95, 0.6)
COUNT_MARGIN = 1e-6            # the cumulative ratio stays this far from the fraction: the count is then no coin toss


@pytest.mark.parametrize("step", [1, 3, 4])
def test_point_clouds_host_repeats_the_last_kept_frame(step):
    rng = np.random.default_rng(5)
    n, F, J = 2, 7, 2                                   # F is a multiple of none of the steps but 1
    pos = rng.standard_normal((n, F, J, 3))
    want = []
    for i in range(n):                                  # features.py:139-150: `frame` is recomputed where idx % step == 0, appended always
        sample, frame = [], None
        for idx in range(F):
            if idx % step == 0:
                frame = pos[i, idx].reshape(-1)
            sample.append(frame)
        want.append(np.concatenate(sample))
    got = point_clouds_host(pos, step)
    assert got.shape == (n, F * J * 3)
    np.testing.assert_array_equal(got, np.asarray(want))


def test_point_clouds_host_refuses_a_bad_shape_or_step():
    with pytest.raises(ValueError):
        point_clouds_host(np.zeros((2, 3, 4)), 1)
    with pytest.raises(ValueError):
        point_clouds_host(np.zeros((2, 3, 4, 3)), 0)


def gapped_matrix(seed, n, p, rank):
    """U diag(s) V^T + mean with s falling by a fifth per component: clear gaps everywhere."""
    rng = np.random.default_rng(seed)
    r = min(rank, n, p)
    U, _ = np.linalg.qr(rng.standard_normal((n, r)))
    V, _ = np.linalg.qr(rng.standard_normal((p, r)))
    s = 10.0 * 0.8 ** np.arange(r)
    return (U * s) @ V.T + rng.standard_normal(p)


@pytest.mark.parametrize("fraction", FRACTIONS)
@pytest.mark.parametrize("shape,rank", [((40, 12), 12), ((12, 40), 3), ((60, 33), 1), ((90, 25), 25)])
def test_pca_leading_host_against_sklearn(shape, rank, fraction):
    from sklearn.decomposition import PCA
    X = gapped_matrix(shape[0] + rank, shape[0], shape[1], rank)
    ref = PCA(n_components=fraction, svd_solver="full").fit(X)
    full = PCA(svd_solver="full").fit(X)
    cum = np.cumsum(full.explained_variance_ratio_)
    assert np.min(np.abs(cum - fraction)) > COUNT_MARGIN          # the precondition: the count rule has a clear answer
    got = pca_leading_host(X, fraction)
    k = int(ref.n_components_)
    assert got["k"] == k and got["vt"].shape == (k, shape[1])
    eps = np.finfo(np.float64).eps
    np.testing.assert_allclose(got["ratios"], ref.explained_variance_ratio_, rtol=64 * eps, atol=64 * eps)
    np.testing.assert_allclose(got["singular_values"], ref.singular_values_, rtol=64 * eps)
    np.testing.assert_allclose(got["mean"], ref.mean_, rtol=0, atol=64 * eps * np.abs(X).max())
    # both are LAPACK's vectors of the same centred matrix: equal up to sign and round-off
    np.testing.assert_allclose(np.abs(got["vt"] @ ref.components_.T), np.eye(k), rtol=0, atol=1e-12)
    for row in got["vt"]:                                           # mg_pca_fit's sign rule
        assert row[int(np.argmax(np.abs(row)))] > 0.0
