"""mg_pca_fit_leading (csrc/mg_fpca.hip) against pca_leading_host (numpy.linalg.svd) on small shapes of ranks 1, 3 and full, its
reproducibility, its cap, one shape beyond mg_pca_fit's limit with a known answer, and HipClusterTreeBuilder's device_features route.

The tolerances.  On every input the test first measures how far mg_pca_fit -- the existing one-sided Jacobi, which forms
no Gram matrix -- lies from numpy's SVD: `spread` of the singular values (relative) and of the vectors (| |V V_ref^T| - I |).  The code
under test iterates on Xc^T Xc, whose eigenvalues are the squares: a singular value s_i comes out with a relative error of the order of
eps (s_1 / s_i)^2, so the values' bound is 8 x (s_1 / s_k)^2 x max(spread, eps); a vector's error is its residual over the gap of its
eigenvalue to the next, so the vectors' bound is 8 x (tol + spread) / (smallest gap among the kept eigenvalues and the first one not
kept, over lambda_1), tol the library's residual bound 64 eps sqrt(max(n, p)).  Conditioning and gaps are numpy's, not the code's."""
import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import cluster_tree_builder as ctb
from morphablegraphs_amd.cluster_tree_sampling import HipClusterTreeSampler, pca_leading_host
from morphablegraphs_amd.motion_primitive_wrapper import HipMotionPrimitiveModelWrapper

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
FRACTION = 0.95
COUNT_MARGIN = 1e-6


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def gapped_matrix(seed, n, p, rank, decay=0.8):
    rng = np.random.default_rng(seed)
    r = min(rank, n, p)
    U, _ = np.linalg.qr(rng.standard_normal((n, r)))
    V, _ = np.linalg.qr(rng.standard_normal((p, r)))
    return (U * (10.0 * decay ** np.arange(r))) @ V.T + rng.standard_normal(p)


def fit_leading(ctx, X, fraction=FRACTION, **kw):
    n, p = X.shape
    with ctx.buffers() as bufs:
        d_x, d_c = bufs.upload(X), bufs.malloc(8 * n * p)
        return _capi.pca_fit_leading(ctx, d_x, n, p, d_c, fraction, **kw)


def fit_jacobi(ctx, X):
    n, p = X.shape
    with ctx.buffers() as bufs:
        d_x, d_c = bufs.upload(X), bufs.malloc(8 * n * p)
        return _capi.pca_fit(ctx, d_x, n, p, d_c)


def bounds(ctx, X, ref):
    """(values' bound, vectors' bound) for X from the measured spread of mg_pca_fit against numpy, as the module's docstring derives them."""
    n, p = X.shape
    k = ref["k"]
    s_all = np.linalg.svd(X - X.mean(axis=0), compute_uv=False)
    jac = fit_jacobi(ctx, X)
    spread_s = float(np.max(np.abs(jac["singular_values"][:k] - s_all[:k]) / s_all[:k]))
    spread_v = float(np.max(np.abs(np.abs(jac["vt"][:k] @ ref["vt"].T) - np.eye(k))))
    lam = s_all ** 2
    edge = lam[:k + 1] if k < len(lam) else np.append(lam[:k], 0.0)
    gap = float(np.min(edge[:-1] - edge[1:]) / lam[0])
    tol = 64.0 * EPS * np.sqrt(max(n, p))
    cond2 = float(lam[0] / lam[k - 1])
    values, vectors = 8.0 * cond2 * max(spread_s, EPS), 8.0 * (tol + spread_v) / gap
    print("shape %s k %d: spread of mg_pca_fit against numpy %.3g (values) %.3g (vectors); (s_1/s_k)^2 %.3g, gap %.3g -> bounds %.3g, %.3g"
          % (X.shape, k, spread_s, spread_v, cond2, gap, values, vectors))
    return values, vectors


@pytest.mark.parametrize("rank", [1, 3, None], ids=["rank1", "rank3", "full"])
@pytest.mark.parametrize("shape", [(40, 12), (12, 40), (257, 130), (513, 70)], ids=lambda s: "%dx%d" % s)
def test_against_numpys_svd(ctx, shape, rank):
    n, p = shape
    X = gapped_matrix(n + p + (rank or 0), n, p, rank or min(n, p))
    ref = pca_leading_host(X, FRACTION)
    s_all = np.linalg.svd(X - X.mean(axis=0), compute_uv=False)
    cum = np.cumsum(s_all ** 2 / np.sum(s_all ** 2))
    assert np.min(np.abs(cum - FRACTION)) > COUNT_MARGIN                  # the count rule has a clear answer
    values, vectors = bounds(ctx, X, ref)
    got = fit_leading(ctx, X)
    k = ref["k"]
    err_s = float(np.max(np.abs(got["singular_values"][:k] - ref["singular_values"][:min(k, got["k"])]) / ref["singular_values"])) if got["k"] == k else np.inf
    print("   mg_pca_fit_leading: k %d, %d iterations, status %d, values off by %.3g" % (got["k"], got["iterations"], got["status"], err_s))
    assert got["k"] == k and got["status"] == 1
    np.testing.assert_allclose(got["singular_values"], ref["singular_values"], rtol=values)
    np.testing.assert_allclose(got["ratios"], ref["ratios"], rtol=2.0 * values)
    np.testing.assert_allclose(got["mean"], ref["mean"], rtol=0, atol=64 * EPS * np.abs(X).max())
    off = float(np.max(np.abs(np.abs(got["vt"] @ ref["vt"].T) - np.eye(k))))
    print("   vectors off by %.3g" % off)
    assert off <= vectors
    for row in got["vt"]:                                                   # mg_pca_fit's sign rule
        assert row[int(np.argmax(np.abs(row)))] > 0.0


def test_two_calls_give_the_same_bits(ctx):
    X = gapped_matrix(4, 257, 130, 3)
    a, b = fit_leading(ctx, X), fit_leading(ctx, X)
    assert a["k"] == b["k"] and a["iterations"] == b["iterations"] and a["status"] == b["status"]
    for key in ("mean", "singular_values", "vt", "ratios"):
        assert np.array_equal(a[key].view(np.uint64), b[key].view(np.uint64)), key


def test_the_cap_is_reported(ctx):
    X = gapped_matrix(6, 257, 130, 130, decay=0.99)                        # a slow gap: neighbours differ by two per cent
    got = fit_leading(ctx, X, max_iterations=1)
    assert got["status"] == 2 and got["iterations"] == 1 and got["k"] >= 1
    assert np.all(np.isfinite(got["vt"])) and np.all(np.isfinite(got["singular_values"]))


def test_misuse(ctx):
    X = gapped_matrix(8, 20, 10, 3)
    for fraction in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(_capi.MGError) as e:
            fit_leading(ctx, X, fraction=fraction)
        assert e.value.status == _capi.MG_ERR_INVALID_ARGUMENT
    Y = X.copy()
    Y[3, 4] = np.inf
    with pytest.raises(_capi.MGError) as e:
        fit_leading(ctx, Y)
    assert e.value.status == _capi.MG_ERR_INVALID_ARGUMENT


def test_a_shape_beyond_jacobis_limit(ctx):
    """(4097, 4097) = U diag(30, 20, 10) V^T + mean, U's columns orthonormal and orthogonal to the ones vector (so centring leaves the
    singular values as constructed): lambda / total = 9/14, 4/14, 1/14 -> three components for 0.95.  No host SVD of that size."""
    n = p = 4097
    rng = np.random.default_rng(12)
    U = np.linalg.qr(np.column_stack((np.ones(n), rng.standard_normal((n, 3)))))[0][:, 1:]
    V = np.linalg.qr(rng.standard_normal((p, 3)))[0]
    s = np.array([30.0, 20.0, 10.0])
    mean = rng.standard_normal(p)
    X = (U * s) @ V.T + mean
    with ctx.buffers() as bufs:
        d_x, d_c = bufs.upload(X), bufs.malloc(8 * n * p)
        with pytest.raises(_capi.MGError) as e:
            _capi.pca_fit(ctx, d_x, n, p, d_c)
        assert e.value.status == _capi.MG_ERR_UNSUPPORTED
        got = _capi.pca_fit_leading(ctx, d_x, n, p, d_c, FRACTION)
    print("4097 x 4097: k %d, %d iterations, status %d, values %r" % (got["k"], got["iterations"], got["status"], got["singular_values"]))
    assert got["k"] == 3 and got["status"] == 1
    # the construction rounds at eps |X| ~ eps 30 per entry; (s_1 / s_3)^2 = 9 in the Gram form
    np.testing.assert_allclose(got["singular_values"], s, rtol=8 * 9 * 64 * EPS * np.sqrt(n))
    np.testing.assert_allclose(got["ratios"], s ** 2 / np.sum(s ** 2), rtol=16 * 9 * 64 * EPS * np.sqrt(n))
    np.testing.assert_allclose(got["mean"], mean, rtol=0, atol=1e-12)
    # gaps of 5/9 and 3/9 of lambda_1: the vectors are V's columns up to sign
    assert float(np.max(np.abs(np.abs(got["vt"] @ V) - np.eye(3)))) <= 8 * 64 * EPS * np.sqrt(n) * 3.0 + 1e-12


def test_the_builder_with_device_features():
    joints, animated = synthetic.make_skeleton()
    sk = _capi.Skeleton(joints, animated)
    data = synthetic.make_primitive(seed=3, n_components=6, n_frames=20, n_basis=8, n_dim=79, n_gmm=2, name="small")
    w = HipMotionPrimitiveModelWrapper()
    w._initialize_from_json(None, data)
    names = ["LeftHand_EndSite", "RightHand_EndSite", "Head_EndSite", "LeftFoot", "RightFoot", "Hips"]
    settings = {"tree_type": ctb.TREE_TYPE_FEATURE_CLUSTER_TREE, "feature_type": ctb.FEATURE_TYPE_EUCLIDEAN_PCA, "output_mode": "json"}
    config = {"model_data_dir": None, "n_random_samples": 300, "n_subdivisions_per_level": 4, "n_levels": 3, "random_seed": 5,
              "only_spatial_parameters": True, "store_data_indices_in_nodes": False, "use_kd_tree": True}
    builder = ctb.HipClusterTreeBuilder(settings)
    assert builder.device_features is False
    builder.set_config(config)
    assert builder.device_features is False
    builder.skeleton, builder.joint_names = sk, names
    sampler = HipClusterTreeSampler(300)
    np.random.seed(2)
    S = np.asarray(sampler.sample_data(w), dtype=np.float64)
    assert S.shape[0] == 300
    # device_features = False: the route as it was
    before = sampler._extract_features(w, S, "euclidean_pca", sk, names, step=1)
    np.testing.assert_array_equal(builder._extract_features(w, S), before)
    # device_features = True (through the config key)
    builder.set_config(dict(config, device_features=True))
    assert builder.device_features is True
    feats = builder._extract_features(w, S)
    clouds = sampler.map_motions_to_euclidean_space(w, sampler._back_project(w, S), sk, names, step=1)
    ref = pca_leading_host(clouds, FRACTION)
    want = (clouds - ref["mean"]) @ ref["vt"].T
    ctx = w.motion_primitive._prim.ctx
    values, vectors = bounds(ctx, clouds, ref)
    assert feats.shape == want.shape
    off = float(np.abs(feats - want).max())
    print("features off by %.3g of %.3g" % (off, ref["singular_values"][0]))
    assert off <= vectors * ref["singular_values"][0]
    feats2, model = sampler.map_to_euclidean_pca_on_device(w, S, sk, names, step=1)
    np.testing.assert_array_equal(feats2, feats)
    assert model.n_components_ == ref["k"] and model.components_.shape == ref["vt"].shape
    np.testing.assert_allclose(model.explained_variance_ratio_, ref["ratios"], rtol=2.0 * values)
    np.testing.assert_allclose(model.transform(clouds[:7]), feats[:7], rtol=0, atol=64 * EPS * ref["singular_values"][0] * np.sqrt(clouds.shape[1]))
    tree = builder._build_feature_tree(None, None, S, w)
    tree.validate(w.get_n_spatial_components())
