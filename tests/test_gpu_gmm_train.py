"""The device GMM trainer (mg_gmm_em_fit, gmm_trainer.fit_gaussian_mixtures / HipGMMTrainer) against the reference's
GMMTrainer as recorded in tests/golden/gmm_train.npz, with the tolerance rule of tests/test_gmm_train_host.py: per
quantity and fit, |ours - sklearn| <= 10 * max(spread_q, 1e-13 * max|q_sklearn|)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gmm_train_host import CASES, G, case, check_fit, close, fit_data, params_of  # noqa: E402

from morphablegraphs_amd import _capi, synthetic  # noqa: E402
from morphablegraphs_amd import gmm_trainer as gt  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from morphablegraphs_amd.motion_primitive import get_context
    return get_context(0)


def init_centres(c, j, X):
    a, b = c["km_offsets"][j], c["km_offsets"][j + 1]
    return X[c["km_init_idx"][a:b]]


def device_fit(ctx, c, js):
    """The fits js (all on the same data) from their recorded labels in one call."""
    X = fit_data(c, js[0])
    Ks = [int(c["fit_k"][j]) for j in js]
    return gt.fit_gaussian_mixtures(X, Ks, init=[c["km_labels"][j] for j in js], ctx=ctx)


def as_dict(g):
    return {"weights": g.weights_, "means": g.means_, "covariances": g.covariances_, "precisions_cholesky": g.precisions_cholesky_,
            "lower_bounds": np.array(g.lower_bounds_), "n_iter": g.n_iter_, "converged": g.converged_, "score": g.train_score_}


@pytest.mark.parametrize("i", CASES)
def test_kmeans_from_recorded_centres_gives_recorded_labels(ctx, i):
    c = case(i)
    for j in range(len(c["fit_k"])):
        K = int(c["fit_k"][j])
        if K < 2:
            continue
        X = fit_data(c, j)
        dev = ctx.upload(X)
        try:
            lab, _, _, n_iter = _capi.kmeans_segments(ctx, dev, len(X), X.shape[1], [0, len(X)], np.arange(len(X)), K, 1,
                                                      init_centres(c, j, X)[None], None, 0, 300, 1e-4)
        finally:
            dev.free()
        assert np.array_equal(lab, c["km_labels"][j]), "%s K=%d" % (c["name"], K)


@pytest.mark.parametrize("i", CASES)
def test_device_em_matches_every_recorded_fit(ctx, i):
    c = case(i)
    sweep = list(np.flatnonzero(c["fit_refit"] == 0))
    refit = list(np.flatnonzero(c["fit_refit"] == 1))
    for js in (sweep, refit):
        for j, g in zip(js, device_fit(ctx, c, js)):
            check_fit(c, j, as_dict(g), "%s K=%d%s device" % (c["name"], int(c["fit_k"][j]), " refit" if c["fit_refit"][j] else ""))


@pytest.mark.parametrize("i", CASES)
def test_trainer_from_recorded_centres(ctx, i):
    c = case(i)
    data = c["data"]
    obs = data[c["perm"]]
    sweep_j = {int(c["fit_k"][j]): j for j in np.flatnonzero(c["fit_refit"] == 0)}
    refit_j = int(np.flatnonzero(c["fit_refit"] == 1)[0])

    def init(X, K):
        if np.array_equal(X, obs):
            return init_centres(c, sweep_j[K], X)
        assert np.array_equal(X, data) and K == int(c["fit_k"][refit_j])
        return init_centres(c, refit_j, X)
    np.random.seed(int(c["seed"]))
    tr = gt.HipGMMTrainer(seed=0, init=init, ctx=ctx)
    tr.fit(data)
    assert tr.numberOfGaussian == int(c["chosen"])
    close("averageScore", tr.averageScore, c["average_score"], c["spread_score"][refit_j])
    js = tr.convert_model_to_json()
    rec = params_of(c)[refit_j]
    close("gmm_weights", js["gmm_weights"], rec["weights"], c["spread_weights"][refit_j])
    close("gmm_means", js["gmm_means"], rec["means"], c["spread_means"][refit_j])
    if "covariances" in rec:
        close("gmm_covars", js["gmm_covars"], rec["covariances"], c["spread_covariances"][refit_j])
    assert np.array(js["gmm_covars"]).shape == (tr.numberOfGaussian, data.shape[1], data.shape[1])


def _bytes(fits):
    return b"".join(np.ascontiguousarray(a).tobytes() for g in fits for a in
                    (g.weights_, g.means_, g.covariances_, g.precisions_cholesky_, np.array(g.lower_bounds_), g.labels_,
                     np.array([g.train_score_, g.n_iter_])))


def test_determinism_and_batch_independence(ctx):
    c = case(0)
    js = list(np.flatnonzero(c["fit_refit"] == 0))
    a = device_fit(ctx, c, js)
    b = device_fit(ctx, c, js)
    assert _bytes(a) == _bytes(b)
    for j, g in zip(js, a):
        alone = device_fit(ctx, c, [j])
        assert _bytes(alone) == _bytes([g]), "K=%d alone differs from the batch" % int(c["fit_k"][j])


def test_device_seeded_path(ctx):
    """init=None: device k-means++ labels; each fit against the host EM from its own initial labels, the spread measured
    by the host EM on 3 row permutations (labels permuted with the rows)."""
    X = case(0)["data"]
    Ks = [1, 2, 3, 5, 8]
    a = gt.fit_gaussian_mixtures(X, Ks, seed=11, ctx=ctx)
    b = gt.fit_gaussian_mixtures(X, Ks, seed=11, ctx=ctx)
    assert _bytes(a) == _bytes(b)
    rng = np.random.default_rng(5)
    for K, g in zip(Ks, a):
        assert g.converged_ or g.n_iter_ == 100
        assert abs(g.weights_.sum() - 1.0) <= 1e-12
        for cov in g.covariances_:
            assert np.array_equal(cov, cov.T)
            np.linalg.cholesky(cov)
        ref = gt.em_from_labels_host(X, g.init_labels_, K)
        spread = dict.fromkeys(("weights", "means", "covariances", "precisions_cholesky", "lower_bounds", "score"), 0.0)
        for _ in range(3):
            p = rng.permutation(len(X))
            q = gt.em_from_labels_host(X[p], g.init_labels_[p], K)
            assert q["n_iter"] == ref["n_iter"]
            for key in spread:
                spread[key] = max(spread[key], float(np.max(np.abs(np.asarray(q[key]) - np.asarray(ref[key])))))
        assert g.n_iter_ == ref["n_iter"] and g.converged_ == ref["converged"]
        mine = as_dict(g)
        for key in spread:
            close("seeded K=%d %s" % (K, key), mine[key], ref[key], spread[key])


def test_overflowing_rows_raise_and_the_context_survives(ctx):
    X = G["overflow_data"]
    assert list(G["overflow_sklearn_raises"]) == [True, True]
    with pytest.raises(ValueError):
        gt.fit_gaussian_mixtures(X, 1, ctx=ctx)
    with pytest.raises(ValueError):
        gt.fit_gaussian_mixtures(X, [3], init=[G["overflow_labels3"]], ctx=ctx)
    g = gt.fit_gaussian_mixtures(case(1)["data"], 2, seed=1, ctx=ctx)
    assert abs(g.weights_.sum() - 1.0) <= 1e-12


def test_trained_mixture_feeds_log_prob(ctx):
    """Case 3's refit (d = 40) in place of walk_seed0's mixture: mg_gmm_log_prob against the trainer's score_samples."""
    c = case([str(x) for x in G["names"]].index("walk_n600_d40"))
    j = int(np.flatnonzero(c["fit_refit"] == 1)[0])
    g = device_fit(ctx, c, [j])[0]
    data = synthetic.make_walk_primitive(seed=0)
    data.update({"gmm_weights": g.weights_.tolist(), "gmm_means": g.means_.tolist(), "gmm_covars": g.covariances_.tolist()})
    prim = _capi.Primitive(ctx, data)
    try:
        lp = prim.gmm_log_prob(c["data"])
    finally:
        prim.close()
    np.testing.assert_allclose(lp, g.score_samples(c["data"]), rtol=1e-9, atol=1e-7)


def test_unsupported_shapes_raise(ctx):
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="features"):
        gt.fit_gaussian_mixtures(rng.standard_normal((100, 65)), 2, ctx=ctx)
    with pytest.raises(ValueError, match="n_components"):
        gt.fit_gaussian_mixtures(rng.standard_normal((100, 4)), [2, 65], ctx=ctx)
    X = rng.standard_normal((100, 65))
    dev = ctx.upload(X)
    try:
        with pytest.raises(_capi.MGError, match="dim"):
            _capi.gmm_em_fit(ctx, dev, 100, 65, [2], np.zeros((1, 100), dtype=np.int32))
        with pytest.raises(_capi.MGError, match="components"):
            _capi.gmm_em_fit(ctx, dev, 100, 4, [65], np.zeros((1, 100), dtype=np.int32))
    finally:
        dev.free()
