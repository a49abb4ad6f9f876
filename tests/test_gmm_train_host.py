"""The GMM trainer's host side against the reference's GMMTrainer as recorded in tests/golden/gmm_train.npz
(tools/gen_gmm_train_golden.py): the NumPy restatement of sklearn's EM from the recorded KMeans labels reproduces every
fit of the sweep and the refit; the AIC choice, averageScore, the JSON shape and the trainer's quirks.

Tolerance, per quantity q and per fit: |ours - sklearn| <= 10 * max(spread_q, 1e-13 * max|q_sklearn|), spread_q being the
largest difference sklearn itself shows when the same fit runs on 3 row permutations of its data."""
import os

import numpy as np
import pytest

from morphablegraphs_amd import gmm_trainer as gt

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "gmm_train.npz")
FACTOR, FLOOR = 10.0, 1e-13


def load():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


G = load()
CASES = list(range(len(G["names"])))


def case(i):
    p = "c%d_" % i
    return {k[len(p):]: v for k, v in G.items() if k.startswith(p)}


def fit_data(c, j):
    """The data fit j saw: the shuffled rows in the sweep, the rows themselves in the refit."""
    return c["data"] if c["fit_refit"][j] else c["data"][c["perm"]]


def close(name, ours, ref, spread):
    ours, ref = np.asarray(ours, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert ours.shape == ref.shape, name
    bound = FACTOR * max(float(spread), FLOOR * float(np.max(np.abs(ref))))
    err = float(np.max(np.abs(ours - ref))) if ref.size else 0.0
    print("%-28s err %.3e bound %.3e" % (name, err, bound))
    assert err <= bound, "%s: |ours - sklearn| = %.3e > %.3e" % (name, err, bound)


def params_of(c):
    """fit index -> {quantity: recorded value} of the fits whose parameters were recorded (weights and means of
    param_fit, covariances and precision Cholesky factors of cov_fit)."""
    out = {}
    for fits, keys in ((c["param_fit"], ("weights", "means")), (c["cov_fit"], ("covariances", "precisions_cholesky"))):
        c0 = 0
        for j in fits:
            K = int(c["fit_k"][j])
            for key in keys:
                out.setdefault(int(j), {})[key] = c["p_" + key.replace("precisions_cholesky", "precisions")][c0:c0 + K]
            c0 += K
    return out


def check_fit(c, j, fit, name, converged=None):
    K, n_iter = int(c["fit_k"][j]), int(c["n_iter"][j])
    assert fit["n_iter"] == n_iter, "%s: n_iter %d, sklearn %d" % (name, fit["n_iter"], n_iter)
    got_conv = fit["converged"] if converged is None else converged
    assert bool(got_conv) == bool(c["converged"][j]), name
    close(name + " lower bounds", fit["lower_bounds"], c["lb"][j, :n_iter], c["spread_lb"][j])
    close(name + " score", fit["score"], c["score"][j], c["spread_score"][j])
    n = len(c["data"])
    aic = -2 * fit["score"] * n + 2 * gt.n_parameters(K, c["data"].shape[1])
    close(name + " aic", aic, c["aic"][j], c["spread_aic"][j])
    for key, ref in params_of(c).get(j, {}).items():
        sk = {"precisions_cholesky": "precisions"}.get(key, key)
        close("%s %s" % (name, key), fit[key], ref, c["spread_" + sk][j])


@pytest.mark.parametrize("i", CASES)
def test_host_em_reproduces_every_recorded_fit(i):
    c = case(i)
    for j in range(len(c["fit_k"])):
        K = int(c["fit_k"][j])
        fit = gt.em_from_labels_host(fit_data(c, j), c["km_labels"][j].astype(np.int64), K)
        check_fit(c, j, fit, "%s K=%d%s" % (c["name"], K, " refit" if c["fit_refit"][j] else ""))


@pytest.mark.parametrize("i", CASES)
def test_host_aic_choice_and_average_score(i):
    c = case(i)
    n = len(c["data"])
    sweep = np.flatnonzero(c["fit_refit"] == 0)
    aics = []
    for j in sweep:
        fit = gt.em_from_labels_host(fit_data(c, j), c["km_labels"][j].astype(np.int64), int(c["fit_k"][j]))
        aics.append(-2 * fit["score"] * n + 2 * gt.n_parameters(int(c["fit_k"][j]), c["data"].shape[1]))
    chosen = min(range(len(aics)), key=aics.__getitem__) + 1
    assert chosen == int(c["chosen"])
    j = int(np.flatnonzero(c["fit_refit"] == 1)[0])
    assert int(c["fit_k"][j]) == chosen
    refit = gt.em_from_labels_host(c["data"], c["km_labels"][j].astype(np.int64), chosen)
    close("averageScore", refit["score"], c["average_score"], c["spread_score"][j])


def test_n_k_clamp_case_is_recorded():
    """n = 30 < 40: the reference sweeps K = 1 .. n - 1."""
    c = case([str(x) for x in G["names"]].index("n30_d4"))
    assert list(c["fit_k"][c["fit_refit"] == 0]) == list(range(1, 30))


class _FakeFit(object):
    def __init__(self, K, d, n):
        rng = np.random.default_rng(K)
        self.weights_ = np.full(K, 1.0 / K)
        self.means_ = rng.standard_normal((K, d))
        self.covariances_ = np.stack([np.eye(d)] * K)
        self.train_score_ = -float(K)
        self.n_components = K

    def train_aic(self, n):
        return [5.0, 3.0, 3.0, 4.0][self.n_components - 1]


def test_trainer_quirks(monkeypatch):
    calls = []

    def fake_fit(X, n_components, init=None, seed=0, ctx=None, **kw):
        calls.append((np.array(X), n_components, seed))
        if np.ndim(n_components) == 0:
            return _FakeFit(int(n_components), X.shape[1], len(X))
        return [_FakeFit(K, X.shape[1], len(X)) for K in n_components]
    monkeypatch.setattr(gt, "fit_gaussian_mixtures", fake_fit)
    data = np.arange(15.0).reshape(5, 3)
    with pytest.raises(AssertionError):
        gt.HipGMMTrainer(seed=1).fit(data[0])
    np.random.seed(3)
    expect = np.random.permutation(data)
    np.random.seed(3)
    tr = gt.HipGMMTrainer(seed=1)
    tr.fit(data)
    # the sweep sees np.random.permutation(data) and K = 1 .. n - 1; the first minimum wins; the refit sees the data
    assert np.array_equal(calls[0][0], expect) and calls[0][1] == [1, 2, 3, 4]
    assert tr.numberOfGaussian == 2
    assert np.array_equal(calls[1][0], data) and calls[1][1] == 2
    assert tr.averageScore == -2.0
    js = tr.convert_model_to_json()
    assert sorted(js) == ["gmm_covars", "gmm_means", "gmm_weights"]
    assert np.array(js["gmm_weights"]).shape == (2,) and np.array(js["gmm_means"]).shape == (2, 3)
    assert np.array(js["gmm_covars"]).shape == (2, 3, 3)
    assert isinstance(js["gmm_covars"][0][0], list)


def test_trainer_seed_drawn_after_the_shuffle(monkeypatch):
    monkeypatch.setattr(gt, "fit_gaussian_mixtures", lambda X, n_components, **kw: (
        _FakeFit(int(n_components), X.shape[1], len(X)) if np.ndim(n_components) == 0 else [_FakeFit(K, X.shape[1], len(X)) for K in n_components]))
    data = np.arange(15.0).reshape(5, 3)
    np.random.seed(9)
    np.random.permutation(data)
    expect = int(np.random.randint(0, 2 ** 31 - 1))
    np.random.seed(9)
    tr = gt.HipGMMTrainer()
    tr.fit(data)
    assert tr.seed == expect


def test_host_em_ill_defined_raises():
    X = 1e160 * (1.0 + np.random.default_rng(7).random((24, 3)))
    with pytest.raises(ValueError):
        gt.em_from_labels_host(X, np.zeros(24, dtype=np.int64), 1)


def test_n_parameters_matches_sklearn_formula():
    K, d = 7, 5
    assert gt.n_parameters(K, d) == int(K * d * (d + 1) / 2.0 + d * K + K - 1) == 7 * 15 + 35 + 6
