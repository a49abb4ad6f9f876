"""Training a motion primitive's Gaussian mixture on the device: the reference's GMMTrainer (construction/motion_primitive/
gmm_trainer.py, called from motion_model_constructor.py:418-429 learn_statistical_model) and the sklearn
GaussianMixture(covariance_type='full') fits it makes.

GMMTrainer shuffles the latents with np.random.permutation, fits a mixture for every K = 1 .. 40 (n - 1 with fewer than 40
samples), keeps the K of least AIC and refits it on the unshuffled data.  Here the 40 fits of the sweep are ONE call of
mg_gmm_em_fit (_capi.gmm_em_fit) and the refit a second: sklearn 1.7's EM statement for statement in float64 (init_params
'kmeans', n_init 1, tol 1e-3, reg_covar 1e-6, max_iter 100), the covariances in sklearn's two-pass form.  The initial labels
come from mg_kmeans_segments (sklearn KMeans semantics, max_iter 300, tol 1e-4) from the device's Philox k-means++ or from
the caller's centres, or are given; K = 1 starts from all zeros.

em_from_labels_host restates the same EM in NumPy (scipy's Cholesky, triangular solve and logsumexp, as sklearn calls them);
it is the yardstick the tests hold the device to.
"""
import json

import numpy as np

from . import _capi

ILL_DEFINED_MESSAGE = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for "
                       "instance caused by singleton or collapsed samples). Try to decrease the number of components, increase "
                       "reg_covar, or scale the input data.")
STATUS_CONVERGED, STATUS_MAX_ITER, STATUS_ILL_DEFINED = _capi.MG_GMM_EM_CONVERGED, _capi.MG_GMM_EM_MAX_ITER, _capi.MG_GMM_EM_ILL_DEFINED
MAX_DIM, MAX_COMPONENTS = _capi.MG_GMM_EM_MAX_DIM, _capi.MG_GMM_EM_MAX_K


# ---- sklearn's full-covariance mixture, restated on the host ------------------------------------------------------------
def _estimate_gaussian_parameters(X, resp, reg_covar):
    nk = resp.sum(axis=0) + 10 * np.finfo(resp.dtype).eps
    means = np.dot(resp.T, X) / nk[:, np.newaxis]
    K, d = means.shape
    cov = np.empty((K, d, d), dtype=X.dtype)
    for k in range(K):
        diff = X - means[k]
        cov[k] = np.dot(resp[:, k] * diff.T, diff) / nk[k]
        cov[k].flat[::d + 1] += reg_covar
    return nk, means, cov


def _compute_precision_cholesky(covariances):
    from scipy import linalg
    K, d, _ = covariances.shape
    prec = np.empty((K, d, d), dtype=covariances.dtype)
    for k, c in enumerate(covariances):
        try:
            chol = linalg.cholesky(c, lower=True)
        except linalg.LinAlgError:
            raise ValueError(ILL_DEFINED_MESSAGE)
        prec[k] = linalg.solve_triangular(chol, np.eye(d, dtype=c.dtype), lower=True).T
    return prec


def _estimate_weighted_log_prob(X, weights, means, prec_chol):
    n, d = X.shape
    K = len(means)
    log_det = np.sum(np.log(prec_chol.reshape(K, -1)[:, ::d + 1]), axis=1)
    log_prob = np.empty((n, K), dtype=X.dtype)
    for k, (mu, pc) in enumerate(zip(means, prec_chol)):
        y = np.dot(X, pc) - np.dot(mu, pc)
        log_prob[:, k] = np.sum(np.square(y), axis=1)
    return -0.5 * (d * np.log(2 * np.pi) + log_prob) + log_det + np.log(weights)


def _estimate_log_prob_resp(X, weights, means, prec_chol):
    from scipy.special import logsumexp
    wlp = _estimate_weighted_log_prob(X, weights, means, prec_chol)
    lpn = logsumexp(wlp, axis=1)
    with np.errstate(under="ignore"):
        log_resp = wlp - lpn[:, np.newaxis]
    return lpn, log_resp


def em_from_labels_host(X, labels, n_components, tol=1e-3, reg_covar=1e-6, max_iter=100):
    """sklearn GaussianMixture(covariance_type='full').fit from the initial labels `labels` (what init_params='kmeans'
    makes of KMeans' labels), op for op in NumPy float64.  Returns the dict _capi.gmm_em_fit returns per fit, with
    `converged` in place of `status`; raises ValueError (sklearn's message) on an ill-defined covariance."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    K = int(n_components)
    resp = np.zeros((n, K))
    resp[np.arange(n), np.asarray(labels, dtype=np.int64)] = 1
    weights, means, cov = _estimate_gaussian_parameters(X, resp, reg_covar)
    weights /= n
    prec = _compute_precision_cholesky(cov)
    lower_bound, lbs, converged, n_iter = -np.inf, [], False, 0
    for n_iter in range(1, max_iter + 1):
        prev = lower_bound
        lpn, log_resp = _estimate_log_prob_resp(X, weights, means, prec)
        weights, means, cov = _estimate_gaussian_parameters(X, np.exp(log_resp), reg_covar)
        weights /= weights.sum()
        prec = _compute_precision_cholesky(cov)
        lower_bound = np.mean(lpn)
        lbs.append(lower_bound)
        if abs(lower_bound - prev) < tol:
            converged = True
            break
    lpn, log_resp = _estimate_log_prob_resp(X, weights, means, prec)
    return {"weights": weights, "means": means, "covariances": cov, "precisions_cholesky": prec, "lower_bounds": np.array(lbs),
            "n_iter": n_iter, "converged": converged, "score": float(np.mean(lpn)), "labels": log_resp.argmax(axis=1)}


def n_parameters(n_components, n_features):
    """GaussianMixture._n_parameters for covariance_type='full'."""
    K, d = int(n_components), int(n_features)
    return int(K * d * (d + 1) / 2.0 + d * K + K - 1)


class FittedGaussianMixture(object):
    """The sklearn-shaped result of one device fit (GaussianMixture's fitted attributes and scoring methods)."""

    covariance_type = "full"

    def __init__(self, fit, init_labels, tol, reg_covar, max_iter):
        self.n_components = len(fit["weights"])
        self.weights_, self.means_ = fit["weights"], fit["means"]
        self.covariances_, self.precisions_cholesky_ = fit["covariances"], fit["precisions_cholesky"]
        self.converged_ = fit["status"] == STATUS_CONVERGED
        self.n_iter_ = fit["n_iter"]
        self.lower_bounds_ = list(fit["lower_bounds"])
        self.lower_bound_ = float(fit["lower_bounds"][-1])
        self.init_labels_ = np.asarray(init_labels)
        self.labels_ = fit["labels"]
        self.train_score_ = fit["score"]          # score(X) of the training data, computed on the device
        self.tol, self.reg_covar, self.max_iter, self.n_init = tol, reg_covar, max_iter, 1

    def _estimate_weighted_log_prob(self, X):
        return _estimate_weighted_log_prob(np.asarray(X, dtype=np.float64), self.weights_, self.means_, self.precisions_cholesky_)

    def score_samples(self, X):
        from scipy.special import logsumexp
        return logsumexp(self._estimate_weighted_log_prob(X), axis=1)

    def score(self, X, y=None):
        return self.score_samples(X).mean()

    def predict(self, X):
        return self._estimate_weighted_log_prob(X).argmax(axis=1)

    def _n_parameters(self):
        return n_parameters(self.n_components, self.means_.shape[1])

    def bic(self, X):
        return -2 * self.score(X) * X.shape[0] + self._n_parameters() * np.log(X.shape[0])

    def aic(self, X):
        return -2 * self.score(X) * X.shape[0] + 2 * self._n_parameters()

    def train_aic(self, n_samples):
        """aic() of the training data from the device's score."""
        return -2 * self.train_score_ * n_samples + 2 * self._n_parameters()

    def train_bic(self, n_samples):
        return -2 * self.train_score_ * n_samples + self._n_parameters() * np.log(n_samples)


def fit_gaussian_mixtures(X, n_components, init=None, seed=0, tol=1e-3, reg_covar=1e-6, max_iter=100, ctx=None, points_dev=None):
    """Fit GaussianMixture(n_components=K, covariance_type='full') for every K of `n_components` (an int or a list) in ONE
    device call.  init: None (device k-means++ keyed by `seed` and K), a callable (X, K) -> (K, d) initial k-means centres,
    or the initial labels (one (n,) array per K).  Returns a FittedGaussianMixture per K (one object for an int)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("Expected 2D array, got %dD array instead" % X.ndim)
    single = np.ndim(n_components) == 0
    Ks = [int(n_components)] if single else [int(k) for k in n_components]
    n, d = X.shape
    if not 1 <= d <= MAX_DIM:
        raise ValueError("fit_gaussian_mixtures: %d features; the device EM supports 1 .. %d" % (d, MAX_DIM))
    for K in Ks:
        if not 1 <= K <= MAX_COMPONENTS:
            raise ValueError("fit_gaussian_mixtures: n_components = %d; the device EM supports 1 .. %d" % (K, MAX_COMPONENTS))
        if n < K:
            raise ValueError("Expected n_samples >= n_components but got n_components = %d, n_samples = %d" % (K, n))
    ctx = _capi.default_context(ctx)
    with ctx.buffers() as bufs:
        if points_dev is None:
            points_dev = bufs.upload(X)
        labels = []
        if init is not None and not callable(init):
            labels = [np.asarray(lab, dtype=np.int32).reshape(n) for lab in init]
            if len(labels) != len(Ks):
                raise ValueError("init: one label array per fit expected, got %d for %d fits" % (len(labels), len(Ks)))
        else:
            everyone = np.arange(n, dtype=np.int64)
            for K in Ks:
                if K == 1:
                    labels.append(np.zeros(n, dtype=np.int32))
                    continue
                centres = None if init is None else np.asarray(init(X, K), dtype=np.float64).reshape(1, K, d)
                lab, _, _, _ = _capi.kmeans_segments(ctx, points_dev, n, d, [0, n], everyone, K, 1, centres,
                                                     np.array([K], dtype=np.uint64), seed, 300, 1e-4)
                labels.append(np.asarray(lab, dtype=np.int32))
        fits = _capi.gmm_em_fit(ctx, points_dev, n, d, Ks, np.stack(labels), tol, reg_covar, max_iter)
    bad = [K for K, f in zip(Ks, fits) if f["status"] == STATUS_ILL_DEFINED]
    if bad:
        raise ValueError(ILL_DEFINED_MESSAGE + " (n_components = %s)" % ", ".join(str(K) for K in bad))
    out = [FittedGaussianMixture(f, lab, tol, reg_covar, max_iter) for f, lab in zip(fits, labels)]
    return out[0] if single else out


class HipGMMTrainer(object):
    """GMMTrainer (reference construction/motion_primitive/gmm_trainer.py) on the device, its quirks kept: fit asserts a
    2-D matrix; the sweep shuffles with np.random.permutation (NumPy's global stream), clamps n_K to n - 1 when there are
    fewer samples, takes the first minimum of the scores; the refit is on the unshuffled data.  seed None draws the
    device k-means++ seed from np.random (as HipGaussianMixture.sample draws its seed); init as fit_gaussian_mixtures
    (a callable gets the shuffled data in the sweep and the data itself in the refit)."""

    def __init__(self, seed=None, init=None, ctx=None):
        self.averageScore = 0
        self.seed, self.init, self.ctx = seed, init, ctx

    def fit(self, data, score='AIC'):
        assert len(data.shape) == 2, ('the data should be a 2d matrix')
        self._train_gmm(data, score=score)
        self._create_gmm(data)

    def _train_gmm(self, data, n_K=40, score='BIC'):
        obs = np.random.permutation(data)
        n_samples = len(data)
        if n_samples < n_K:
            n_K = n_samples - 1
        if score not in ('BIC', 'AIC'):
            raise NotImplementedError
        if self.seed is None:
            self.seed = int(np.random.randint(0, 2 ** 31 - 1))
        K = list(range(1, n_K + 1))
        self.sweep = fit_gaussian_mixtures(obs, K, init=self.init, seed=self.seed, ctx=self.ctx)
        if score == 'BIC':
            self.model_scores = [g.train_bic(n_samples) for g in self.sweep]
        else:
            self.model_scores = [g.train_aic(n_samples) for g in self.sweep]
        min_idx = min(range(n_K), key=self.model_scores.__getitem__)
        self.numberOfGaussian = min_idx + 1

    def _create_gmm(self, data):
        self.gmm = fit_gaussian_mixtures(data, self.numberOfGaussian, init=self.init, seed=self.seed + 1, ctx=self.ctx)
        scores = self.gmm.train_score_
        self.averageScore = np.mean(scores)

    def convert_model_to_json(self):
        model_data = {'gmm_weights': self.gmm.weights_.tolist(),
                      'gmm_means': self.gmm.means_.tolist(),
                      'gmm_covars': self.gmm.covariances_.tolist()}
        return model_data

    def save_model(self, filename):
        with open(filename, "w") as f:
            json.dump(self.convert_model_to_json(), f)
