"""Writes tests/golden/reachability_scores.npz: seeded full-covariance mixtures and targets with what sklearn's GaussianMixture --
the library the reference's reachability models are trained and scored with -- gives for them: score_samples (log p) and
_estimate_weighted_log_prob (the weighted log-probabilities of every component).  The tests read the file and never sklearn.

Cases (K, dim): (1, 3), (3, 4), (5, 6), (40, 3), (2, 17), (4, 96).  Every case's targets hold draws around the means, every mean
itself, and points so far out that every exp(wlp - max) but one underflows; case (3, 4) has a component of weight 0.  The
covariances are multiples of 2^-8 (and banded at dim 96), so that the compressed file stays at a few tens of KB.  A case's
threshold is the midpoint of the widest gap between two neighbouring scores of its near targets, so that no score lies within
REACHABLE_MARGIN of it: checked here, on the CPU.

    python tools/gen_reachability_golden.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "reachability_scores.npz")

CASES = ((1, 3), (3, 4), (5, 6), (40, 3), (2, 17), (4, 96))
ZERO_WEIGHT_CASE = 1
N_NEAR = 12
REACHABLE_MARGIN = 1e-3          # far above the 1e-7 + 1e-9 |log p| the device's log p is held to against the host's


def grid(a, bits=8):
    return np.round(np.asarray(a) * 2.0 ** bits) / 2.0 ** bits


def make_case(rng, K, dim, zero_weight):
    weights = rng.dirichlet(np.full(K, 2.0))
    if zero_weight:
        weights[1] = 0.0
        weights /= weights.sum()
    means = grid(rng.uniform(-4.0, 4.0, (K, dim)))
    covars = np.zeros((K, dim, dim))
    for k in range(K):
        if dim <= 32:
            a = rng.standard_normal((dim, dim)) * 0.4
            c = a @ a.T
        else:                                                   # banded: the factor's inverse is a full triangle all the same
            c = np.zeros((dim, dim))
            for off in (1, 2, 5):
                v = rng.uniform(-0.25, 0.25, dim - off)
                c += np.diag(v, off) + np.diag(v, -off)
        c = grid(c)
        c = np.tril(c) + np.tril(c, -1).T
        c[np.diag_indices(dim)] = grid(np.abs(c).sum(axis=1) - np.abs(np.diag(c)) + rng.uniform(0.25, 1.0, dim))   # strictly diagonally dominant: positive definite
        covars[k] = c
    near = means[rng.integers(0, K, N_NEAR)] + rng.standard_normal((N_NEAR, dim)) * 0.8
    base, sign, reach = means[rng.integers(0, K, 3)], rng.choice([-1.0, 1.0], (3, dim)), rng.uniform(40.0, 80.0, (3, 1))
    while True:                                                 # further out until one component alone is left of the sum
        X = np.concatenate((near, means, base + sign * reach))
        wlp = sklearn_values(weights, means, covars, X)[1][-3:]
        with np.errstate(under="ignore"):
            if K == 1 or ((np.exp(wlp - wlp.max(axis=1, keepdims=True)) > 0).sum(axis=1) == 1).all():
                return weights, means, covars, X
        reach = reach * 4.0


def sklearn_values(weights, means, covars, X):
    from sklearn.mixture import GaussianMixture
    from sklearn.mixture._gaussian_mixture import _compute_precision_cholesky
    gm = GaussianMixture(n_components=len(weights), covariance_type="full")
    gm.weights_, gm.means_, gm.covariances_ = weights, means, covars
    gm.precisions_cholesky_ = _compute_precision_cholesky(covars, "full")
    with warnings.catch_warnings(), np.errstate(divide="ignore"):
        warnings.simplefilter("ignore")                         # log(0) of the zero-weight component
        return gm.score_samples(X), gm._estimate_weighted_log_prob(X)


def deviation(got, want):
    """The largest |got - want| / max(1, |want|): relative for large values, absolute for small ones."""
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def main():
    rng = np.random.default_rng(20260)
    out = {"n_cases": np.int64(len(CASES)), "n_near": np.int64(N_NEAR), "reachable_margin": np.float64(REACHABLE_MARGIN)}
    for c, (K, dim) in enumerate(CASES):
        weights, means, covars, X = make_case(rng, K, dim, c == ZERO_WEIGHT_CASE)
        logp, wlp = sklearn_values(weights, means, covars, X)
        assert np.isfinite(logp).all()
        # the far targets: every term of the sum but the largest underflows
        with np.errstate(under="ignore"):
            terms = np.exp(wlp[-3:] - wlp[-3:].max(axis=1, keepdims=True))
        assert K == 1 or ((terms > 0).sum(axis=1) == 1).all(), (K, dim, (terms > 0).sum(axis=1))
        s = np.sort(logp[:N_NEAR])
        at = int(np.argmax(np.diff(s)))
        threshold = 0.5 * (s[at] + s[at + 1])
        assert np.abs(logp - threshold).min() > REACHABLE_MARGIN
        assert (logp < threshold).any() and not (logp < threshold).all()
        p = "c%d_" % c
        out.update({p + "weights": weights, p + "means": means, p + "covars": covars, p + "X": X, p + "threshold": np.float64(threshold),
                    p + "logp": logp, p + "wlp": wlp})
        print("case %d: K %d dim %d, %d targets, log p %.4g .. %.4g, threshold %.6g" % (c, K, dim, len(X), logp.min(), logp.max(), threshold))
    np.savez_compressed(OUT, **out)
    print("%s: %d bytes" % (OUT, os.path.getsize(OUT)))
    # what the tests hold mixture_scores_host to: its largest deviation from these values, measured here
    from morphablegraphs_amd import feature_point_model as fpm
    worst = 0.0
    for c in range(len(CASES)):
        p = "c%d_" % c
        logp, wlp = fpm.mixture_scores_host(out[p + "weights"], out[p + "means"], out[p + "covars"], out[p + "X"])
        finite = np.isfinite(out[p + "wlp"])
        assert np.array_equal(finite, np.isfinite(wlp))
        dev = max(deviation(logp, out[p + "logp"]), deviation(wlp[finite], out[p + "wlp"][finite]))
        print("case %d: mixture_scores_host deviates by %.3g" % (c, dev))
        worst = max(worst, dev)
    print("largest deviation %.3g (tests/test_reachability_scores_host.py: MEASURED_DEVIATION)" % worst)


if __name__ == "__main__":
    main()
