"""What tests/test_reachability_scores_host.py and tests/test_gpu_reachability_scores.py share: the sklearn fixture
(tests/golden/reachability_scores.npz, tools/gen_reachability_golden.py), seeded mixtures, and the tolerances with where they come
from."""
import numpy as np

from conftest import load_golden

# log p of mg_gmm_log_prob(_host) against its NumPy statement / the recorded values: tests/test_gpu_parity.py
# (test_gmm_log_prob_golden and the float64 checks at its end) -- taken over, not chosen
LOGP_RTOL, LOGP_ATOL = 1e-9, 1e-7
# mixture_scores_host against sklearn's values: the largest |got - want| / max(1, |want|) over all fixture cases as
# tools/gen_reachability_golden.py measured it on the CPU (sklearn's BLAS sums in another order than the statement), and the 8x
# allowed on top of it for other BLAS builds' orders
MEASURED_DEVIATION = 6.51e-16
FIXTURE_MARGIN = 8.0


def fixture_cases():
    """[dict(weights, means, covars, X, threshold, logp, wlp)] of the sklearn fixture."""
    g = load_golden("reachability_scores")
    cases = []
    for c in range(int(g["n_cases"])):
        p = "c%d_" % c
        cases.append({key[len(p):]: g[key] for key in g.files if key.startswith(p)})
        cases[-1]["threshold"] = float(cases[-1]["threshold"])
    return cases, float(g["reachable_margin"])


def assert_within_fixture_tolerance(got, want, what=""):
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite), what
    assert np.array_equal(got[~finite], want[~finite]), what          # (-inf of a zero-weight component)
    dev = float((np.abs(got[finite] - want[finite]) / np.maximum(1.0, np.abs(want[finite]))).max()) if finite.any() else 0.0
    print("%s: deviation %.3g (allowed %.3g)" % (what, dev, FIXTURE_MARGIN * MEASURED_DEVIATION))
    assert dev <= FIXTURE_MARGIN * MEASURED_DEVIATION, (what, dev)


def seeded_mixture(K, dim, seed=0):
    """(weights (K,), means (K, dim), covars (K, dim, dim)) of a well-conditioned seeded mixture."""
    rng = np.random.default_rng([seed, K, dim])
    weights = rng.dirichlet(np.full(K, 2.0))
    means = rng.uniform(-3.0, 3.0, (K, dim))
    a = rng.standard_normal((K, dim, min(dim, 6))) * 0.4
    covars = a @ a.transpose(0, 2, 1) + (0.3 + 0.2 * rng.random((K, 1, 1))) * np.eye(dim)
    return weights, means, covars


def seeded_targets(means, n, seed=0):
    """n targets around the mixture's means (the first exactly at mean 0, when there is one)."""
    rng = np.random.default_rng([seed, n, means.shape[1], 7])
    X = means[rng.integers(0, len(means), n)] + rng.standard_normal((n, means.shape[1])) * 0.7
    if n:
        X[0] = means[0]
    return X


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
