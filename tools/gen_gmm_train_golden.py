"""Writes tests/golden/gmm_train.npz: what the reference's GMMTrainer (construction/motion_primitive/gmm_trainer.py) does
on small latent sets -- its shuffle, every sklearn GaussianMixture fit of the AIC sweep and of the refit, and the KMeans
call inside each -- with, per fit, the reference's own sensitivity to the order of its sums.

    python tools/gen_gmm_train_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--out tests/golden/gmm_train.npz]

The reference's gmm_trainer module is imported unmodified; anim_utils.utilities.io_helper_functions is a stub and its prints
are discarded.  GMMTrainer().fit(X) runs under np.random.seed(seed) with the installed sklearn on one thread.  For every
GaussianMixture.fit the tool records the k-means++ picks (row indices into the fit's data: the centres are those rows;
sklearn picks them from X - X.mean(0)), the KMeans labels and n_iter_, the per-iteration lower bounds, n_iter_,
converged_, score(X) and aic(X); the weights and means of the refit and of K in {1, 2, 3, chosen, last} (every K when
d <= 6), their covariances and precision Cholesky factors too, except the last K's when d > 6 and all but K in {1, 2, 3}
when d > 12 (the others would not fit the file into 1 MB).

Spread: every fit is refitted by sklearn's EM from its recorded KMeans labels on 3 row permutations of its data (a
GaussianMixture whose _initialize_parameters takes the labels); per quantity the largest absolute difference from the
recorded fit is stored (spread_*).  A case is drawn again with the next seed when (a) in some KMeans call a member's two
smallest squared distances to the initial or to the final centres lie within 1e-9 relative, (b) some fit's |change of the
lower bound| lies within 1e-6 relative of tol, (c) a permuted refit's n_iter_ or converged_ differs, or (d) the best two
AICs of the sweep differ by less than 1000 x their spread.  At most a quarter of all draws may be redraws, or the tool
fails; each case records its redraw count.

Per case `c<i>_`: name, data, seed, redraws, perm (obs = data[perm]), chosen, average_score, and per fit (the sweep's K =
1 .. n_K, then the refit): fit_k, fit_refit, km_offsets/km_init_idx, km_labels (int8, one row per fit), km_n_iter, lb
(padded with NaN to max_iter), n_iter, converged, score, aic, spread_{weights,means,covariances,precisions,lb,score,aic};
param_fit (fit indices) with p_weights, p_means and cov_fit with p_covariances, p_precisions, concatenated over their
components.  Also
overflow_data (rows of magnitude 1e160), overflow_labels3 and overflow_sklearn_raises (K = 1 and K = 3 from those labels).
The archive is written with fixed timestamps, so running the tool again gives the identical file.
"""
import argparse
import contextlib
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from morphablegraphs_amd import synthetic  # noqa: E402
from morphablegraphs_amd.gaussian_mixture import sample_like_sklearn  # noqa: E402

MARGIN = 1e-9
MAX_ITER = 100
TOL = 1e-3
RECORD = {"fits": [], "km": []}


def load_reference(reference):
    for name in ("anim_utils", "anim_utils.utilities", "anim_utils.utilities.io_helper_functions"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["anim_utils.utilities.io_helper_functions"].write_to_json_file = lambda *args, **kwargs: None
    path = os.path.join(reference, "morphablegraphs", "construction", "motion_primitive", "gmm_trainer.py")
    spec = importlib.util.spec_from_file_location("gmm_trainer", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def instrument():
    from sklearn.cluster import KMeans, _kmeans
    from sklearn.mixture import GaussianMixture
    plusplus = _kmeans._kmeans_plusplus

    def _kmeans_plusplus(*args, **kwargs):
        centres, idx = plusplus(*args, **kwargs)
        RECORD["init_idx"] = np.asarray(idx).copy()
        return centres, idx
    _kmeans._kmeans_plusplus = _kmeans_plusplus
    km_fit = KMeans.fit

    def km_fit_and_record(self, X, y=None, sample_weight=None):
        out = km_fit(self, X, y, sample_weight)
        RECORD["km"].append({"init_idx": RECORD.pop("init_idx"), "labels": self.labels_.copy(), "n_iter": int(self.n_iter_),
                             "centres": self.cluster_centers_.copy()})
        return out
    KMeans.fit = km_fit_and_record
    gm_fit = RECORD["gm_fit"] = GaussianMixture.fit

    def gm_fit_and_record(self, X, y=None):
        X = np.asarray(X, dtype=np.float64)
        out = gm_fit(self, X, y)
        km = RECORD["km"].pop()
        RECORD["fits"].append({"X": X, "K": self.n_components, "km": km, "lb": np.array(self.lower_bounds_), "n_iter": int(self.n_iter_),
                               "converged": bool(self.converged_), "score": float(self.score(X)), "aic": float(self.aic(X)),
                               "weights": self.weights_.copy(), "means": self.means_.copy(), "covariances": self.covariances_.copy(),
                               "precisions": self.precisions_cholesky_.copy()})
        return out
    GaussianMixture.fit = gm_fit_and_record


def label_mixture(labels, K):
    from sklearn.mixture import GaussianMixture

    class LabelGaussianMixture(GaussianMixture):
        def _initialize_parameters(self, X, random_state):
            resp = np.zeros((len(X), self.n_components), dtype=X.dtype)
            resp[np.arange(len(X)), self._labels] = 1
            self._initialize(X, resp)
    gm = LabelGaussianMixture(n_components=K, covariance_type='full')
    gm._labels = np.asarray(labels)
    return gm


def _refit(X, labels, K):
    import warnings
    from sklearn.exceptions import ConvergenceWarning
    gm = label_mixture(labels, K)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        RECORD["gm_fit"](gm, X)     # not recorded
    return gm


def spreads(fit, rng):
    """Largest difference of each recorded quantity across 3 row permutations of the fit, and whether n_iter_/converged_
    held."""
    X, K, labels = fit["X"], fit["K"], fit["km"]["labels"]
    sp = dict.fromkeys(("weights", "means", "covariances", "precisions", "lb", "score", "aic"), 0.0)
    same = True
    for _ in range(3):
        p = rng.permutation(len(X))
        gm = _refit(X[p], labels[p], K)
        same &= gm.n_iter_ == fit["n_iter"] and bool(gm.converged_) == fit["converged"]
        q = {"weights": gm.weights_, "means": gm.means_, "covariances": gm.covariances_, "precisions": gm.precisions_cholesky_,
             "score": gm.score(X[p]), "aic": gm.aic(X[p])}
        for key, v in q.items():
            sp[key] = max(sp[key], float(np.max(np.abs(np.asarray(v) - fit[key]))))
        if len(gm.lower_bounds_) == len(fit["lb"]):
            sp["lb"] = max(sp["lb"], float(np.max(np.abs(np.array(gm.lower_bounds_) - fit["lb"]))))
    return sp, same


def _two_best_close(X, centres):
    d = ((X[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2)
    if d.shape[1] < 2:
        return False
    d.sort(axis=1)
    return bool(np.any(d[:, 1] - d[:, 0] <= MARGIN * np.maximum(d[:, 1], 1e-300)))


def _run(mod, data, seed):
    from threadpoolctl import threadpool_limits
    import warnings
    from sklearn.exceptions import ConvergenceWarning
    RECORD["fits"], RECORD["km"] = [], []
    np.random.seed(seed)
    with threadpool_limits(1), contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        trainer = mod.GMMTrainer()
        trainer.fit(data)
    return trainer, list(RECORD["fits"])


def _cases():
    rng = np.random.default_rng(4242)

    def blobs(n, d, centres, spread=3.0):
        c = rng.standard_normal((centres, d)) * spread
        return c[rng.integers(0, centres, n)] + rng.standard_normal((n, d))
    walk = synthetic.make_walk_primitive(seed=0)
    w, m, cv = (np.array(walk[k]) for k in ("gmm_weights", "gmm_means", "gmm_covars"))

    def walk_latents(n, s):
        X, _ = sample_like_sklearn(n, w, m, cv, random_state=np.random.RandomState(s))
        return X
    temporal = 0.1 * rng.standard_normal((500, 3))
    return [
        ("n200_d8", blobs(200, 8, 5)),
        ("n30_d4", blobs(30, 4, 3)),
        ("walk_n600_d40", walk_latents(600, 11)),
        ("offset_n400_d12", blobs(400, 12, 4) + 1e3),
        ("walk_time_n500_d43", np.hstack([walk_latents(500, 12), temporal])),
    ]


def _write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def _check_draw(fits, sp, same):
    """The redraw rules; returns the reason or None."""
    for f in fits:
        X, km = f["X"], f["km"]
        if f["K"] > 1 and (_two_best_close(X, X[km["init_idx"]]) or _two_best_close(X, km["centres"])):
            return "(a) KMeans near tie at K = %d" % f["K"]
        lb = np.concatenate([[-np.inf], f["lb"]])
        change = np.abs(np.diff(lb))[1:]
        if np.any(np.abs(change - TOL) <= 1e-6 * TOL):
            return "(b) lower-bound change near tol at K = %d" % f["K"]
    if not all(same):
        return "(c) n_iter differs across permutations"
    sweep = fits[:-1]
    aic = np.array([f["aic"] for f in sweep])
    if len(aic) > 1:
        order = np.argsort(aic, kind="stable")
        gap = aic[order[1]] - aic[order[0]]
        if gap < 1000 * max(sp[order[0]]["aic"], sp[order[1]]["aic"]):
            return "(d) AIC gap %.3g" % gap
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of dfki-asr/morphablegraphs")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gmm_train.npz"))
    args = ap.parse_args()
    mod = load_reference(args.reference)
    instrument()
    cases = _cases()
    out = {"names": np.array([c[0] for c in cases])}
    draws = redraws_total = 0
    for i, (name, data) in enumerate(cases):
        data = np.ascontiguousarray(data, dtype=np.float64)
        n, d = data.shape
        redraws = 0
        for seed in range(10 * i, 10 * i + 10):
            draws += 1
            trainer, fits = _run(mod, data, seed)
            rng = np.random.default_rng(1000 + seed)
            from threadpoolctl import threadpool_limits
            with threadpool_limits(1):
                res = [spreads(f, rng) for f in fits]
            why = _check_draw(fits, [r[0] for r in res], [r[1] for r in res])
            if why is None:
                break
            print("%s: seed %d: %s; next seed" % (name, seed, why))
            redraws += 1
            redraws_total += 1
        else:
            raise RuntimeError("%s: no seed passes the redraw rules" % name)
        obs = fits[0]["X"]
        row_of = {data[r].tobytes(): r for r in range(n)}
        perm = np.array([row_of[obs[r].tobytes()] for r in range(n)], dtype=np.int32)
        chosen = trainer.numberOfGaussian
        F = len(fits)
        p = "c%d_" % i
        sp = [r[0] for r in res]
        lb = np.full((F, MAX_ITER), np.nan)
        for j, f in enumerate(fits):
            lb[j, :len(f["lb"])] = f["lb"]
        Ks = [f["K"] for f in fits]
        n_sweep = F - 1
        keep = list(range(F)) if d <= 6 else sorted({0, 1, 2, chosen - 1, n_sweep - 1, F - 1})
        keep_cov = keep if d <= 6 else sorted({0, 1, 2, chosen - 1, F - 1}) if d <= 12 else [0, 1, 2]
        out.update({p + "name": np.array(name), p + "data": data, p + "seed": np.int64(seed), p + "redraws": np.int64(redraws),
                    p + "perm": perm, p + "chosen": np.int64(chosen), p + "average_score": np.float64(trainer.averageScore),
                    p + "fit_k": np.array(Ks, dtype=np.int32), p + "fit_refit": np.array([0] * n_sweep + [1], dtype=np.int8),
                    p + "km_offsets": np.concatenate([[0], np.cumsum(Ks)]).astype(np.int32),
                    p + "km_init_idx": np.concatenate([f["km"]["init_idx"] for f in fits]).astype(np.int32),
                    p + "km_labels": np.stack([f["km"]["labels"] for f in fits]).astype(np.int8),
                    p + "km_n_iter": np.array([f["km"]["n_iter"] for f in fits], dtype=np.int32),
                    p + "lb": lb, p + "n_iter": np.array([f["n_iter"] for f in fits], dtype=np.int32),
                    p + "converged": np.array([f["converged"] for f in fits]), p + "score": np.array([f["score"] for f in fits]),
                    p + "aic": np.array([f["aic"] for f in fits]), p + "param_fit": np.array(keep, dtype=np.int32),
                    p + "cov_fit": np.array(keep_cov, dtype=np.int32)})
        for key in ("weights", "means", "covariances", "precisions", "lb", "score", "aic"):
            out[p + "spread_" + key] = np.array([s[key] for s in sp])
        for key in ("weights", "means"):
            out[p + "p_" + key] = np.concatenate([fits[j][key] for j in keep])
        for key in ("covariances", "precisions"):
            out[p + "p_" + key] = np.concatenate([fits[j][key] for j in keep_cov])
        print("%-20s seed %3d  redraws %d  n %4d  d %2d  fits %2d  chosen K %2d  averageScore %.6f" % (name, seed, redraws, n, d, F,
                                                                                                      chosen, trainer.averageScore))
    if 4 * redraws_total > draws:
        raise RuntimeError("%d of %d draws redrawn: more than a quarter" % (redraws_total, draws))
    # rows of magnitude 1e160: the covariance overflows; sklearn raises for K = 1 and for K = 3 from given labels
    orng = np.random.default_rng(7)
    over = 1e160 * (1.0 + orng.random((24, 3)))
    lab3 = np.arange(24, dtype=np.int32) % 3
    raises = []
    for K, lab in ((1, np.zeros(24, dtype=np.int32)), (3, lab3)):
        try:
            _refit(over, lab, K)
            raises.append(False)
        except ValueError:
            raises.append(True)
    out.update({"overflow_data": over, "overflow_labels3": lab3, "overflow_sklearn_raises": np.array(raises),
                "draws": np.int64(draws), "redraws": np.int64(redraws_total)})
    _write_npz(args.out, out)
    print("draws %d, redraws %d" % (draws, redraws_total))
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
