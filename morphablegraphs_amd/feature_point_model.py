"""Feature-point (reachability) models of motion primitives (reference construction/feature_point_model.py and
feature_point_model_builder.py).

FeaturePointModel draws n latents, back-projects each to a whole motion and keeps the root's ground position and heading at the
last frame (create_root_pos_ori), or the position of a few joints at one frame relative to the first root position
(create_feature_points); it fits a Gaussian mixture to those 3, 4 or 3 J numbers and stores it with a log-likelihood threshold,
so that check_reachability / score_trajectory_target can say whether the primitive gets to a target at all.  Here the features
of every candidate -- of every node, for the builder -- come from ONE mg_feature_points call (csrc/mg_feature_points.hip), which
evaluates the three frames that are asked for and writes no frame to memory; the mixture is trained by HipGMMTrainer.

The reference's own default is the time-warped motion (back_project(s, use_time_parameters=True)): with time_warped=True the
features of a primitive with a time model come from ONE mg_feature_points_warped call, which takes from every candidate's time
function the one sample it needs.  Without the keyword that combination raises NotImplementedError, as before.

feature_points_host and feature_points_warped_host are the NumPy statements of the kernels' arithmetic; they need no library.

Scoring targets: score_targets, score_trajectory_targets and check_reachability_batch take device=True, which scores the rows by
mg_mixture_scores (csrc/mg_mixture_scores.hip) against the model's mixture, uploaded once; HipReachabilityIndex scores a set of
targets against the mixtures of ALL nodes of a graph in ONE launch.  mixture_scores_host is the NumPy statement of that kernel.

Not restated: plot_orientation; smoothed time functions without the primitive's opt-in smooth_on_device (with it: one
mg_feature_points_warped_smoothed call) and speeds other than 1 in the time-warped features; the reference's mixture.GMM class (loading gives FeatureMixture, the
same JSON).
"""
import json
import os

import numpy as np

from . import _capi
from . import graph_walk as gw
from .gaussian_mixture import sample_like_sklearn
from .time_smoothing import require_smoothing_window
from .gmm_trainer import ILL_DEFINED_MESSAGE, HipGMMTrainer, _compute_precision_cholesky, _estimate_weighted_log_prob

REF_DIR = (0.0, 0.0, 1.0)          # pose_orientation_quat turns this axis


# ---- the arithmetic on the host ------------------------------------------------------------------------------------
def _rotate(q, v):
    """v turned by the unit quaternion q = (w, u): v + 2 (w u x v + u x (u x v))."""
    u = q[1:]
    return v + 2.0 * (q[0] * np.cross(u, v) + np.cross(u, np.cross(u, v)))


def joint_position_host(skeleton, frame, joint):
    """Global position of `joint` in one pose vector: mg_joint_positions' loop (every chain quaternion made unit and multiplied
    into the accumulated orientation, the child's offset turned by it and added)."""
    chain = skeleton.chain(joint)
    p = np.array(frame[:3], dtype=np.float64)
    q = np.array([1.0, 0.0, 0.0, 0.0])
    for parent, child in zip(chain[:-1], chain[1:]):
        ch = int(skeleton.quat_channel[parent])
        if ch >= 0:
            qj = np.asarray(frame[ch:ch + 4], dtype=np.float64)
            q = _capi._quat_mul(q, qj / np.linalg.norm(qj))
        p = p + _rotate(q, np.asarray(skeleton.offsets[child], dtype=np.float64))
    return p


def heading_host(frame):
    """(unit (x, z), length before the division) of the root quaternion of `frame`, made unit, applied to (0, 0, 1)."""
    q = np.asarray(frame[3:7], dtype=np.float64)
    v = _rotate(q / np.linalg.norm(q), np.array(REF_DIR))
    d = np.array([v[0], v[2]])
    length = np.linalg.norm(d)
    return d / length, length


def _nan_outputs(n, J, **more):
    """The outputs of n candidates with J joints, NaN until a row is stated; more: an entry point's own arrays."""
    out = {"start_root": np.full((n, 3), np.nan), "root_end": np.full((n, 2), np.nan), "heading_end": np.full((n, 2), np.nan),
           "heading_len": np.full(n, np.nan)}
    out.update(more)
    if J:
        out["points"] = np.full((n, 3 * J), np.nan)
    return out


def _state_row(out, b, fr, skeleton, joints):
    """Row b of the outputs from its frames fr: the first, the one of `joints` (none: points stays NaN), the last."""
    out["start_root"][b] = fr[0, :3]
    for j, joint in enumerate(joints):
        out["points"][b, 3 * j:3 * j + 3] = joint_position_host(skeleton, fr[1], joint) - fr[0, :3]
    out["root_end"][b] = fr[2, 0], fr[2, 2]
    out["heading_end"][b], out["heading_len"][b] = heading_host(fr[2])


def feature_points_host(model, S, skeleton=None, joints=(), frame_idx=0):
    """The NumPy statement of mg_feature_points for one item.  model: the reference's JSON dict or a primitive; S (n, >= L): a
    candidate reads its first L columns; skeleton: a _capi.Skeleton (needed with joints); joints: names or indices.  Returns the
    dict of float64 arrays _capi.feature_points returns: start_root (n, 3), points (n, 3 J; with joints), root_end (n, 2),
    heading_end (n, 2), heading_len (n,).  A row with a latent that is not finite is NaN throughout."""
    hm = model if isinstance(model, gw._HostModel) else gw._HostModel(model)
    S = np.atleast_2d(np.asarray(S, dtype=np.float64))
    F, L = hm.n_canonical_frames, hm.n_components
    if not 0 <= int(frame_idx) < F:
        raise ValueError("frame_idx %d outside 0 .. %d" % (frame_idx, F - 1))
    joints = [skeleton.index(j) for j in joints]
    times = np.linspace(0, F, F)[[0, int(frame_idx), F - 1]]
    out = _nan_outputs(len(S), len(joints))
    for b in range(len(S)):
        if np.isfinite(S[b, :L]).all():
            _state_row(out, b, hm.frames(S[b, :L], times)[1], skeleton, joints)
    return out


def _time_model_host(model):
    """(knots, mean vector, eigen vectors (n_basis_time, Lt)) of the time model of the reference's JSON dict or a primitive."""
    if isinstance(model, dict):
        return (np.asarray(model["b_spline_knots_time"], dtype=np.float64), np.asarray(model["mean_time_vector"], dtype=np.float64),
                np.asarray(model["eigen_vectors_time"], dtype=np.float64))
    t_pca = getattr(model, "motion_primitive", model).t_pca
    return (np.asarray(t_pca["knots"], dtype=np.float64), np.asarray(t_pca["mean_vector"], dtype=np.float64),
            np.asarray(t_pca["eigen_vectors"], dtype=np.float64))


def canonical_time_function_host(time_model, F, gamma):
    """t(t') at the canonical frames (motion_primitive.py:289-302): the running sum of exp(mean spline + harmonics . gamma) in
    canonical-frame order, minus 1."""
    from scipy.interpolate import splev
    knots, mean, eig = time_model
    frames = np.arange(F)
    mean_t = splev(frames, (knots, mean, 3))
    phi = np.array([splev(frames, (knots, eig[:, l].copy(), 3)) for l in range(eig.shape[1])]).T
    out = [0]
    for i in range(F):
        out.append(out[-1] + np.exp(mean_t[i] + np.dot(phi[i], gamma)))
    return np.array(out[1:]) - 1.0


def sample_time_function_host(canonical, speed=1.0):
    """The spline's time function (motion_primitive.py:304-319) as HipMotionPrimitive._invert_canonical_to_sample_
    time_function states it: 0, scipy's interpolating cubic through (t(t'), t') at linspace(1, t(F - 2), int(round(t(F - 2)) *
    (1 / speed))), F - 1.  None for a time function that is not finite or asks for more than 2^24 samples (the kernels' test)."""
    from scipy.interpolate import splev, splrep
    canonical = np.asarray(canonical, dtype=np.float64)
    F, last = len(canonical), canonical[-2]
    if not np.isfinite(last) or not abs(last) <= 1.0e300 or np.round(last) * (1.0 / float(speed)) > 16777216.0:
        return None
    n_inner = int(np.round(last) * (1.0 / float(speed)))
    if n_inner <= 0:
        return np.array([0.0, F - 1.0])
    if not np.isfinite(canonical).all():
        return np.concatenate(([0.0], np.full(n_inner, np.nan), [F - 1.0]))
    inner = splev(np.linspace(1.0, last, n_inner), splrep(canonical, np.arange(F), k=3))
    return np.concatenate(([0.0], inner, [F - 1.0]))


def feature_points_warped_host(model, S, skeleton=None, joints=(), frame_idx=0, time_mid=None, smooth=False):
    """The NumPy statement of mg_feature_points_warped for one item.  model: the reference's JSON dict or a primitive, with a
    time model; S (n, >= L + Lt): a candidate reads L spatial latents and, right behind them, Lt time latents; frame_idx counts
    the frames of the WARPED motion.  The frames are those of the times 0, time_mid and F - 1; with time_mid (n,) given, the mid
    frame is evaluated at those times instead of the statement's own (a NaN there: the candidate's motion is shorter).  Returns
    what feature_points_host returns and time_mid (n,), n_frames (n,) int32.  n_frames = 0 (no time function): NaN in every
    output of the row; a spatial latent that is not finite: NaN in the feature outputs; frame_idx >= n_frames: NaN in points
    and time_mid only.  smooth: the time function passes through time_smoothing.smooth_time_row_host first, which moves all three
    times -- the first one becomes row 0 of the hat matrix on the first 15 samples (it can be negative), the last one row 14 on the
    last 15 and is no longer F - 1; a candidate of fewer than 15 frames is NaN in every output but n_frames."""
    from .time_smoothing import WINDOW, smooth_time_row_host
    hm = model if isinstance(model, gw._HostModel) else gw._HostModel(model)
    tm = _time_model_host(model)
    S = np.atleast_2d(np.asarray(S, dtype=np.float64))
    F, L, Lt = hm.n_canonical_frames, hm.n_components, tm[2].shape[1]
    frame_idx = int(frame_idx)
    if frame_idx < 0:
        raise ValueError("frame_idx %d below 0" % frame_idx)
    joints = [skeleton.index(j) for j in joints]
    n = len(S)
    out = _nan_outputs(n, len(joints), time_mid=np.full(n, np.nan), n_frames=np.zeros(n, dtype=np.int32))
    for b in range(n):
        with np.errstate(over="ignore", invalid="ignore"):
            times = sample_time_function_host(canonical_time_function_host(tm, F, S[b, L:L + Lt]))
        if times is None:
            continue
        out["n_frames"][b] = len(times)
        if smooth:
            if len(times) < WINDOW:
                continue
            times = smooth_time_row_host(times)
        short = frame_idx >= len(times)
        if not short:
            out["time_mid"][b] = times[frame_idx]
        mid = out["time_mid"][b] if time_mid is None else float(np.asarray(time_mid)[b])
        short = short or (time_mid is not None and np.isnan(mid))
        if not np.isfinite(S[b, :L]).all():
            continue
        first, last = (times[0], times[-1]) if smooth else (0.0, F - 1.0)
        _, fr = hm.frames(S[b, :L], np.array([first, first if short else mid, last]))
        _state_row(out, b, fr, skeleton, () if short else joints)
    return out


def _two_sum(a, b):
    """(s, e) with s = fl(a + b) and a + b = s + e exactly (Knuth)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _fma(a, b, c):
    """fl(a b + c) with ONE rounding, on float64 arrays, as the C fma gives it: the product exactly as two doubles (Veltkamp's
    split, Dekker's product), then Boldo and Melquiond's three-term sum -- the small terms added with rounding to odd, so that
    the last addition rounds the exact value.  Holds while no intermediate overflows and the product's low half is a normal
    number (|a b| between about 1e-290 and 1e290): the ranges of a mixture's statements, not of every double.  A NaN or an
    infinity among the operands gives a + b * c, which has their special value."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        ph = a * b
        ta, tb = 134217729.0 * a, 134217729.0 * b                    # 2^27 + 1
        ah, bh = ta - (ta - a), tb - (tb - b)
        al, bl = a - ah, b - bh
        pl = al * bl - (((ph - ah * bh) - al * bh) - ah * bl)
        th, tl = _two_sum(c, ph)
        v, e = _two_sum(tl, pl)
        # rounding to odd: where the sum was inexact and its last bit is even, one step towards the error
        even = (v.view(np.int64) & 1) == 0
        v = np.where((e != 0.0) & even, np.nextafter(v, np.where(e > 0.0, np.inf, -np.inf)), v)
        z = th + v
        return np.where(np.isfinite(ph) & np.isfinite(c), z, ph + c)


LOG_2PI = 1.8378770664093453          # log(2 pi) to the nearest double, as csrc/mg_mixture_image.h writes it


def mixture_image_host(weights, means, covars):
    """The image mg_feature_mixture_create forms, statement for statement (csrc/mg_mixture_image.h): (P (K, dim, dim) upper
    triangular, m (K, dim), c (K,)).  The Cholesky factor row by row and its inverse by forward substitution, every product and
    difference rounded on its own, the sums in ascending index order; m_j = mu_0 P[0][j], then fma(mu_i, P[i][j], .); c = (-0.5
    dim log(2 pi) + (log P[0][0] + log P[1][1] + ..)) + log w, the logarithms by the C library's log (math.log), -inf for a weight
    of 0.  ValueError with sklearn's text for a covariance that is not positive definite."""
    import math
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    mu = np.atleast_2d(np.asarray(means, dtype=np.float64))
    K, d = mu.shape
    C = np.asarray(covars, dtype=np.float64).reshape(K, d, d)
    Lo = np.zeros((K, d, d))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(d):
            s = C[:, i, :i + 1].copy()                       # s[j], j = 0 .. i; the subtractions reach every s[j] in ascending p
            for p in range(i):
                Lo[:, i, p] = s[:, p] / Lo[:, p, p]
                s[:, p + 1:] = s[:, p + 1:] - Lo[:, i, p, None] * Lo[:, p + 1:i + 1, p]
            if not (np.isfinite(s[:, i]) & (s[:, i] > 0.0)).all():
                raise ValueError(ILL_DEFINED_MESSAGE)
            Lo[:, i, i] = np.sqrt(s[:, i])
        X = np.zeros((K, d, d))                                  # inv(chol): X[r][c] = ((r == c) - sum_{p = c}^{r - 1} chol[r][p] X[p][c]) / chol[r][r]
        S = np.broadcast_to(np.eye(d), (K, d, d)).copy()
        for p in range(d):
            X[:, p, :p + 1] = S[:, p, :p + 1] / Lo[:, p, p, None]
            S[:, p + 1:, :p + 1] = S[:, p + 1:, :p + 1] - Lo[:, p + 1:, p, None] * X[:, p, None, :p + 1]
    P = np.transpose(X, (0, 2, 1)).copy()
    m = np.empty((K, d))
    for j in range(d):
        acc = mu[:, 0] * P[:, 0, j]
        for i in range(1, j + 1):
            acc = _fma(mu[:, i], P[:, i, j], acc)
        m[:, j] = acc
    c = np.empty(K)
    for k in range(K):
        if not all(np.isfinite(P[k, j, j]) and P[k, j, j] > 0.0 for j in range(d)):
            raise ValueError(ILL_DEFINED_MESSAGE)
        logdet = math.log(P[k, 0, 0])
        for j in range(1, d):
            logdet = logdet + math.log(P[k, j, j])
        c[k] = (-0.5 * d * LOG_2PI + logdet) + (math.log(w[k]) if w[k] > 0.0 else -np.inf)
    return P, m, c


def mixture_scores_host(weights, means, covars, X, image=None):
    """The NumPy statement of mg_mixture_scores for one item: (logp (n,), wlp (n, K)) of the targets X (n, dim) under the
    full-covariance mixture, float64, every operation rounded on its own, in the kernel's order (no BLAS dot, whose summation
    order is the library's own):
        y_j   = (x_0 P[0][j], then fma(x_i, P[i][j], .) for i = 1 .. j) - m_j
        q     = y_0 y_0, then fma(y_j, y_j, .)
        wlp_k = fma(-0.5, q, c_k)
        logp  = max + log(exp(wlp_0 - max) + exp(wlp_1 - max) + ..); -inf where every wlp_k is -inf.
    A target with a coordinate that is not finite is NaN in both.  image: (P, m, c) in place of mixture_image_host's."""
    P, m, c = image if image is not None else mixture_image_host(weights, means, covars)
    K, d = m.shape
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    if X.shape[1] != d:
        raise ValueError("X has %d features, but the mixture expects %d" % (X.shape[1], d))
    bad = ~np.isfinite(X).all(axis=1)
    Xs = np.where(bad[:, None], 0.0, X)
    n = len(X)
    q = np.zeros((n, K))
    for j in range(d):
        acc = Xs[:, 0, None] * P[None, :, 0, j]
        for i in range(1, j + 1):
            acc = _fma(Xs[:, i, None], P[None, :, i, j], acc)
        y = acc - m[None, :, j]
        q = y * y if j == 0 else _fma(y, y, q)
    wlp = _fma(-0.5, q, c[None, :])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mx = wlp.max(axis=1) if n else np.zeros(0)
        safe = np.where(np.isfinite(mx), mx, 0.0)
        s = np.exp(wlp[:, 0] - safe)
        for k in range(1, K):
            s = s + np.exp(wlp[:, k] - safe)
        logp = np.where(mx == -np.inf, -np.inf, mx + np.log(s))
    wlp[bad] = np.nan
    logp[bad] = np.nan
    return logp, wlp


def rotation_angle(point1, point2):
    """anim_utils' get_rotation_angle: the angle from point1 to point2 in degrees, brought into [-180, 180] (restated, unpinned)."""
    theta1 = np.rad2deg(np.arctan2(point1[1], point1[0]))
    theta2 = np.rad2deg(np.arctan2(point2[1], point2[0]))
    delta = theta2 - theta1
    if delta < -180.0:
        delta += 360.0
    elif delta > 180.0:
        delta -= 360.0
    return delta


def orientations_to_angles(orientations, ref_ori=(0, -1)):
    """convert_ori_to_angle_deg's loop (feature_point_model.py:97-103), deg2rad(-get_rotation_angle(ori, ref_ori)) per row, for
    all rows at once: rotation_angle's statements on arrays."""
    ori = np.asarray(orientations, dtype=np.float64).reshape(-1, 2)
    theta1 = np.rad2deg(np.arctan2(ori[:, 1], ori[:, 0]))
    theta2 = np.rad2deg(np.arctan2(ref_ori[1], ref_ori[0]))
    delta = theta2 - theta1
    delta = np.where(delta < -180.0, delta + 360.0, np.where(delta > 180.0, delta - 360.0, delta))
    return list(np.deg2rad(-delta))


# ---- the stored mixture --------------------------------------------------------------------------------------------
class FeatureMixture(object):
    """A full-covariance mixture over 3, 4 or 3 J features with the attribute names the reference's JSON writer reads
    (weights_, means_, covars_) and the old sklearn GMM's calling shapes the reference relies on: score(X) is the per-row
    log p, sample(n) the rows alone.  The log-density is gmm_trainer's host restatement of sklearn's."""

    def __init__(self, weights, means, covars):
        self.weights_ = np.asarray(weights, dtype=np.float64)
        self.means_ = np.atleast_2d(np.asarray(means, dtype=np.float64))
        self.covars_ = np.asarray(covars, dtype=np.float64).reshape(len(self.weights_), self.means_.shape[1], self.means_.shape[1])
        self.covariances_ = self.covars_
        self.precisions_cholesky_ = _compute_precision_cholesky(self.covars_)
        self.n_components = len(self.weights_)
        self.converged_ = True

    def score_samples(self, X):
        from scipy.special import logsumexp
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        if X.shape[1] != self.means_.shape[1]:
            raise ValueError("X has %d features, but the mixture expects %d" % (X.shape[1], self.means_.shape[1]))
        return logsumexp(_estimate_weighted_log_prob(X, self.weights_, self.means_, self.precisions_cholesky_), axis=1)

    score = score_samples

    def sample(self, n_samples=1):
        return sample_like_sklearn(n_samples, self.weights_, self.means_, self.covars_)[0]


def _mixture_json(dist):
    return {"gmm_weights": dist.weights_.tolist(), "gmm_means": dist.means_.tolist(), "gmm_covars": dist.covars_.tolist()}


# ---- the model -----------------------------------------------------------------------------------------------------
class HipFeaturePointModel(object):
    """FeaturePointModel's method table over a HipMotionPrimitive (or a node that carries one as .motion_primitive) and a
    _capi.Skeleton (None is enough for the root features).

    latents: None draws them like the reference, one GaussianMixture.sample per candidate from NumPy's global stream (a seeded
    stream gives the reference's latents); device=True draws the whole batch with the device sampler (same distribution, another
    stream); latents= passes them in.  The features come from one mg_feature_points call.

    time_warped=True: on a primitive with a time model and use_time_parameters=True the features are those of the time-warped
    motion -- the reference's default -- from one mg_feature_points_warped call on full latent rows (spatial + time); a candidate
    whose warped motion has no frame frame_idx raises IndexError, as the reference's indexing does; so does a candidate without a
    time function (n_frames 0: exp overflowed, or a time latent is not finite) in the root features and in the builder, which name
    it instead of training on NaN rows.  smooth_time_parameters=True
    on the primitive raises NotImplementedError unless the primitive also sets smooth_on_device: then one
    mg_feature_points_warped_smoothed call takes all three of a candidate's times from the smoothed time function (the
    Savitzky-Golay pass inside the kernel), and a candidate of fewer than 15 frames raises ValueError, as scipy would.
    Without a time model, or with use_time_parameters=False, the keyword changes nothing.

    Training: the reference writes GMMTrainer(training_samples) and reads .gmm and .averageScore, which does not match
    GMMTrainer's constructor (it takes no data; fit(data, score='AIC') trains).  What is built is what it means:
    HipGMMTrainer().fit(samples) with the AIC default; max_components bounds the sweep (GMMTrainer's n_K, 40).  The thresholds
    are averageScore (root features) and averageScore - 5 (feature points), as written."""

    def __init__(self, primitive, skeleton=None, use_time_parameters=True, device=False, latents=None, max_components=40, seed=None, ctx=None,
                 time_warped=False):
        self.motion_primitive_model = gw._primitive_of(primitive)
        self.skeleton = skeleton
        self.time_warped = bool(time_warped)
        self.use_time_parameters, self.device, self.latents = use_time_parameters, bool(device), latents
        self.max_components, self.seed, self.ctx = int(max_components), seed, ctx
        self.low_dimension_vectors = []
        self.feature_points = []
        self.orientations = []
        self.feature_point = None
        self.feature_point_list = []
        self.threshold = None
        self.root_pos = []
        self.root_low_dimension_vectors = []
        self.root_orientation = []
        self.root_rot_angles = []
        self.heading_lengths = []          # the headings' lengths before the division (a degenerate heading shows here)
        self.feature_point_dist = None
        self.root_feature_dist = None
        self.root_feature_dist_type = None
        self.root_threshold = None

    # ---- latents and the one call ------------------------------------------------------------------
    def _warps(self):
        """Whether the features are those of the time-warped motion: use_time_parameters on a primitive with a time model."""
        mp = self.motion_primitive_model
        return bool(self.use_time_parameters and mp.has_time_parameters and mp.t_pca.get("n_components", 0) > 0)

    def _draw(self, n):
        mp = self.motion_primitive_model
        if self._warps():
            if not self.time_warped:
                raise NotImplementedError("time-warped feature points: pass time_warped=True, or use_time_parameters=False, for a primitive with a time model")
            if getattr(mp, "smooth_time_parameters", False) and not getattr(mp, "smooth_on_device", False):
                raise NotImplementedError("time-warped feature points of a smoothed time function: set smooth_on_device on the primitive for the "
                                          "Savitzky-Golay pass inside the kernel")
        if self.latents is not None:
            S = _capi._latents(self.latents)
            if len(S) != n:
                raise ValueError("%d latents passed, %d asked for" % (len(S), n))
            return S
        gmm = mp.gaussian_mixture_model
        if self.device:
            return np.ascontiguousarray(gmm.sample(n, device=True)[0])
        if n == 0:
            return np.zeros((0, gmm.means_.shape[1]))
        return np.vstack([mp.sample_low_dimensional_vector() for _ in range(n)])

    def _item(self, S, joints=(), frame_idx=0):
        return {"prim": self.motion_primitive_model._prim, "S": S, "skeleton": self.skeleton, "joints": list(joints), "frame_idx": frame_idx}

    def _features(self, items, wanted, smooth=None):
        """One call for `items` (all of this model's kind): mg_feature_points_warped where the motion is time-warped,
        mg_feature_points_warped_smoothed where a time function is smoothed (smooth_on_device).  smooth: one flag per item (None:
        this model's for all of them)."""
        if not self._warps():
            return _capi.feature_points(items, wanted)
        smooth = [self._smooths()] * len(items) if smooth is None else list(smooth)
        if any(smooth):
            return _capi.feature_points_warped(items, wanted, smooth=smooth)
        return _capi.feature_points_warped(items, wanted)

    def _smooths(self):
        mp = self.motion_primitive_model
        return bool(getattr(mp, "smooth_time_parameters", False) and getattr(mp, "smooth_on_device", False))

    def _require_window(self, out, name=""):
        """ValueError, as scipy's, for the first candidate whose time function is too short to smooth (out: with "n_frames")."""
        if self._warps() and self._smooths() and "n_frames" in out:
            require_smoothing_window(out["n_frames"], (name and name + ": ") + "candidate %d")

    @staticmethod
    def _require_frame(out, frame_idx, name=""):
        """IndexError for the first candidate whose warped motion has no frame frame_idx (out: with "n_frames")."""
        short = np.flatnonzero(out["n_frames"] <= frame_idx) if "n_frames" in out else ()
        if len(short):
            raise IndexError("%scandidate %d: index %d is out of bounds for a warped motion of %d frames" % (name and name + ": ", short[0], frame_idx,
                                                                                                             out["n_frames"][short[0]]))

    def _root_outputs(self):
        """What the root features ask of the call; with the warp also n_frames, so that a candidate without a time function (0 frames:
        exp overflowed, or time latents that are not finite) raises through _require_frame(out, 0) instead of training on NaN."""
        return ("root_end", "heading_end", "heading_len") + (("n_frames",) if self._warps() else ())

    def _take_root(self, out, S):
        self.root_low_dimension_vectors += np.asarray(S, dtype=np.float64).tolist()      # (the reference does not keep these)
        self.root_pos += list(out["root_end"])
        self.root_orientation += list(out["heading_end"])
        self.heading_lengths += list(out["heading_len"])
        self.root_feature_dist_type = 'vector'

    # ---- feature_point_model.py:58-103 -------------------------------------------------------------
    def create_feature_points(self, joint_name_list, n, frame_idx):
        assert type(joint_name_list) == list, 'joint names should be a list'
        if self.skeleton is None:
            raise ValueError("feature points of joints need a skeleton")
        self.feature_point_list = joint_name_list
        S = self._draw(n)
        warps = self._warps()
        out = self._features([self._item(S, joint_name_list, frame_idx)], ("points", "heading_end", "heading_len") + (("n_frames",) if warps else ()))[0]
        self._require_window(out)
        self._require_frame(out, int(frame_idx))
        self.low_dimension_vectors += np.asarray(S, dtype=np.float64).tolist()
        self.feature_points += list(out["points"])
        self.orientations += out["heading_end"].tolist()
        self.heading_lengths += list(out["heading_len"])

    def create_root_pos_ori(self, n):
        S = self._draw(n)
        out = self._features([self._item(S)], self._root_outputs())[0]
        self._require_window(out)
        self._require_frame(out, 0)
        self._take_root(out, S)

    def convert_ori_to_angle_deg(self, ref_ori=[0, -1]):
        assert len(self.root_orientation) > 0, ("please create root orientation list first!")
        self.root_rot_angles += orientations_to_angles(self.root_orientation, ref_ori)
        self.root_feature_dist_type = 'angle'

    # ---- training ----------------------------------------------------------------------------------
    def _train(self, samples):
        trainer = HipGMMTrainer(seed=self.seed, ctx=self.ctx)
        assert len(samples.shape) == 2, ('the data should be a 2d matrix')      # GMMTrainer.fit with score='AIC'
        trainer._train_gmm(samples, n_K=self.max_components, score='AIC')
        trainer._create_gmm(samples)
        return FeatureMixture(trainer.gmm.weights_, trainer.gmm.means_, trainer.gmm.covariances_), float(trainer.averageScore)

    def model_root_dist(self):
        if self.root_feature_dist_type == 'vector':
            training_samples = np.concatenate((np.asarray(self.root_pos), np.asarray(self.root_orientation)), axis=1)
        elif self.root_feature_dist_type == 'angle':
            training_samples = np.concatenate((np.asarray(self.root_pos), np.reshape(self.root_rot_angles, (len(self.root_rot_angles), 1))), axis=1)
        else:
            raise ValueError('The type of root feature points is not specified!')
        self.root_feature_dist, self.root_threshold = self._train(training_samples)

    def model_feature_points(self):
        self.feature_point_dist, score = self._train(np.asarray(self.feature_points))
        self.threshold = score - 5

    # ---- sampling and scoring ----------------------------------------------------------------------
    def sample_new_root_feature(self):
        new_sample = np.ravel(self.root_feature_dist.sample())
        if self.root_feature_dist_type == 'vector':
            new_sample[2:] = new_sample[2:] / np.linalg.norm(new_sample[2:])
        return new_sample

    def sample_new_feature(self):
        return np.ravel(self.feature_point_dist.sample())

    def device_mixture(self, which="points", host=False):
        """The model's mixture ("points": feature_point_dist and threshold; "root": root_feature_dist and root_threshold) as a
        _capi.FeatureMixture, made on first use and kept until the model's mixture or threshold is another object or value
        (retrained, reloaded); host=True: without a device copy, for _capi.mixture_scores_host."""
        dist, threshold = (self.feature_point_dist, self.threshold) if which == "points" else (self.root_feature_dist, self.root_threshold)
        assert dist is not None, 'Please model or load the %s distribution.' % ("feature point" if which == "points" else "root feature")
        cache = self.__dict__.setdefault("_device_mixtures", {})
        kept = cache.get((which, host))
        if kept is None or kept[0] is not dist or kept[1] != threshold:
            if kept is not None:
                kept[2].close()
            mix = _capi.FeatureMixture(self.ctx, dist.weights_, dist.means_, dist.covars_, -np.inf if threshold is None else threshold, host=host)
            kept = cache[(which, host)] = (dist, threshold, mix)
        return kept[2]

    def _device_scores(self, which, targets, output="logp"):
        mix = self.device_mixture(which)
        targets = np.atleast_2d(np.asarray(targets, dtype=np.float64))
        if targets.shape[1] != mix.dim:
            raise ValueError("X has %d features, but the mixture expects %d" % (targets.shape[1], mix.dim))
        return _capi.mixture_scores([(mix, targets)], (output,))[0][output]

    def score_trajectory_targets(self, targets, device=False):
        """Per-row log p of root targets under the root mixture: (n, 4) for 'vector', (n, 3) for 'angle'.  device=True: by
        mg_mixture_scores."""
        assert self.root_feature_dist is not None, 'Please model or load root feature distribution.'
        targets = np.atleast_2d(np.asarray(targets, dtype=np.float64))
        width = 4 if self.root_feature_dist_type == 'vector' else 3
        assert targets.shape[1] == width, 'The trajectory target should be a vector of length %d.' % width
        if device:
            return self._device_scores("root", targets)
        return self.root_feature_dist.score_samples(targets)

    def score_trajectory_target(self, target):
        return self.score_trajectory_targets([target, ])[0]

    def score_targets(self, targets, device=False):
        """Per-row log p of feature-point targets (n, 3 J) under the stored mixture.  device=True: by mg_mixture_scores."""
        assert self.feature_point_dist is not None, 'Please model or load the feature point distribution.'
        if device:
            return self._device_scores("points", targets)
        return self.feature_point_dist.score_samples(targets)

    def check_reachability_batch(self, targets, device=False):
        if device:
            return self._device_scores("points", targets, "reachable")
        return ~(self.score_targets(targets) < self.threshold)

    def evaluate_target_point(self, target_point):
        if len(self.feature_points) > 0:
            assert len(target_point) == len(self.feature_points[0]), 'the length of feature is not correct'
        return self.score_targets([target_point, ])[0]

    def check_reachability(self, target_point):
        score = self.evaluate_target_point(target_point)
        if score < self.threshold:
            return False
        else:
            return True

    # ---- JSON --------------------------------------------------------------------------------------
    def root_feature_dist_json(self):
        data = {'name': self.motion_primitive_model.name, 'feature_point': 'Hips'}
        data.update(_mixture_json(self.root_feature_dist))
        data.update({'threshold': self.root_threshold, 'feature_type': self.root_feature_dist_type})
        return data

    def save_root_feature_dist(self, save_filename):
        with open(save_filename, 'w') as outfile:
            json.dump(self.root_feature_dist_json(), outfile)

    def load_root_feature_dist(self, model_file):
        with open(model_file, 'r') as infile:
            data = json.load(infile)
        self.root_feature_dist = FeatureMixture(data['gmm_weights'], data['gmm_means'], data['gmm_covars'])
        self.root_feature_dist_type = data['feature_type']
        self.root_threshold = self.root_feature_threshold = data['threshold']      # (the reference's loader names it root_feature_threshold)

    def save_feature_distribution(self, save_filename):
        data = {'name': self.motion_primitive_model.name, 'feature_point': self.feature_point}
        data.update(_mixture_json(self.feature_point_dist))
        data['threshold'] = self.threshold
        with open(save_filename, 'w') as outfile:
            json.dump(data, outfile)

    def load_feature_dist(self, dist_file):
        with open(dist_file, 'r') as infile:
            data = json.load(infile)
        self.feature_point_dist = FeatureMixture(data['gmm_weights'], data['gmm_means'], data['gmm_covars'])
        self.threshold = data['threshold']

    def save_data(self, save_filename):
        output_data = {'motion_vectors': [list(map(float, v)) for v in self.low_dimension_vectors],
                       'feature_points': [list(map(float, v)) for v in self.feature_points],
                       'orientations': [list(map(float, v)) for v in self.orientations]}
        with open(save_filename, 'w') as outfile:
            json.dump(output_data, outfile)

    def load_data_from_json(self, data_file):
        with open(data_file, 'r') as infile:
            training_data = json.load(infile)
        self.low_dimension_vectors = training_data['motion_vectors']
        self.feature_points = training_data["feature_points"]
        self.orientations = training_data["orientations"]


# ---- the builder ---------------------------------------------------------------------------------------------------
class HipFeaturePointModelBuilder(object):
    """FeaturePointModelBuilder (feature_point_model_builder.py): the root-feature mixture of every primitive.  build() takes a
    graph (its .nodes), a dict {node_key: node or primitive} or nothing -- then every *_quaternion_mm.json below
    morphable_model_directory is loaded, keyed (elementary action, motion primitive) from the file name as the reference splits
    it.  The features of all nodes come from ONE mg_feature_points call; with time_warped=True among the model options the nodes
    whose motion is time-warped go in one mg_feature_points_warped call and the others in one mg_feature_points call."""

    def __init__(self, context=None, **model_options):
        self.morphable_model_directory = None
        self.skeleton_file = None
        self.n_samples = 10000
        self.context = context
        self.model_options = model_options        # passed to every HipFeaturePointModel (device=, max_components=, seed=, ...)

    def set_config(self, config_file_path):
        with open(config_file_path) as config_file:
            config = json.load(config_file)
        self.morphable_model_directory = config["model_data_dir"]
        self.skeleton_file = config["skeleton_file_dir"]
        self.n_samples = config["n_samples"]

    def _nodes_of_directory(self):
        from .motion_primitive import HipMotionPrimitive
        nodes, where = {}, {}
        for root, dirs, files in os.walk(self.morphable_model_directory):
            for file in sorted(files):
                if "_quaternion_mm.json" in file:
                    segments = file.split('_')
                    key = (segments[0], segments[1])
                    nodes[key] = HipMotionPrimitive(root + os.sep + file, context=self.context)
                    where[key] = root
        return nodes, where

    def build(self, graph_or_nodes=None):
        if graph_or_nodes is None:
            if self.morphable_model_directory is None:
                raise ValueError("no nodes and no model directory: call set_config or pass a graph")
            nodes, where = self._nodes_of_directory()
        else:
            nodes = dict(getattr(graph_or_nodes, "nodes", graph_or_nodes))
            where = {key: self.morphable_model_directory for key in nodes}
        models = {key: HipFeaturePointModel(node, None, **self.model_options) for key, node in nodes.items()}
        keys = list(models)
        latents = [models[key]._draw(self.n_samples) for key in keys]
        dtypes = set(S.dtype for S in latents)
        if len(dtypes) > 1:
            latents = [S.astype(np.float64) for S in latents]
        outs = [None] * len(keys)
        for warped in (True, False):
            which = [k for k, key in enumerate(keys) if models[key]._warps() == warped]
            if which:
                first = models[keys[which[0]]]
                got = first._features([models[keys[k]]._item(latents[k]) for k in which], first._root_outputs(), [models[keys[k]]._smooths() for k in which])
                for k, out in zip(which, got):
                    models[keys[k]]._require_window(out, str(keys[k]))
                    first._require_frame(out, 0, str(keys[k]))
                    outs[k] = out
        result = {}
        for key, out, S in zip(keys, outs, latents):
            model = models[key]
            model._take_root(out, S)
            model.convert_ori_to_angle_deg()
            model.model_root_dist()
            if where.get(key) is not None:
                name = key if isinstance(key, str) else '_'.join(str(k) for k in key[:2])
                model.save_root_feature_dist(where[key] + os.sep + '_'.join([name, "root_dist_angle.json"]))
            result[key] = model.root_feature_dist_json()
        self.models = models
        return result


# ---- every node's mixture against a set of targets ----------------------------------------------------------------
class HipReachabilityIndex(object):
    """The reachability mixtures of many nodes, on the device once, so that a planner's question -- which of a graph's N nodes
    get to each of M targets -- is ONE mg_mixture_scores launch over one upload of the targets instead of N score_samples calls.

    models: a {key: HipFeaturePointModel} dict, a built HipFeaturePointModelBuilder (its .models), or a directory of the
    reference's JSON files: *_root_dist_angle.json for which="root", keyed (elementary action, motion primitive) from the file
    name as the builder writes it; for which="points" every other *.json with gmm_weights, keyed by its "name".  which: "root"
    (root_feature_dist, root_threshold) or "points" (feature_point_dist, threshold).  The nodes keep the order of `models`
    (a directory: sorted file names).  host=True scores by mg_mixture_scores_host: the same statements on the host, no device."""

    def __init__(self, models, which="root", ctx=None, host=False):
        if which not in ("root", "points"):
            raise ValueError("which is 'root' or 'points', got %r" % (which,))
        self.which, self.ctx, self.host = which, ctx, bool(host)
        if isinstance(models, str):
            entries = self._entries_of_directory(models, which)
        else:
            models = getattr(models, "models", models)
            entries = []
            for key, model in models.items():
                dist, threshold = (model.feature_point_dist, model.threshold) if which == "points" else (model.root_feature_dist, model.root_threshold)
                if dist is None:
                    raise ValueError("node %r has no %s distribution" % (key, which))
                entries.append((key, dist.weights_, dist.means_, dist.covars_, threshold))
        self.keys = [e[0] for e in entries]
        self.mixtures = [_capi.FeatureMixture(ctx, w, mu, cov, -np.inf if thr is None else thr, host=self.host) for _, w, mu, cov, thr in entries]
        self._of = {key: k for k, key in enumerate(self.keys)}

    @staticmethod
    def _entries_of_directory(directory, which):
        entries = []
        for root, dirs, files in sorted(os.walk(directory)):
            for file in sorted(files):
                is_root = file.endswith("_root_dist_angle.json")
                if not file.endswith(".json") or is_root != (which == "root"):
                    continue
                with open(root + os.sep + file, 'r') as infile:
                    data = json.load(infile)
                if not isinstance(data, dict) or "gmm_weights" not in data:
                    continue
                segments = file.split('_')
                key = (segments[0], segments[1]) if is_root and len(segments) >= 5 else data.get("name", file[:-len(".json")])
                entries.append((key, data["gmm_weights"], data["gmm_means"], data["gmm_covars"], data.get("threshold")))
        return entries

    def __len__(self):
        return len(self.keys)

    def close(self):
        for mix in self.mixtures:
            mix.close()

    def _run(self, items, outputs):
        return _capi.mixture_scores_host(items, outputs) if self.host else _capi.mixture_scores(items, outputs, ctx=self.mixtures[0].ctx)

    def _all(self, targets, output):
        dims = sorted(set(mix.dim for mix in self.mixtures))
        if len(dims) > 1:
            raise ValueError("the index holds mixtures of %s dimensions: one set of targets cannot serve them all (scores_each takes a set per node)" % dims)
        targets = np.atleast_2d(np.asarray(targets, dtype=np.float64))
        if not self.mixtures:
            return np.zeros((0, len(targets)), dtype=bool if output == "reachable" else np.float64)
        if targets.shape[1] != dims[0]:
            raise ValueError("targets have %d features, but the mixtures expect %d" % (targets.shape[1], dims[0]))
        targets = np.ascontiguousarray(targets)
        return np.stack([out[output] for out in self._run([(mix, targets) for mix in self.mixtures], (output,))])

    def scores(self, targets):
        """(n_nodes, n_targets) log p of every target under every node's mixture: one launch, one upload of the targets."""
        return self._all(targets, "logp")

    def reachable(self, targets):
        """(n_nodes, n_targets) bool: not (log p < the node's threshold)."""
        return self._all(targets, "reachable")

    def reachable_nodes(self, target):
        """The keys of the nodes that reach the one target, in the index's order."""
        return [key for key, ok in zip(self.keys, self.reachable([target])[:, 0]) if ok]

    def best_nodes(self, targets):
        """Per target the key of the node with the highest log p; of equal scores the first in the index's order wins (NaN scores
        never do, unless a target has no other)."""
        scores = self.scores(targets)
        if not len(self.keys):
            raise ValueError("the index holds no node")
        with np.errstate(invalid="ignore"):
            filled = np.where(np.isnan(scores), -np.inf, scores)
        return [self.keys[k] for k in np.argmax(filled, axis=0)]

    def scores_each(self, targets_of, output="logp"):
        """{key: log p (n_key,)} of per-node target sets {key: targets (n_key, dim of that node)} in the same single launch; the
        nodes' mixtures may differ in dimension."""
        keys = list(targets_of)
        items = []
        for key in keys:
            mix = self.mixtures[self._of[key]]
            X = np.ascontiguousarray(np.atleast_2d(np.asarray(targets_of[key], dtype=np.float64)).reshape(-1, mix.dim))
            items.append((mix, X))
        if not items:
            return {}
        return {key: out[output] for key, out in zip(keys, self._run(items, (output,)))}
