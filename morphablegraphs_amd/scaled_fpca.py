"""Scaled functional PCA on the device: the reference's construction/fpca/scaled_fpca.py (ScaledFunctionalPCA) and the
objective sfpca_objective_func of construction/fpca/objective_functions.py -- the `scaling == 'scaled'` branch of
MotionDimensionReductor.optimize_feature_weights / MotionPrimitiveConstructor.reduce_dimensionality_using_scaled_fpca.

One weight per root channel and one per joint (its four quaternion channels share it) are chosen so that a PCA with npc
components of the weighted spline coefficients reconstructs the motions with the least error in joint-position space.

What the reference states and runs (steps 1 to 3 of the objective): the weights spread over the D = 3 + 4 J channels, sklearn
PCA(n_components=npc) fit_transform / inverse_transform of the weighted coefficients reshaped to (n, n_basis * D), the
reconstruction divided by the weights again.  With X the coefficient rows, Xc = X - mean and Dw the diagonal of spread
weights that reconstruction is mean + U_k U_k^T Xc, U the eigenvectors of Xc Dw^2 Xc^T = sum_g w_g^2 G_g, G_g the (n, n) Gram
matrix of group g's centred columns: the device forms the G_g once (mg_sfpca_create) and an objective value is a weighted sum
of them, the leading eigenvectors of an n x n matrix and one fused product / forward kinematics / reduction
(csrc/mg_sfpca.hip).

RESTATED, not the reference's (step 4): its modules motion_analysis.prepare_data (convert_quat_functional_data_to_cartesian_
functional_data) and utilities.custom_math (cartesian_splines_distance) are not in the reference tree, and anim_utils is not
installed, so the reference's scaled_fpca module does not import.  The error of a reconstruction here is the mean, over the n
samples, the sampled canonical frames f = 0, step, 2 step, ... < F and the chosen joints, of the squared Euclidean distance
between the joint's global position in the reconstructed and in the original motion; both motions are evaluated from their
control points by the cubic B-spline at those integer frames and go through the pose statements of mg_joint_positions (every
chain quaternion made unit and multiplied into the accumulated orientation, the child's offset turned by it and added).

optimize_weights keeps the reference's call -- scipy.optimize.minimize, method "SLSQP", bounds (0.0001, None), maxiter 1000 --
without its options maxfun and gtol, which are not SLSQP options (scipy warns and ignores them).  The gradient is SLSQP's own
forward difference, absolute step 1.4901161193847656e-08, from ONE mg_sfpca_errors call over the 3 + J + 1 points.  Reading and
writing the weight JSON files stays out.

sfpca_errors_host is the NumPy statement (numpy.linalg.svd of the weighted centred matrix, exactly as steps 1 to 3 read); it
needs no library.  Its forward kinematics, joint_positions_host, is feature_point_model.joint_position_host stated for all
frames at once (tests/test_scaled_fpca_host.py holds one to the other).  The class has no CPU fallback.
"""
import numpy as np

from . import _capi
from .fpca import apply_sign_rule, bspline_design_matrix

LEN_CARTESIAN, LEN_QUAT = 3, 4
SLSQP_EPSILON = 1.4901161193847656e-08        # scipy's _minimize_slsqp default eps = sqrt(machine epsilon)
WEIGHT_LOWER_BOUND, MAX_ITERATIONS = 0.0001, 1000
MAX_SAMPLES, MAX_BASIS, MAX_JOINTS = _capi.MG_SFPCA_MAX_SAMPLES, _capi.MG_SFPCA_MAX_BASIS, _capi.MG_SFPCA_MAX_JOINTS


# ---- host restatements ---------------------------------------------------------------------------------------------------
def spread_weights(weights, n_dims):
    """(m, 3 + J) weights -> (m, D = 3 + 4 J): a root channel its own weight, a joint's four channels its one."""
    w = np.atleast_2d(np.asarray(weights, dtype=np.float64))
    n_joints = (int(n_dims) - LEN_CARTESIAN) // LEN_QUAT
    if LEN_CARTESIAN + LEN_QUAT * n_joints != int(n_dims) or w.shape[1] != LEN_CARTESIAN + n_joints:
        raise ValueError("%d weights for %d channels (3 + J weights, 3 + 4 J channels)" % (w.shape[1], n_dims))
    return np.concatenate([w[:, :LEN_CARTESIAN], np.repeat(w[:, LEN_CARTESIAN:], LEN_QUAT, axis=1)], axis=1)


def sampled_frames(n_frames, step=1):
    return np.arange(0, int(n_frames), int(step))


def sampled_design(knots, n_frames, step=1):
    """The (F', n_basis) design rows at the sampled canonical frames 0, step, ... < n_frames."""
    return bspline_design_matrix(knots, sampled_frames(n_frames, step).astype(np.float64))


def joint_positions_host(skeleton, frames, joints):
    """(N, D) pose vectors -> (N, len(joints), 3): feature_point_model.joint_position_host's loop for every frame at once."""
    frames = np.asarray(frames, dtype=np.float64)
    out = np.empty((len(frames), len(joints), 3))
    for k, joint in enumerate(joints):
        chain = skeleton.chain(joint)
        p = frames[:, :3].copy()
        q = np.zeros((len(frames), 4))
        q[:, 0] = 1.0
        for parent, child in zip(chain[:-1], chain[1:]):
            ch = int(skeleton.quat_channel[parent])
            if ch >= 0:
                b = frames[:, ch:ch + 4]
                b = b / np.sqrt(np.sum(b * b, axis=1))[:, None]
                q = np.stack([q[:, 0] * b[:, 0] - q[:, 1] * b[:, 1] - q[:, 2] * b[:, 2] - q[:, 3] * b[:, 3],
                              q[:, 0] * b[:, 1] + q[:, 1] * b[:, 0] + q[:, 2] * b[:, 3] - q[:, 3] * b[:, 2],
                              q[:, 0] * b[:, 2] - q[:, 1] * b[:, 3] + q[:, 2] * b[:, 0] + q[:, 3] * b[:, 1],
                              q[:, 0] * b[:, 3] + q[:, 1] * b[:, 2] - q[:, 2] * b[:, 1] + q[:, 3] * b[:, 0]], axis=1)
            v = np.broadcast_to(np.asarray(skeleton.offsets[child], dtype=np.float64), p.shape)
            u = q[:, 1:]
            p = p + (v + 2.0 * (q[:, :1] * np.cross(u, v) + np.cross(u, np.cross(u, v))))
        out[:, k] = p
    return out


def sfpca_reconstruct_host(coeffs, weights, npc):
    """Steps 1 to 3 of sfpca_objective_func for ONE weight vector: (n, n_basis, D) -> the unweighted reconstruction, same
    shape.  PCA as sklearn's full solver states it: numpy.linalg.svd of the weighted centred matrix."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    n, n_basis, D = coeffs.shape
    ext = spread_weights(weights, D)[0]
    Xw = (coeffs * ext).reshape(n, n_basis * D)
    mean = Xw.mean(axis=0)
    U, s, Vt = np.linalg.svd(Xw - mean, full_matrices=False)
    k = int(npc)
    back = (U[:, :k] * s[:k]) @ Vt[:k] + mean
    return back.reshape(n, n_basis, D) / ext


def group_grams_host(coeffs):
    """The 3 + J Gram matrices G_g (n, n) of the centred coefficients' column groups."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    n, n_basis, D = coeffs.shape
    xc = coeffs - coeffs.mean(axis=0)
    groups = [[d] for d in range(LEN_CARTESIAN)] + [list(range(d, d + LEN_QUAT)) for d in range(LEN_CARTESIAN, D, LEN_QUAT)]
    out = np.empty((len(groups), n, n))
    for g, cols in enumerate(groups):
        a = xc[:, :, cols].reshape(n, -1)
        out[g] = a @ a.T
    return out


def projector_host(coeffs, weights, npc):
    """U_k (n, npc): the leading eigenvectors of sum_g w_g^2 G_g, each column's entry of largest magnitude positive."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    A = np.tensordot(w * w, group_grams_host(coeffs), axes=1)
    lam, U = np.linalg.eigh(A)
    order = np.argsort(-lam, kind="stable")[:int(npc)]
    return apply_sign_rule(U[:, order].T).T


def gram_reconstruct_host(coeffs, weights, npc):
    """mean + U_k U_k^T Xc with U_k from the Gram matrices: what steps 1 to 3 come to."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    mean = coeffs.mean(axis=0)
    xc = (coeffs - mean).reshape(len(coeffs), -1)
    U = projector_host(coeffs, weights, npc)
    return (U @ (U.T @ xc)).reshape(coeffs.shape) + mean


def reconstruction_error_host(coeffs, reconstruction, skeleton, design, joints, original_positions=None):
    """The restated step 4: mean squared joint-position distance between two sets of control points at the sampled frames."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    n, n_basis, D = coeffs.shape
    joints = [skeleton.index(j) for j in joints]
    if original_positions is None:
        original_positions = joint_positions_host(skeleton, np.einsum("fb,nbd->nfd", design, coeffs).reshape(-1, D), joints)
    frames = np.einsum("fb,nbd->nfd", design, np.asarray(reconstruction, dtype=np.float64)).reshape(-1, D)
    d = joint_positions_host(skeleton, frames, joints) - original_positions
    return float(np.mean(np.sum(d * d, axis=2)))


def sfpca_errors_host(coeffs, weights, npc, skeleton, design, joints):
    """The NumPy statement of mg_sfpca_errors: the restated error of every row of weights (m, 3 + J) -> (m,)."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    D = coeffs.shape[2]
    W = np.atleast_2d(np.asarray(weights, dtype=np.float64))
    idx = [skeleton.index(j) for j in joints]
    original = joint_positions_host(skeleton, np.einsum("fb,nbd->nfd", design, coeffs).reshape(-1, D), idx)
    return np.array([reconstruction_error_host(coeffs, sfpca_reconstruct_host(coeffs, w, npc), skeleton, design, idx, original) for w in W])


def forward_difference_points(x, epsilon=SLSQP_EPSILON):
    """The 3 + J + 1 points of one SLSQP gradient: x, then x with epsilon added to one entry at a time -- the points scipy's
    approx_derivative ('2-point', abs_step=epsilon, no upper bound) evaluates.  Returns (points, dx): dx = (x + epsilon) - x,
    the steps as they round, which scipy divides by."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    pts = np.repeat(x[None, :], len(x) + 1, axis=0)
    idx = np.arange(len(x))
    pts[idx + 1, idx] += epsilon
    return pts, pts[idx + 1, idx] - x


def scale_root_channels(functional_motion_data):
    """The reference's root scaling as heuristic_initialization uses it: the root channels' largest magnitudes over all
    samples and control points (ones where a channel never leaves 0)."""
    m = np.max(np.abs(np.asarray(functional_motion_data, dtype=np.float64)[:, :, :LEN_CARTESIAN]), axis=(0, 1))
    scale = np.where(m > 0.0, m, 1.0)
    scaled = np.array(functional_motion_data, dtype=np.float64)
    scaled[:, :, :LEN_CARTESIAN] /= scale
    return scaled, scale


# ---- the device ------------------------------------------------------------------------------------------------------------
def sfpca_objective_func(weights, data):
    """sfpca_objective_func(weights, data), batched over the rows of weights: data is a HipScaledFunctionalPCA (the
    reference's tuple holds what that object holds).  A 1-D vector gives a float, (m, 3 + J) rows give (m,) errors from one
    mg_sfpca_errors call."""
    w = np.asarray(weights, dtype=np.float64)
    errors = data.errors(np.atleast_2d(w))
    return float(errors[0]) if w.ndim == 1 else errors


class HipScaledFunctionalPCA(object):
    """ScaledFunctionalPCA.  functional_motion_data (n, n_basis, 3 + 4 n_joints) spline coefficients; npc; skeleton: a
    _capi.Skeleton whose animated joints are the data's quaternion channels; knots: the coefficients' knot vector (its last
    knot is the last canonical frame); joints: the joints whose positions are compared (names or indices; None: every joint
    of the skeleton); step: every step-th canonical frame is compared.  pca_statuses_ / n_objective_calls_ are ours."""

    def __init__(self, functional_motion_data, npc, skeleton, knots, n_joints, joints=None, step=1, ctx=None):
        self.functional_motion_data = np.ascontiguousarray(functional_motion_data, dtype=np.float64)
        assert self.functional_motion_data.ndim == 3, "functional data should be a 3d array"
        n, n_basis, n_dims = self.functional_motion_data.shape
        if n_dims != LEN_CARTESIAN + LEN_QUAT * int(n_joints):
            raise ValueError("%d channels are not 3 + 4 x %d joints" % (n_dims, n_joints))
        self.npc, self.skeleton, self.n_joints = int(npc), skeleton, int(n_joints)
        self.knots = np.asarray(knots, dtype=np.float64)
        self.n_frames = int(round(self.knots[-1])) + 1
        self.step = int(step)
        self.joints = skeleton.indices(range(len(skeleton.names)) if joints is None else joints)
        self.design = sampled_design(self.knots, self.n_frames, self.step)
        self.len_weights = self.n_joints + LEN_CARTESIAN
        self.ctx = _capi.default_context(ctx)
        self.weight_vec = None
        self.pca_statuses_ = None
        self.n_objective_calls_ = 0
        with self.ctx.buffers() as bufs:
            self._handle = _capi.ScaledFPCA(self.ctx, bufs.upload(self.functional_motion_data), n, n_basis, n_dims, skeleton, self.joints, self.design)

    def errors(self, weights):
        """The restated error of every row of weights (m, 3 + J), one device call."""
        self.n_objective_calls_ += 1
        errors, self.pca_statuses_ = self._handle.errors(weights, self.npc)
        return errors

    def heuristic_initialization(self):
        _, root_scale_vector = scale_root_channels(self.functional_motion_data)
        unscaled_weights = np.ones(self.len_weights)
        root_normalization_weights = np.ones(self.len_weights)
        root_normalization_weights[:LEN_CARTESIAN] = 1.0 / np.asarray(root_scale_vector)
        unscaled_error, root_normalization_error = self.errors(np.stack([unscaled_weights, root_normalization_weights]))   # two values, one call
        if unscaled_error > root_normalization_error:
            self.initialize_weights(root_normalization_weights)
        else:
            self.initialize_weights(unscaled_weights)

    def initialize_weights(self, weight_vec=None):
        self.weight_vec = np.array(weight_vec, dtype=np.float64) if weight_vec is not None else np.ones(self.len_weights)

    def _value_and_gradient(self, x):
        """f(x) and SLSQP's forward-difference gradient from one call over the 3 + J + 1 points."""
        pts, dx = forward_difference_points(x)
        f = self.errors(pts)
        return float(f[0]), (f[1:] - f[0]) / dx

    def optimize_weights(self, callback=None):
        """minimize(..., method="SLSQP", bounds=(0.0001, None), maxiter=1000); every value SLSQP asks for comes with its
        gradient from the same call, kept until the point changes.  Returns result.x; the OptimizeResult is result_."""
        from scipy.optimize import minimize
        if self.weight_vec is None:
            self.initialize_weights()
        cache = {}

        def both(x):
            key = np.asarray(x, dtype=np.float64).tobytes()
            if cache.get("key") != key:
                cache["key"], cache["value"] = key, self._value_and_gradient(x)
            return cache["value"]
        bnds = tuple((WEIGHT_LOWER_BOUND, None) for _ in range(len(self.weight_vec)))
        self.result_ = minimize(lambda x: both(x)[0], self.weight_vec, jac=lambda x: both(x)[1], bounds=bnds, method="SLSQP",
                                options={"maxiter": MAX_ITERATIONS}, callback=callback)
        return self.result_.x

    def fit(self, weight_vector=None):
        """The weights (given, or heuristic_initialization + optimize_weights), then the PCA of the weighted coefficients:
        components_ (npc, n_basis * D) and mean_ as sklearn's PCA holds them, from the device's projector."""
        if weight_vector is None:
            self.heuristic_initialization()
            weight_vector = self.optimize_weights()
        self.weight_vec = np.array(weight_vector, dtype=np.float64)
        n = len(self.functional_motion_data)
        ext = spread_weights(self.weight_vec, self.functional_motion_data.shape[2])[0]
        self.reshaped_functional_data = (self.functional_motion_data * ext).reshape(n, -1)
        self.mean_ = self.reshaped_functional_data.mean(axis=0)
        U, self.pca_status_ = self._handle.projector(self.weight_vec, self.npc)
        low = U.T @ (self.reshaped_functional_data - self.mean_)          # (npc, p) = S_k Vt_k
        self.singular_values_ = np.sqrt(np.sum(low * low, axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            self.components_ = np.where(self.singular_values_[:, None] > 0.0, low / self.singular_values_[:, None], 0.0)

    def transform(self):
        return (self.reshaped_functional_data - self.mean_) @ self.components_.T

    def inverse_transform(self, X):
        back = np.asarray(X, dtype=np.float64) @ self.components_ + self.mean_
        return back.reshape((-1,) + self.functional_motion_data.shape[1:])

    def close(self):
        self._handle.close()
