"""Functional PCA of aligned motions on the device: the reference's construction/fpca (FunctionalData, PCAFunctionalData,
FPCASpatialData, FPCATimeSemantic, run_pca) and the align_frames=False leg of MotionModelConstructor.construct_model
(motion_model_constructor.py:355-524), shaped like the reference's classes so that a construction script swaps an import.

Spline fit: with given interior knots scipy's splrep solves min |B c - y|, B the (F, n_basis) cubic design matrix at
x = 0 .. F - 1.  B is the same for every motion and channel, so the host factors it once (QR, float64) into the (n_basis, F)
least-squares operator and the device applies it to every motion (mg_spline_fit_batch).
PCA: mg_pca_fit, one-sided Jacobi on the short side of the centred matrix; the projections are mg_pca_project /
mg_pca_backproject.  run_pca keeps the reference's quirk: npc comes from the k = max(1, min(shape) - 1) largest singular
values only (svds never computes the smallest) and k rows are returned.  Singular-vector signs: each row's entry of largest
magnitude is positive, the first one on ties (the reference's signs are whatever ARPACK returns).

spline_fit_host and pca_fit_host restate the two device calls in NumPy (np.linalg.svd); they are the yardstick of the CPU
tests.  The classes have no CPU fallback.
"""
import collections

import numpy as np

from . import _capi
from .synthetic import cubic_b_spline_knots

MAX_BASIS, MAX_FRAMES, MAX_SHORT_SIDE = _capi.MG_FPCA_MAX_BASIS, _capi.MG_FPCA_MAX_FRAMES, _capi.MG_PCA_MAX_SHORT
MAX_LONG_SIDE = _capi.MG_PCA_MAX_LONG
BSPLINE_DEGREE = 3


# ---- host restatements ---------------------------------------------------------------------------------------------------
def bspline_design_matrix(knots, x, degree=BSPLINE_DEGREE):
    """(len(x), n_basis) values of the B-splines of `knots` at x (de Boor's recurrence; x at the last knot belongs to the
    last interval, as in FITPACK)."""
    t = np.asarray(knots, dtype=np.float64)
    k = degree
    n = len(t) - k - 1
    B = np.zeros((len(x), n))
    for r, xv in enumerate(np.asarray(x, dtype=np.float64)):
        l = int(np.searchsorted(t, xv, side="right")) - 1
        l = min(max(l, k), n - 1)
        h = np.zeros(k + 1)
        h[0] = 1.0
        for j in range(1, k + 1):
            hh = h[:j].copy()
            h[0] = 0.0
            for i in range(j):
                li, lj = l + i + 1, l + i + 1 - j
                f = hh[i] / (t[li] - t[lj])
                h[i] = h[i] + f * (t[li] - xv)
                h[i + 1] = f * (xv - t[lj])
        B[r, l - k:l + 1] = h
    return B


def spline_fit_operator(n_basis, n_frames):
    """The (n_basis, n_frames) operator c = P y of min |B c - y| on the reference's knots, from the QR factors of B."""
    knots = cubic_b_spline_knots(n_basis, n_frames)
    B = bspline_design_matrix(knots, np.arange(n_frames))
    Q, R = np.linalg.qr(B)
    return np.ascontiguousarray(np.linalg.solve(R, Q.T)), knots


def spline_fit_host(motion_mat, n_basis):
    """FunctionalData.convert_motions_to_functional_data: (N, F, D) -> (N, n_basis, D)."""
    motion_mat = np.asarray(motion_mat, dtype=np.float64)
    P, _ = spline_fit_operator(n_basis, motion_mat.shape[1])
    return np.einsum("bf,nfd->nbd", P, motion_mat)


def apply_sign_rule(Vt):
    """Each row's entry of largest magnitude made positive (the first one on ties)."""
    Vt = np.array(Vt, dtype=np.float64)
    for row in Vt:
        if row[np.argmax(np.abs(row))] < 0:
            row *= -1
    return Vt


def pca_fit_host(A, centre=True):
    """What _capi.pca_fit returns, from np.linalg.svd: mean, centred, singular_values and vt (all min(N, P), sign rule)."""
    A = np.asarray(A, dtype=np.float64)
    mean = A.mean(axis=0) if centre else np.zeros(A.shape[1])
    centred = A - mean
    _, s, Vt = np.linalg.svd(centred, full_matrices=False)
    return {"mean": mean, "centred": centred, "singular_values": s, "vt": apply_sign_rule(Vt)}


def npc_from_singular_values(singular_values, shape, fraction):
    """run_pca's choice (fpca/utils.py:33-52): the cumulated variance over the k = max(1, min(shape) - 1) largest values only."""
    assert 0 <= fraction <= 1
    k = max(1, min(shape) - 1)
    eigen = np.asarray(singular_values, dtype=np.float64)[:k] ** 2
    sumvariance = np.cumsum(eigen)
    sumvariance /= sumvariance[-1]
    return k, int(np.searchsorted(sumvariance, fraction) + 1)


CLOSE_ATOL, CLOSE_RTOL, REPAIR_STEP = 1e-8, 1e-5, 0.01


def _nearly_equal(a, b):
    """NumPy's default closeness of a to b (what the reference's repair asks np.allclose)."""
    return abs(a - b) <= CLOSE_ATOL + CLOSE_RTOL * abs(b)


def get_monotonic_indices(indices, epsilon=REPAIR_STEP):
    """What FPCATimeSemantic._get_monotonic_indices makes of control points that do not rise: two short sequential passes
    over the interior points, on the host.  Forwards, a point at or below its left neighbour is lifted by `epsilon` as often
    as it takes to stand above it and not nearly equal to it.  Backwards from the end, points are lowered in the same steps
    against their right neighbour, and the pass ends at the first point that is already below it.  The steps are repeated
    additions, not one multiple: the result's bits depend on it."""
    v = np.array(indices, dtype=np.float64)
    last = len(v) - 1
    if v[0] == v[last]:
        raise ValueError("a warping function must end above its start")
    for i in range(1, last):
        left = v[i - 1]
        if v[i] <= left:
            while v[i] <= left or _nearly_equal(v[i], left):
                v[i] += epsilon
    i = last - 1
    while i > 0 and not v[i] < v[i + 1]:
        right = v[i + 1]
        while v[i] >= right or _nearly_equal(v[i], right):
            v[i] -= epsilon
        i -= 1
    return v


def is_strict_increasing(indices):
    """No step down and no neighbours nearly equal (the reference's test after the repair)."""
    v = np.asarray(indices, dtype=np.float64)
    return bool(np.all(v[1:] >= v[:-1]) and not np.any(np.abs(v[1:] - v[:-1]) <= CLOSE_ATOL + CLOSE_RTOL * np.abs(v[:-1])))


def z_t_transform_vector(vec):
    """The z-t transform of one row of control points (FPCATimeSemantic.z_t_transform_vector): start moved to 0, repair,
    then the logarithm of the increments of 1 + w with a leading increment from 0 (which is 1: the first entry is 0)."""
    w = np.array(vec, dtype=np.float64)
    w = get_monotonic_indices(w - w[0])
    if not is_strict_increasing(w):
        raise AssertionError("the monotonic repair left control points that do not rise")
    raised = w + 1.0
    steps = np.empty_like(raised)
    steps[0] = raised[0]
    steps[1:] = raised[1:] - raised[:-1]
    return np.log(steps)


def temporal_functional_data_host(coeffs, warping_functions):
    """The host's part of FPCATimeSemantic.functional_data_representation after the spline fit: the end control points
    overwritten with the function's ends, then the z-t transform, per warping function."""
    coeffs = np.array(coeffs, dtype=np.float64)
    w = np.asarray(warping_functions, dtype=np.float64)
    coeffs[:, 0], coeffs[:, -1] = w[:, 0], w[:, -1]
    return np.asarray([z_t_transform_vector(c) for c in coeffs])


def get_max_translation(motions):
    m = np.zeros(3)
    for frames in motions.values():
        m = np.maximum(m, np.max(np.abs(np.asarray(frames)[:, :3]), axis=0))
    return m


def normalize_root_translation(motions):
    """construction/utils.py normalize_root_translation: root channels divided by their largest magnitudes over all motions;
    if a channel never leaves 0 nothing is scaled and the scale is reported as ones."""
    scale_vec = get_max_translation(motions)
    if not np.all(scale_vec):
        return motions, np.array([1, 1, 1])
    scaled = collections.OrderedDict((key, np.array(frames, dtype=np.float64)) for key, frames in motions.items())
    for frames in scaled.values():
        frames[:, :3] /= scale_vec
    return scaled, scale_vec


def align_quaternion_frames(n_animated_joints, motions):
    """construction/utils.py:161-184: every joint quaternion flipped into the hemisphere of the first frame of the first motion."""
    first = np.asarray(next(iter(motions.values())), dtype=np.float64)[0]
    out = collections.OrderedDict()
    for key, m in motions.items():
        m = np.array(m, dtype=np.float64)
        for j in range(n_animated_joints):
            o = 3 + 4 * j
            flip = m[:, o:o + 4] @ first[o:o + 4] < 0
            m[flip, o:o + 4] *= -1
        out[key] = m
    return out


def scale_root_translation_in_fpca_data(mean, eigen_vectors, scale_vec, n_coeffs, n_dims):
    mean, eigen_vectors = np.array(mean, dtype=np.float64), np.array(eigen_vectors, dtype=np.float64)
    for axis in range(3):
        cols = np.arange(n_coeffs) * n_dims + axis
        eigen_vectors[:, cols] *= scale_vec[axis]
        mean[cols] *= scale_vec[axis]
    return mean, eigen_vectors


def gen_gaussian_eigen(covars):
    """construction/utils.py:201-210 (v3 files): rows of sqrt(eigenvalue) * eigenvector per covariance."""
    covars = np.asarray(covars, dtype=np.float64)
    eigen = np.empty(covars.shape)
    for i, covar in enumerate(covars):
        s, U = np.linalg.eigh(covar)
        eigen[i] = np.transpose(U * np.sqrt(s.clip(0)))
    return eigen


# ---- the device ------------------------------------------------------------------------------------------------------------
class _DevicePCA(object):
    """mg_pca_fit of a device matrix and the projections on its leading rows; owns the centred matrix on the device."""

    def __init__(self, ctx, a_dev, n, p, centre=True):
        self.ctx, self.n, self.p = ctx, int(n), int(p)
        self.vt_dev = self.mean_dev = self.centred_dev = None
        if min(self.n, self.p) > MAX_SHORT_SIDE or max(self.n, self.p) > MAX_LONG_SIDE:
            raise ValueError("PCA of a %d x %d matrix: the short side may have at most %d, the long side %d" % (self.n, self.p, MAX_SHORT_SIDE,
                                                                                                            MAX_LONG_SIDE))
        with ctx.buffers() as bufs:
            centred_dev = bufs.malloc(8 * self.n * self.p)
            self.fit = _capi.pca_fit(ctx, a_dev, n, p, centred_dev, centre)
            self.centred_dev = bufs.release(centred_dev)

    def centred(self):
        return self.ctx.download(self.centred_dev, (self.n, self.p), np.float64)

    def use(self, eigenvectors):
        self.free_basis()
        self.l = len(eigenvectors)
        self.vt_dev = self.ctx.upload(np.ascontiguousarray(eigenvectors, dtype=np.float64))
        self.mean_dev = self.ctx.upload(self.fit["mean"])

    def project(self, x_dev, n):
        with self.ctx.buffers() as bufs:
            low_dev = bufs.malloc(8 * int(n) * self.l)
            _capi.pca_project(self.ctx, x_dev, self.vt_dev, n, self.p, self.l, low_dev)
            return self.ctx.download(low_dev, (int(n), self.l), np.float64)

    def project_host(self, data):
        data = np.ascontiguousarray(data, dtype=np.float64).reshape(-1, self.p)
        if self.l == 0 or len(data) == 0:
            return np.zeros((len(data), self.l))
        with self.ctx.buffers() as bufs:
            return self.project(bufs.upload(data), len(data))

    def backproject_host(self, low_vecs):
        low = np.ascontiguousarray(low_vecs, dtype=np.float64).reshape(-1, self.l)
        if self.l == 0 or len(low) == 0:
            return np.tile(self.fit["mean"], (len(low), 1))
        with self.ctx.buffers() as bufs:
            low_dev, high_dev = bufs.upload(low), bufs.malloc(8 * len(low) * self.p)
            _capi.pca_backproject(self.ctx, low_dev, self.vt_dev, self.mean_dev, len(low), self.p, self.l, high_dev)
            return self.ctx.download(high_dev, (len(low), self.p), np.float64)

    def free_basis(self):
        for buf in (self.vt_dev, self.mean_dev):
            if buf is not None:
                buf.free()
        self.vt_dev = self.mean_dev = None

    def free_centred(self):
        if self.centred_dev is not None:
            self.centred_dev.free()
        self.centred_dev = None

    def close(self):
        self.free_basis()
        self.free_centred()


def run_pca(A, fraction=0.90, ctx=None):
    """fpca/utils.py run_pca on the device: (Vt, npc), Vt the k = max(1, min(A.shape) - 1) leading right singular vectors of A
    as it is (not centred again), npc from the cumulated variance over those k values."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    ctx = _capi.default_context(ctx)
    with ctx.buffers() as bufs:
        pca = _DevicePCA(ctx, bufs.upload(A), A.shape[0], A.shape[1], centre=False)
        pca.close()
    k, npc = npc_from_singular_values(pca.fit["singular_values"], A.shape, fraction)
    return pca.fit["vt"][:k], npc


def _spline_fit_device(ctx, bufs, motions, n_basis):
    """The spline coefficients (n, n_basis, n_dims) of the host motions (n, n_frames, n_dims), a device buffer of the scope
    `bufs`, and the knots.  The uploaded motions and the operator are gone when this returns: what the caller allocates next
    (the PCA's work matrices) does not sit on top of them."""
    n, n_frames, n_dims = motions.shape
    if n_basis > MAX_BASIS or n_frames > MAX_FRAMES:
        raise ValueError("spline fit: n_basis = %d (at most %d), n_frames = %d (at most %d)" % (n_basis, MAX_BASIS, n_frames, MAX_FRAMES))
    P, knots = spline_fit_operator(n_basis, n_frames)
    with ctx.buffers() as inputs:
        m_dev, op_dev, coeffs_dev = inputs.upload(motions), inputs.upload(P), bufs.malloc(8 * n * n_basis * n_dims)
        _capi.spline_fit_batch(ctx, m_dev, n, n_frames, n_dims, op_dev, n_basis, coeffs_dev)
    return coeffs_dev, knots


class HipFunctionalData(object):
    """FunctionalData (fpca/functional_data.py) with the fits of all motions and channels in one device call."""

    def __init__(self, ctx=None):
        self.knots = None
        self.ctx = ctx

    def get_knots(self, n_basis, n_frames):
        self.knots = cubic_b_spline_knots(n_basis, n_frames)

    def convert_motions_to_functional_data(self, motion_mat, n_basis, degree=3):
        assert degree == BSPLINE_DEGREE
        motion_mat = np.ascontiguousarray(motion_mat, dtype=np.float64)
        n, n_frames, n_dims = motion_mat.shape
        ctx = _capi.default_context(self.ctx)
        with ctx.buffers() as bufs:
            c_dev, self.knots = _spline_fit_device(ctx, bufs, motion_mat, n_basis)
            return ctx.download(c_dev, (n, n_basis, n_dims), np.float64)

    def convert_motion_to_functional_data(self, motion_data, n_basis=7, degree=3):
        return self.convert_motions_to_functional_data(np.asarray(motion_data)[None], n_basis, degree)[0]


class HipPCAFunctionalData(object):
    """PCAFunctionalData (fpca/pca_functional_data.py): spline fit, centring, PCA and projection without leaving the device
    in between.  singular_values_ (all min(N, P) of them), n_sweeps_ and pca_status_ are ours.  After construction only the
    eigenvectors and the mean stay on the device (for project_data / backproject_data); they go with the object, or with
    close()."""

    def __init__(self, input_data, n_basis=7, fraction=0.90, n_pc=None, ctx=None):
        self.input_data = np.ascontiguousarray(input_data, dtype=np.float64)
        assert len(self.input_data.shape) == 3, ('input data should be a 3d array')
        self.n_basis = n_basis
        self.ctx = _capi.default_context(ctx)
        n, n_frames, n_dims = self.input_data.shape
        p = n_basis * n_dims
        with self.ctx.buffers() as bufs:
            c_dev, self.knots = _spline_fit_device(self.ctx, bufs, self.input_data, n_basis)
            self.functional_data = self.ctx.download(c_dev, (n, n_basis, n_dims), np.float64)
            self.origin_shape = (n, n_basis, n_dims)
            self._pca = _DevicePCA(self.ctx, c_dev, n, p)      # the flat index coeff * D + d is the table's own
        fit = self._pca.fit
        self.reshaped_fd, self.mean = self._pca.centred(), fit["mean"]
        self.singular_values_, self.n_sweeps_, self.pca_status_ = fit["singular_values"], fit["n_sweeps"], fit["status"]
        k, self.npc_ = npc_from_singular_values(self.singular_values_, (n, p), fraction)
        Vt = fit["vt"][:k]
        self.eigenvectors = Vt[:self.npc_] if n_pc is None else Vt[:n_pc]
        self._pca.use(self.eigenvectors)
        self.low_vecs = self._pca.project(self._pca.centred_dev, n)
        self._pca.free_centred()       # reshaped_fd is its host copy; what stays on the device is the basis and the mean

    def convert_to_fd(self):
        return HipFunctionalData(self.ctx).convert_motions_to_functional_data(self.input_data, self.n_basis)

    @classmethod
    def reshape_fd(cls, functional_data):
        assert len(functional_data.shape) == 3, ("functional data should be a 3d array")
        n_samples, n_coefs, n_dim = functional_data.shape
        return np.reshape(functional_data, (n_samples, n_coefs * n_dim)).copy(), (n_samples, n_coefs, n_dim)

    @classmethod
    def from_pca_to_data(cls, data, original_shape):
        return np.reshape(np.asarray(data), original_shape).copy()

    def project_data(self, data):
        return self._pca.project_host(data)

    def backproject_data(self, low_vecs):
        return self._pca.backproject_host(low_vecs)

    def close(self):
        self._pca.close()


class HipFPCASpatialData(object):
    """FPCASpatialData (fpca/fpca_spatial_data.py)."""

    def __init__(self, n_basis, n_components=None, fraction=0.95, ctx=None):
        self.n_basis = n_basis
        self.fraction = fraction
        self.reshaped_data = None
        self.fpcaobj = None
        self.fileorder = None
        self.n_components = n_components
        self.ctx = ctx

    def fit_motion_dictionary(self, motion_dic):
        self.fileorder = list(motion_dic.keys())
        self.fit(np.asarray(list(motion_dic.values())))

    def fit(self, motion_data):
        assert len(motion_data.shape) == 3
        self.fpcaobj = HipPCAFunctionalData(motion_data, n_basis=self.n_basis, fraction=self.fraction, n_pc=self.n_components, ctx=self.ctx)


class HipFPCATimeSemantic(object):
    """FPCATimeSemantic (fpca/fpca_time_semantic.py) for warping functions without semantic channels: set
    temporal_semantic_data to the (N, F) warping functions (or pass temporal_data, a dict of them), then functional_pca()."""

    def __init__(self, n_basis, n_components_temporal=None, precision_temporal=0.99, temporal_data=None, ctx=None):
        self.n_basis = n_basis
        self.n_components_temporal = n_components_temporal
        self.precision_temporal = precision_temporal
        self.semantic_annotation_list = []
        self.temporal_semantic_data = None
        self.file_order = None
        if temporal_data is not None:
            self.file_order = list(temporal_data.keys())
            self.temporal_semantic_data = np.asarray(list(temporal_data.values()), dtype=np.float64)
        self.ctx = ctx
        self.fpca_data = self.mean_vec = self.eigenvectors = self.lowVs = self.npc = None

    def get_b_spline_knots(self, n_basis, n_canonical_frames):
        return cubic_b_spline_knots(n_basis, n_canonical_frames)

    def functional_data_representation(self):
        w = np.ascontiguousarray(self.temporal_semantic_data, dtype=np.float64)
        assert w.ndim == 2, "warping functions (N, F) expected (semantic annotation channels are not supported)"
        n, n_frames = w.shape
        ctx = _capi.default_context(self.ctx)
        with ctx.buffers() as bufs:
            c_dev, _ = _spline_fit_device(ctx, bufs, w[:, :, None], self.n_basis)
            coeffs = ctx.download(c_dev, (n, self.n_basis), np.float64)
        self.fpca_data = temporal_functional_data_host(coeffs, w)

    def functional_pca(self):
        self.functional_data_representation()
        ctx = _capi.default_context(self.ctx)
        n, p = self.fpca_data.shape
        with ctx.buffers() as bufs:
            pca = _DevicePCA(ctx, bufs.upload(self.fpca_data), n, p)
        self.fpca_data, self.mean_vec = pca.centred(), pca.fit["mean"]
        self.singular_values_, self.n_sweeps_, self.pca_status_ = pca.fit["singular_values"], pca.fit["n_sweeps"], pca.fit["status"]
        k, npc = npc_from_singular_values(self.singular_values_, (n, p), self.precision_temporal)
        Vt = pca.fit["vt"][:k]
        self.eigenvectors = Vt[:self.n_components_temporal] if self.n_components_temporal is not None else Vt[:npc]
        try:
            pca.use(self.eigenvectors)
            self.lowVs = pca.project(pca.centred_dev, n)
        finally:
            pca.close()
        self.npc = npc

    def project_data(self, data):
        return np.asarray([np.dot(self.eigenvectors, row) for row in np.asarray(data)])


# ---- construct_model without the alignment -----------------------------------------------------------------------------------
def model_to_json(spatial, temporal, gmm_data, n_frames, config, animated_joints, frame_time, name="", version=1, keyframes=None):
    """MotionModelConstructor.convert_motion_model_to_json (versions 1, 2 and 3) from the stage results."""
    weights, means, covars = gmm_data['gmm_weights'], gmm_data['gmm_means'], gmm_data['gmm_covars']
    mean_motion = np.asarray(spatial["mean"]).tolist()
    spatial_eigenvectors = np.asarray(spatial["eigenvectors"]).tolist()
    scale_vec, n_dim_spatial, n_basis_spatial = spatial["scale_vec"], spatial["n_dim"], spatial["n_basis"]
    spatial_knots = cubic_b_spline_knots(n_basis_spatial, n_frames).tolist()
    if temporal is not None:
        temporal_mean = np.asarray(temporal["mean"]).tolist()
        temporal_eigenvectors = np.asarray(temporal["eigenvectors"]).tolist()
        n_basis_temporal = temporal["n_basis"]
        temporal_knots = cubic_b_spline_knots(n_basis_temporal, n_frames).tolist()
        semantic_label = temporal["semantic_annotation"]
    else:
        temporal_mean, temporal_eigenvectors, n_basis_temporal, temporal_knots, semantic_label = [], [], 0, [], dict()
    if version == 1:
        data = {'name': name, 'gmm_weights': weights, 'gmm_means': means, 'gmm_covars': covars,
                'eigen_vectors_spatial': spatial_eigenvectors, 'mean_spatial_vector': mean_motion, 'n_canonical_frames': n_frames,
                'translation_maxima': scale_vec, 'n_basis_spatial': n_basis_spatial, 'npc_spatial': len(spatial_eigenvectors),
                'eigen_vectors_temporal_semantic': temporal_eigenvectors, 'mean_temporal_semantic_vector': temporal_mean,
                'n_dim_spatial': n_dim_spatial, 'n_basis_temporal_semantic': n_basis_temporal,
                'b_spline_knots_spatial': spatial_knots, 'b_spline_knots_temporal_semantic': temporal_knots,
                'npc_temporal_semantic': config["npc_temporal"], 'semantic_annotation': {}, 'n_dim_temporal_semantic': 1}
    elif version == 2:
        data = {'name': name, 'gmm_weights': weights, 'gmm_means': means, 'gmm_covars': covars,
                'eigen_vectors_spatial': spatial_eigenvectors, 'mean_spatial_vector': mean_motion, 'n_canonical_frames': n_frames,
                'translation_maxima': scale_vec, 'n_basis_spatial': n_basis_spatial, 'eigen_vectors_time': temporal_eigenvectors,
                'mean_time_vector': temporal_mean, 'n_dim_spatial': n_dim_spatial, 'n_basis_time': n_basis_temporal,
                'b_spline_knots_spatial': spatial_knots, 'b_spline_knots_time': temporal_knots}
    else:
        data = {'sspm': {'eigen': spatial_eigenvectors, 'mean': mean_motion, 'n_coeffs': n_basis_spatial, 'n_dims': n_dim_spatial,
                         'knots': spatial_knots, 'animated_joints': animated_joints, 'degree': BSPLINE_DEGREE},
                'gmm': {'covars': covars, 'means': means, 'weights': weights, 'eigen': gen_gaussian_eigen(covars).tolist()},
                'tspm': {'eigen': temporal_eigenvectors, 'mean': temporal_mean, 'n_coeffs': n_basis_temporal, 'n_dims': 1,
                         'knots': temporal_knots, 'degree': BSPLINE_DEGREE, 'semantic_labels': semantic_label, 'frame_time': frame_time}}
    data["keyframes"] = keyframes if keyframes is not None else dict()
    return data


def construct_motion_primitive_model(aligned_frames, temporal_data, config, n_animated_joints=None, animated_joints=None, name="", version=1,
                                     keyframes=None, frame_time=None, gmm_trainer=None, ctx=None, return_stages=False):
    """The align_frames=False leg of MotionModelConstructor.construct_model: aligned_frames {key: (F, D) quaternion frames},
    temporal_data {key: (F,) warping function} or None; config as the reference's (n_spatial_basis_factor, n_components,
    fraction, n_basis_functions_temporal, npc_temporal, precision_temporal).  Root normalisation, quaternion sign alignment,
    spatial and temporal fPCA, root rescale of mean and eigenvectors, HipGMMTrainer (or gmm_trainer: an object with fit and
    convert_model_to_json) on the concatenated latents, and the v1 / v2 / v3 dict.  The two things the reference takes from a
    skeleton are arguments: animated_joints (or their number) and frame_time.

    The dicts are the reference constructor's, key for key and shape for shape.  HipMotionPrimitive loads v1 as returned and
    v3 through model_io.primitive_dict_from_json; both loaders read the spatial model and the mixture and no time model.  A
    v2 dict built WITH temporal data does not load, here as in the reference: the constructor writes eigen_vectors_time as
    (npc_temporal, n_basis_time) while the loaders expect (n_basis_time, n_time_components), and the constructed time model
    (a PCA of log control-point increments) is not what back_project_time_function inverts."""
    if n_animated_joints is None:
        n_animated_joints = len(animated_joints)
    aligned_frames = collections.OrderedDict((k, np.asarray(v, dtype=np.float64)) for k, v in aligned_frames.items())
    key = list(aligned_frames.keys())[0]
    n_frames = len(aligned_frames[key])
    n_basis = int(n_frames * config["n_spatial_basis_factor"])
    scaled, scale_vec = normalize_root_translation(aligned_frames)
    smoothed = align_quaternion_frames(n_animated_joints, scaled)
    fpca_spatial = HipFPCASpatialData(n_basis, config["n_components"], config["fraction"], ctx=ctx)
    fpca_spatial.fileorder = list(smoothed.keys())
    fpca_spatial.fit(np.array(list(smoothed.values())))
    obj = fpca_spatial.fpcaobj
    spatial = {'parameters': obj.low_vecs, 'file_order': fpca_spatial.fileorder, 'n_basis': obj.n_basis,
               'n_coeffs': obj.functional_data.shape[1], 'n_dim': obj.functional_data.shape[2], 'scale_vec': [1, 1, 1]}
    spatial['mean'], spatial['eigenvectors'] = scale_root_translation_in_fpca_data(obj.mean, obj.eigenvectors, scale_vec, spatial['n_coeffs'],
                                                                                   spatial['n_dim'])
    obj.close()
    temporal = None
    if temporal_data is not None:
        ft = HipFPCATimeSemantic(config["n_basis_functions_temporal"], n_components_temporal=config["npc_temporal"],
                                 precision_temporal=config["precision_temporal"], ctx=ctx)
        ft.temporal_semantic_data = np.array([temporal_data[k] for k in temporal_data.keys()], dtype=np.float64)
        ft.functional_pca()
        temporal = {'eigenvectors': ft.eigenvectors, 'mean': ft.mean_vec, 'parameters': ft.lowVs, 'n_basis': ft.n_basis, 'n_dim': 1,
                    'semantic_annotation': []}
        motion_parameters = np.concatenate((spatial["parameters"], temporal["parameters"]), axis=1)
    else:
        motion_parameters = spatial["parameters"]
    if gmm_trainer is None:
        from .gmm_trainer import HipGMMTrainer
        gmm_trainer = HipGMMTrainer(ctx=ctx)
    gmm_trainer.fit(motion_parameters)
    gmm_data = gmm_trainer.convert_model_to_json()
    if animated_joints is None:
        animated_joints = list(range(n_animated_joints))
    data = model_to_json(spatial, temporal, gmm_data, n_frames, config, animated_joints, frame_time, name, version, keyframes)
    if return_stages:
        return data, {"spatial": spatial, "temporal": temporal, "motion_parameters": motion_parameters, "scale_vec": scale_vec,
                      "functional_data": obj.functional_data, "input_data": obj.input_data}
    return data
