"""The data-producing half of ClusterTreeBuilder (reference morphablegraphs/construction/cluster_tree_builder.py:
159-192, 293-301) on the HIP back end: drawing the training samples of a space partitioning, filtering them by
likelihood, and back-projecting them to frames for the feature maps.  The reference scores and back-projects one
sample at a time (`gmm.score([s])[0]`, `spline.evaluate(frame_idx)` per frame); here each method is one batched
call.  The Euclidean feature map of the feature trees (features.py:125-153: global positions of a set of joints in
every frame of every sample, then sklearn's PCA keeping 95 % of the variance) gets its positions from one forward-kinematics
launch (mg_joint_positions).  Clustering itself (k-means / KD tree construction, sklearn) is offline tooling and stays
where it is.

Method names and results are the reference's; `motion_primitive` is a HipMotionPrimitiveModelWrapper or a
HipMotionStateGraphNode.  There is no CPU fallback.
"""
import heapq

import numpy as np

from . import _capi


def point_clouds_host(positions, step):
    """The NumPy statement of mg_point_cloud_features' layout rule (features.py:139-150): positions (n, F, J, 3), the joints' global
    positions in EVERY canonical frame -> (n, F * J * 3) in which frame f holds the cloud of frame step * (f // step)."""
    P = np.asarray(positions, dtype=np.float64)
    if P.ndim != 4 or P.shape[3] != 3 or int(step) < 1:
        raise ValueError("positions must be (n, F, J, 3) and step at least 1")
    n, F = P.shape[0], P.shape[1]
    return P[:, int(step) * (np.arange(F) // int(step)), :, :].reshape(n, -1)


def _positive_largest(vt):
    """mg_pca_fit's sign rule: each row's entry of largest magnitude positive (the first one on ties)."""
    vt = np.array(vt, dtype=np.float64)
    for row in vt:
        if row[int(np.argmax(np.abs(row)))] < 0.0:
            row *= -1.0
    return vt


def pca_leading_host(x, fraction):
    """The NumPy statement of mg_pca_fit_leading: numpy.linalg.svd of the centred matrix, the components sklearn's PCA(n_components=
    fraction) keeps -- searchsorted(cumsum(ratio), fraction, side="right") + 1 with ratio = s^2 / sum(s^2) -- under mg_pca_fit's sign
    rule.  Returns {"mean", "k", "singular_values", "vt", "ratios"}."""
    X = np.asarray(x, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 2 or not 0.0 < float(fraction) < 1.0:
        raise ValueError("x must be (n >= 2, p) and fraction inside (0, 1)")
    mean = X.mean(axis=0)
    _, s, vt = np.linalg.svd(X - mean, full_matrices=False)
    ratios = s * s / np.sum(s * s)
    k = int(np.searchsorted(np.cumsum(ratios), float(fraction), side="right")) + 1
    k = min(k, len(s))
    return {"mean": mean, "k": k, "singular_values": s[:k].copy(), "vt": _positive_largest(vt[:k]), "ratios": ratios[:k].copy()}


class DevicePCAModel(object):
    """What map_to_euclidean_pca_on_device fitted, with sklearn's attribute names; transform(point_clouds) projects new samples
    (mg_pca_project)."""

    def __init__(self, ctx, fit):
        self.ctx = ctx
        self.mean_ = fit["mean"]
        self.components_ = fit["vt"]
        self.singular_values_ = fit["singular_values"]
        self.explained_variance_ratio_ = fit["ratios"]
        self.n_components_ = int(fit["k"])
        self.n_iter_, self.status_ = int(fit["iterations"]), int(fit["status"])

    def transform(self, point_clouds):
        X = np.ascontiguousarray(np.asarray(point_clouds, dtype=np.float64) - self.mean_)
        if X.ndim != 2 or X.shape[1] != self.components_.shape[1]:
            raise ValueError("point_clouds must be (n, %d)" % self.components_.shape[1])
        n, p, k = X.shape[0], X.shape[1], self.n_components_
        if n == 0:
            return np.zeros((0, k))
        with self.ctx.buffers() as bufs:
            d_x, d_v, d_low = bufs.upload(X), bufs.upload(self.components_), bufs.malloc(8 * n * k)
            _capi.pca_project(self.ctx, d_x, d_v, n, p, k, d_low)
            return self.ctx.download(d_low, (n, k), np.float64)


def _log_likelihoods(motion_primitive, samples):
    """`get_gaussian_mixture_model().score([s])[0]` for every row (the reference's mixture wrappers return
    per-sample log-likelihoods from score(); extended_mgrd_mixture_model.py:100-108), in one launch."""
    return np.asarray(motion_primitive.get_gaussian_mixture_model().score_samples(np.asarray(samples)), dtype=np.float64)


class HipClusterTreeSampler(object):
    def __init__(self, n_samples=10000):
        self.n_samples = int(n_samples)          # cluster_tree_builder.py:124, config "n_random_samples"

    def set_config(self, config):
        self.n_samples = int(config["n_random_samples"])

    # cluster_tree_builder.py:159-175
    def _get_samples_using_threshold(self, motion_primitive, threshold=0, max_iter_count=5):
        """Rounds of n_samples draws, keeping the rows whose log-likelihood exceeds `threshold`, until n_samples
        are kept (every row of the round that crosses the line is kept, like the reference) or the rounds run
        out -> None."""
        data = []
        count = 0
        iter_count = 0
        while count < self.n_samples and iter_count < max_iter_count:
            samples = np.asarray(motion_primitive.sample_low_dimensional_vectors(self.n_samples))
            keep = _log_likelihoods(motion_primitive, samples) > threshold
            data.extend(samples[keep])
            count += int(keep.sum())
            iter_count += 1
        if iter_count < max_iter_count:
            return np.asarray(data)
        return None

    # cluster_tree_builder.py:177-189
    def _get_best_samples(self, motion_primitive):
        """2 n draws, likelihoods pushed on a heap as (-likelihood, idx); the FIRST n entries of the heap's list
        (heap order, not sorted order -- kept as the reference has it), shuffled."""
        data = np.asarray(motion_primitive.sample_low_dimensional_vectors(self.n_samples * 2))
        likelihoods = []
        for idx, likelihood in enumerate(_log_likelihoods(motion_primitive, data)):
            heapq.heappush(likelihoods, (-float(likelihood), idx))
        indices = [idx for _, idx in likelihoods[:self.n_samples]]
        data = data[indices]
        np.random.shuffle(data)
        return data

    # cluster_tree_builder.py:191-192
    def sample_data(self, motion_primitive):
        return motion_primitive.sample_low_dimensional_vectors(self.n_samples)

    # cluster_tree_builder.py:293-301
    def _back_project(self, mp, data):
        """(n, F, D): every sample evaluated at the integer canonical frames 0 .. F-1 (`spline.evaluate(frame_idx)`),
        float64 through the float64 frames path."""
        prim_obj = mp.motion_primitive if hasattr(mp, "motion_primitive") else mp
        prim = prim_obj._prim
        n_frames = int(mp.get_n_canonical_frames())
        S = np.asarray(data, dtype=np.float64)[:, :prim.n_components]
        grid = prim.time_grid(np.arange(n_frames, dtype=np.float64))
        try:
            return prim.back_project_frames_f64(S, grid)
        finally:
            grid.close()

    # cluster_tree_builder.py:266-291
    def _extract_features(self, motion_primitive, data, feature_type="latent", skeleton=None, joint_names=None, step=1, device_features=False):
        """The features a FeatureClusterTree is built on: the spatial latents themselves, or (feature_type "euclidean_pca",
        the reference's FEATURE_TYPE_EUCLIDEAN_PCA) the PCA projection of every sample's joint point cloud over its frames.
        skeleton: a _capi.Skeleton; joint_names: the reference passes END_EFFECTORS2 and step = 1.  device_features: the opt-in device
        route of "euclidean_pca" (map_to_euclidean_pca_on_device)."""
        if feature_type != "euclidean_pca":
            n_spatial = motion_primitive.get_n_spatial_components()
            return np.asarray(data)[:, :n_spatial]
        if device_features:
            return self.map_to_euclidean_pca_on_device(motion_primitive, data, skeleton, joint_names, step)[0]
        motions = self._back_project(motion_primitive, data)
        return self.map_motions_to_euclidean_pca(motion_primitive, motions, skeleton, joint_names, step)[0]

    # space_partitioning/features.py:133-153
    def map_motions_to_euclidean_space(self, motion_primitive, motions, skeleton, joint_names, step=4):
        """(n, F * len(joint_names) * 3): per sample the global positions of `joint_names` in its frames, flattened.  As
        in the reference a frame whose index is not a multiple of `step` REPEATS the cloud of the last one that is (its
        `sample.append(frame)` sits outside the `if idx % step == 0`), so the vector always has F entries."""
        prim_obj = motion_primitive.motion_primitive if hasattr(motion_primitive, "motion_primitive") else motion_primitive
        ctx = prim_obj._prim.ctx
        motions = np.asarray(motions, dtype=np.float64)
        n, F, D = motions.shape
        keep = np.arange(0, F, int(step))
        pos = ctx.joint_positions(skeleton, joint_names, motions[:, keep, :].reshape(-1, D)).reshape(n, len(keep), -1)
        return pos[:, np.arange(F) // int(step), :].reshape(n, -1)

    def point_clouds_on_device(self, motion_primitive, data, skeleton, joint_names, step=1):
        """map_motions_to_euclidean_space(_back_project(data)) without frames in memory (mg_point_cloud_features, one launch): a device
        buffer (n, F * len(joint_names) * 3) float64, the caller's to free; bit for bit the host route's array."""
        prim_obj = motion_primitive.motion_primitive if hasattr(motion_primitive, "motion_primitive") else motion_primitive
        prim = prim_obj._prim
        S = np.asarray(data)
        if S.dtype != np.float32:
            S = S.astype(np.float64)
        S = np.ascontiguousarray(S[:, :prim.n_components])
        n, F = S.shape[0], int(motion_primitive.get_n_canonical_frames())
        idx = skeleton.indices(joint_names)
        grid = prim.time_grid(np.arange(F, dtype=np.float64))      # the integer canonical frames, as _back_project evaluates them
        try:
            with prim.ctx.buffers() as bufs:
                d_S, d_out = bufs.upload(S), bufs.malloc(8 * n * F * len(idx) * 3)
                _capi.point_cloud_features_dev(prim, grid, skeleton, idx, step, d_S, S.dtype, n, S.shape[1], d_out)
                prim.ctx.synchronize()              # (d_S and the grid are freed on the way out)
                return bufs.release(d_out)
        finally:
            grid.close()

    def map_to_euclidean_pca_on_device(self, motion_primitive, data, skeleton, joint_names, step=1, fraction=0.95):
        """The device route of map_motions_to_euclidean_pca: the point clouds (point_clouds_on_device), their leading principal
        components (mg_pca_fit_leading, sklearn's count for n_components=fraction) and the projection (mg_pca_project) without the
        clouds leaving the device.  Returns (features (n, k) ndarray, model: a DevicePCAModel)."""
        prim_obj = motion_primitive.motion_primitive if hasattr(motion_primitive, "motion_primitive") else motion_primitive
        ctx = prim_obj._prim.ctx
        n = len(data)
        p = int(motion_primitive.get_n_canonical_frames()) * len(joint_names) * 3
        d_x = self.point_clouds_on_device(motion_primitive, data, skeleton, joint_names, step)
        try:
            with ctx.buffers() as bufs:
                d_c = bufs.malloc(8 * n * p)
                model = DevicePCAModel(ctx, _capi.pca_fit_leading(ctx, d_x, n, p, d_c, fraction))
                k = model.n_components_
                d_v, d_low = bufs.upload(model.components_), bufs.malloc(8 * n * k)
                _capi.pca_project(ctx, d_c, d_v, n, p, k, d_low)
                return ctx.download(d_low, (n, k), np.float64), model
        finally:
            d_x.free()

    # space_partitioning/features.py:125-130
    def map_motions_to_euclidean_pca(self, motion_primitive, motions, skeleton, joint_names, step=4):
        from sklearn.decomposition import PCA
        point_clouds = self.map_motions_to_euclidean_space(motion_primitive, motions, skeleton, joint_names, step)
        pca = PCA(n_components=0.95)
        return pca.fit_transform(point_clouds), pca
