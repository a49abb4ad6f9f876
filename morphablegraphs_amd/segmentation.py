"""Cutting motion clips out of captures at keyframe poses on the device: the reference's construction/keyframe_detection.py
(argmin, argmin_multi, KeyframeDetector.find_instance / find_instances / calculate_distances) and construction/segmentation.py
(Segmentation.extract_single_segments / extract_segments), shaped like the reference's modules so that a construction script
swaps an import.  The slices extract_segments returns are the motions dtw.align_frames_temporally takes.

All captures go through ONE batched mg_keyframe_distances call (every frame's distance to the start and to the end keyframe,
each frame read once) and ONE mg_segment_search call; the clouds stay on the device from the forward kinematics
(mg_joint_positions) through the distances and the search, and only the (start, end) pairs and their counts come back.  For
given distances the pairs are the reference's exactly: every arg-min is the first index of the least value, the instances are
the frames with v <= min + threshold.  The distance itself is the cell of the DTW grids (csrc/mg_dtw.hip states the formula and
the order of its sums): the keyframe is fitted onto the frame; the reference's own, anim_utils'
_transform_invariant_point_cloud_distance, is not available: PARITY UNPINNED for the distances.

Differences from the reference:
  * non-finite distances or clouds are refused (ValueError on the host, MG_ERR_INVALID_ARGUMENT on the device); the reference's
    `v < min_v` silently skips a NaN;
  * find_instances2 / extracted_filtered_minima are not reproduced: nothing in the reference calls them, and under current
    NumPy detect_local_minima raises on its subtraction of boolean arrays.

argmin, argmin_multi, keyframe_distances_host and segment_search_host restate the reference and the two device calls in NumPy /
plain Python; they are the yardstick of the CPU tests.  The device functions have no CPU fallback.
"""
import numpy as np

from . import _capi
from .dtw import _offsets, distance_grid_host

SINGLE, MULTI = _capi.MG_SEGMENT_SINGLE, _capi.MG_SEGMENT_MULTI
MAX_KEYFRAMES, MAX_JOINTS = _capi.MG_SEGMENT_MAX_KEYFRAMES, _capi.MG_SEGMENT_MAX_JOINTS


# ---- host restatements ---------------------------------------------------------------------------------------------------
def argmin(values):
    """keyframe_detection.py argmin: the FIRST index of the least value (0 for no values)."""
    min_idx, min_v = 0, np.inf
    for idx, v in enumerate(values):
        if v < min_v:
            min_idx, min_v = idx, v
    return min_idx


def argmin_multi(values, threshold=1.0):
    """keyframe_detection.py argmin_multi: the indices, in order, of the values within `threshold` of the least."""
    min_v = np.inf
    for v in values:
        if v < min_v:
            min_v = v
    return [idx for idx, v in enumerate(values) if v <= min_v + threshold]


def _check_distances(start_dist, end_dist):
    s, e = np.asarray(start_dist, dtype=np.float64).reshape(-1), np.asarray(end_dist, dtype=np.float64).reshape(-1)
    if len(s) != len(e) or len(s) < 1:
        raise ValueError("segment search: %d start and %d end distances (one of each per frame, at least one frame)" % (len(s), len(e)))
    if not (np.all(np.isfinite(s)) and np.all(np.isfinite(e))):
        raise ValueError("segment search: the distances hold non-finite values")
    return s, e


def _check_search(mode, threshold, min_segment_size):
    if mode not in (SINGLE, MULTI):
        raise ValueError("segment search: mode %r" % (mode,))
    if mode == MULTI and (np.isnan(threshold) or int(min_segment_size) < 0):
        raise ValueError("segment search: threshold %r, min_segment_size %r" % (threshold, min_segment_size))


def segment_search_host(start_dist, end_dist, mode, threshold=1.0, min_segment_size=10):
    """What mg_segment_search writes for one motion: the list of kept (start, end) pairs.  SINGLE: extract_single_segments'
    pair; MULTI: the loop of segmentation.py:61-80."""
    _check_search(mode, threshold, min_segment_size)
    s, e = _check_distances(start_dist, end_dist)
    s, e = s.tolist(), e.tolist()
    if mode == SINGLE:
        return [(argmin(s), argmin(e))]
    instances = argmin_multi(s, threshold)
    segments = []
    for i, start in enumerate(instances):
        window_end = len(s) - 1 if i + 1 == len(instances) else instances[i + 1]
        if window_end - start < min_segment_size:
            continue
        end = start + argmin(e[start:window_end])
        if end - start > min_segment_size:
            segments.append((start, end))
    return segments


def _as_clouds(clouds, n_joints=None):
    out = [np.asarray(c, dtype=np.float64) for c in clouds]
    for c in out:
        if c.ndim != 3 or c.shape[2] != 3 or c.shape[1] != (out[0].shape[1] if n_joints is None else n_joints):
            raise ValueError("point clouds are (F, J, 3) arrays with one J")
    return out


def _check_limits(clouds, keyframes):
    if keyframes.ndim != 3 or keyframes.shape[2] != 3 or not 1 <= len(keyframes) <= MAX_KEYFRAMES:
        raise ValueError("keyframes: a (K, J, 3) array, 1 <= K <= %d" % MAX_KEYFRAMES)
    if not 1 <= keyframes.shape[1] <= MAX_JOINTS:
        raise ValueError("keyframe distances: %d joints (1 to %d)" % (keyframes.shape[1], MAX_JOINTS))
    if any(len(c) < 1 for c in clouds):
        raise ValueError("keyframe distances: a motion without frames")


def keyframe_distances_host(clouds, keyframes, weights=None):
    """What mg_keyframe_distances computes: per motion the (K, F_n) distances of its frames (clouds: a list of (F_n, J, 3)
    arrays) to the keyframes (K, J, 3); cell (frame, keyframe) of dtw.distance_grid_host."""
    keyframes = np.asarray(keyframes, dtype=np.float64)
    clouds = _as_clouds(clouds, keyframes.shape[1] if keyframes.ndim == 3 else None)
    _check_limits(clouds, keyframes)
    if not all(np.all(np.isfinite(c)) for c in clouds + [keyframes]):
        raise ValueError("keyframe distances: the point clouds or the keyframes hold non-finite values")
    return [np.ascontiguousarray(distance_grid_host(c, keyframes, weights).T) for c in clouds]


# ---- the device ------------------------------------------------------------------------------------------------------------
def _segment_offsets(lengths, mode, min_segment_size):
    room = [1 if mode == SINGLE else int(f) // (int(min_segment_size) + 1) + 1 for f in lengths]
    return _offsets(room)


def _search_on_device(ctx, bufs, start_dev, end_dev, off, mode, threshold, min_segment_size):
    """mg_segment_search and the download of its pairs: per motion a (count, 2) int32 array."""
    _check_search(mode, threshold, min_segment_size)
    n = len(off) - 1
    seg_off = _segment_offsets(np.diff(off), mode, min_segment_size)
    p_dev, c_dev = bufs.malloc(8 * int(seg_off[-1])), bufs.malloc(4 * n)
    _capi.segment_search(ctx, start_dev, end_dev, off, mode, threshold, min_segment_size, seg_off, p_dev, c_dev)
    counts = ctx.download(c_dev, (n,), np.int32)
    pairs = ctx.download(p_dev, (int(seg_off[-1]), 2), np.int32)
    return [pairs[int(seg_off[m]):int(seg_off[m]) + int(counts[m])].copy() for m in range(n)]


def keyframe_distances(clouds, keyframes, weights=None, ctx=None):
    """mg_keyframe_distances: per motion the (K, F_n) distances of the clouds (a list of (F_n, J, 3) arrays) to the keyframes
    (K, J, 3)."""
    ctx = _capi.default_context(ctx)
    keyframes = np.ascontiguousarray(keyframes, dtype=np.float64)
    clouds = _as_clouds(clouds, keyframes.shape[1] if keyframes.ndim == 3 else None)
    if not clouds:
        return []
    _check_limits(clouds, keyframes)
    off = _offsets([len(c) for c in clouds])
    k, total = len(keyframes), int(off[-1])
    with ctx.buffers() as bufs:
        c_dev, k_dev, d_dev = bufs.upload(np.concatenate(clouds)), bufs.upload(keyframes), bufs.malloc(8 * k * total)
        _capi.keyframe_distances(ctx, c_dev, off, keyframes.shape[1], k_dev, k, weights, d_dev)
        dist = ctx.download(d_dev, (k, total), np.float64)
    return [dist[:, int(off[m]):int(off[m + 1])].copy() for m in range(len(clouds))]


def segment_search(start_dists, end_dists, mode, threshold=1.0, min_segment_size=10, ctx=None):
    """mg_segment_search on given distances (two lists of (F_n,) arrays): per motion the (count, 2) int32 array of kept
    (start, end) pairs."""
    ctx = _capi.default_context(ctx)
    if len(start_dists) != len(end_dists):
        raise ValueError("segment search: %d and %d motions" % (len(start_dists), len(end_dists)))
    if not len(start_dists):
        return []
    s = [np.asarray(d, dtype=np.float64).reshape(-1) for d in start_dists]
    e = [np.asarray(d, dtype=np.float64).reshape(-1) for d in end_dists]
    if any(len(a) != len(b) or len(a) < 1 for a, b in zip(s, e)):
        raise ValueError("segment search: one start and one end distance per frame, at least one frame per motion")
    off = _offsets([len(a) for a in s])
    with ctx.buffers() as bufs:
        return _search_on_device(ctx, bufs, bufs.upload(np.concatenate(s)), bufs.upload(np.concatenate(e)), off, mode, threshold, min_segment_size)


class KeyframeDetector(object):
    """keyframe_detection.py KeyframeDetector on the device.  skeleton: a _capi.Skeleton, joints: the joints (names or indices)
    whose global positions make a frame's point cloud (mg_joint_positions); both may be None when only point clouds are handed
    in.  A motion is an (F, D) array of quaternion frames or an (F, J, 3) point cloud, a keyframe a (D,) pose or a (J, 3)
    cloud; one call takes one kind.  weights: per joint, None = ones (the reference has none)."""

    def __init__(self, skeleton, joints=None, ctx=None, weights=None):
        self._skeleton, self._joints, self._ctx, self._weights = skeleton, joints, ctx, weights

    def _clouds_to_device(self, ctx, bufs, motions, keyframes):
        """The clouds of the motions and, behind them, of the keyframes in one device table: (table, keyframes' address,
        offsets, n_joints)."""
        motions = [np.asarray(m, dtype=np.float64) for m in motions]
        keyframes = [np.asarray(k, dtype=np.float64) for k in keyframes]
        if not 1 <= len(keyframes) <= MAX_KEYFRAMES:
            raise ValueError("%d keyframes (1 to %d)" % (len(keyframes), MAX_KEYFRAMES))
        if any(len(m) < 1 for m in motions):
            raise ValueError("keyframe distances: a motion without frames")
        off = _offsets([len(m) for m in motions])
        total = int(off[-1])
        if all(m.ndim == 3 for m in motions) and all(k.ndim == 2 for k in keyframes):
            keys = np.stack(keyframes)
            clouds = _as_clouds(motions, keys.shape[1])
            _check_limits(clouds, keys)
            nj = keys.shape[1]
            c_dev = bufs.upload(np.concatenate(clouds + [keys]))
        elif all(m.ndim == 2 for m in motions) and all(k.ndim == 1 for k in keyframes):
            if self._skeleton is None or self._joints is None:
                raise ValueError("quaternion frames need a skeleton and the point cloud's joints")
            n_dim = len(keyframes[0])
            if any(m.shape[1] != n_dim for m in motions) or any(len(k) != n_dim for k in keyframes):
                raise ValueError("the motions and keyframes of one call have the same channels")
            idx = self._skeleton.indices(self._joints)
            nj = len(idx)
            if not 1 <= nj <= MAX_JOINTS:
                raise ValueError("keyframe distances: %d joints (1 to %d)" % (nj, MAX_JOINTS))
            rows = total + len(keyframes)
            f_dev, c_dev = bufs.upload(np.concatenate(motions + [np.stack(keyframes)])), bufs.malloc(8 * rows * nj * 3)
            ctx.joint_positions_dev(self._skeleton, idx, f_dev, rows, n_dim, c_dev)
        else:
            raise ValueError("one call takes quaternion frames with keyframe poses, or point clouds (F, J, 3) with keyframe clouds (J, 3)")
        return c_dev, c_dev.address + 8 * total * nj * 3, off, nj

    def _distances_on_device(self, ctx, bufs, motions, keyframes):
        c_dev, k_addr, off, nj = self._clouds_to_device(ctx, bufs, motions, keyframes)
        d_dev = bufs.malloc(8 * len(keyframes) * int(off[-1]))
        _capi.keyframe_distances(ctx, c_dev, off, nj, k_addr, len(keyframes), self._weights, d_dev)
        return d_dev, off

    def calculate_distances(self, point_clouds, keyframe):
        """Per motion the (F_n,) distances of its frames to the keyframe, all motions in one call."""
        if not len(point_clouds):
            return []
        ctx = _capi.default_context(self._ctx)
        with ctx.buffers() as bufs:
            d_dev, off = self._distances_on_device(ctx, bufs, point_clouds, [keyframe])
            dist = ctx.download(d_dev, (int(off[-1]),), np.float64)
        return [dist[int(off[m]):int(off[m + 1])].copy() for m in range(len(off) - 1)]

    def find_instance(self, point_cloud, keyframe):
        """The first frame closest to the keyframe."""
        ctx = _capi.default_context(self._ctx)
        with ctx.buffers() as bufs:
            d_dev, off = self._distances_on_device(ctx, bufs, [point_cloud], [keyframe])
            return int(_search_on_device(ctx, bufs, d_dev, d_dev, off, SINGLE, 0.0, 0)[0][0, 0])

    def find_instances(self, point_cloud, keyframe, threshold=1.0):
        """The frames, in order, whose distance to the keyframe is within `threshold` of the least."""
        d = self.calculate_distances([point_cloud], keyframe)[0]
        return [int(i) for i in np.flatnonzero(d <= d.min() + threshold)]


class Segmentation(object):
    """segmentation.py Segmentation on the device; see KeyframeDetector for skeleton, joints, the two kinds of motions and
    keyframes, and weights."""

    def __init__(self, skeleton, joints=None, min_segment_size=10, ctx=None, weights=None):
        self._keyframe_detector = KeyframeDetector(skeleton, joints, ctx, weights)
        self.min_segment_size = min_segment_size

    def segment_indices(self, motions, start_keyframe, end_keyframe, threshold=1.0, single=False):
        """The (motion index, start, end) triples of the segments, in motion order and then start order.  single: the one
        (argmin, argmin) pair of extract_single_segments per motion, else extract_segments' search."""
        if not len(motions):
            return []
        det = self._keyframe_detector
        ctx = _capi.default_context(det._ctx)
        with ctx.buffers() as bufs:
            d_dev, off = det._distances_on_device(ctx, bufs, motions, [start_keyframe, end_keyframe])
            pairs = _search_on_device(ctx, bufs, d_dev, d_dev.address + 8 * int(off[-1]), off, SINGLE if single else MULTI, threshold,
                                      self.min_segment_size)
        return [(m, int(s), int(e)) for m, p in enumerate(pairs) for s, e in p]

    def extract_single_segments(self, motions, start_keyframe, end_keyframe):
        """One slice per motion, from the frame closest to the start keyframe to the one closest to the end keyframe (empty
        when that one does not come later): views into the caller's motions."""
        return [motions[m][s:e] for m, s, e in self.segment_indices(motions, start_keyframe, end_keyframe, single=True)]

    def extract_segments(self, motions, start_keyframe, end_keyframe, threshold=1.0):
        """The flat list of slices motion[start:end], in motion order and then start order: views into the caller's
        motions."""
        return [motions[m][s:e] for m, s, e in self.segment_indices(motions, start_keyframe, end_keyframe, threshold)]
