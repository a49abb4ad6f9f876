"""HipMotionModelConstructor: the reference's MotionModelConstructor (construction/motion_model_constructor.py:113-524) with
every stage on the device -- captured clips in, the motion primitive's dict out.

    constructor = HipMotionModelConstructor(skeleton, config, joints=..., skeleton_json=...)
    constructor.set_motions(motions)                      # {key: (F_k, D) quaternion frames}
    data = constructor.construct_model("walk_leftStance", version=3)

construct_model gives the dict of the loose chain spatial_alignment.align_motions_spatially -> dtw.align_frames_temporally ->
fpca.construct_motion_primitive_model, array for array.  What the class adds is the reference's method table and the data's
residence: the captures are uploaded once, and the spatially aligned frames stay on the device through forward kinematics,
the distance grids, the paths and the warp; the warped frames go from there into mg_prepare_aligned_frames and the spline
fit.  Downloads on that leg: the warping functions and the warped frames once each (they are the reference's _temporal_data
and _aligned_frames, which callers read), then the stages' own results.  With set_dtw_sections the spatially aligned frames
come down once, because the sections are cut on the host (dtw.align_frames_temporally takes host motions).

What the reference takes from an anim_utils skeleton is an argument: `skeleton` is a _capi.Skeleton (forward kinematics and
animated_joints), `frame_time` the v3 file's tspm.frame_time, and `skeleton_json` the dict save_skeleton=True stores
(skeleton.to_json() is anim_utils'); save_skeleton=True without it raises ValueError.

Not reproduced: config["temp_data_dir"] and the BVH export behind it (_export_aligned_frames, export_sample, export_coeffs,
temporal_data.npy): file output through anim_utils' BVHWriter.  config["use_multi_processing"] has no meaning here.
"""
import collections

import numpy as np

from . import _capi, dtw, fpca, spatial_alignment

_OrderedDict = collections.OrderedDict


class _DeviceMotions(object):
    """A ragged table of motions on the device: what _align_frames_spatially hands to the temporal alignment."""

    def __init__(self, ctx, keys, buf, offsets, n_dim):
        self.ctx, self._keys, self.buf, self.offsets, self.n_dim = ctx, list(keys), buf, offsets, int(n_dim)

    def keys(self):
        return list(self._keys)

    def __len__(self):
        return len(self._keys)

    def lengths(self):
        return _OrderedDict((k, int(self.offsets[i + 1] - self.offsets[i])) for i, k in enumerate(self._keys))

    def host(self):
        table = self.ctx.download(self.buf, (int(self.offsets[-1]), self.n_dim), np.float64)
        return _OrderedDict((k, table[int(self.offsets[i]):int(self.offsets[i + 1])].copy()) for i, k in enumerate(self._keys))

    def free(self):
        if self.buf is not None:
            self.buf.free()
        self.buf = None


def _host_motions(motions):
    return motions.host() if isinstance(motions, _DeviceMotions) else motions


class HipMotionModelConstructor(object):
    def __init__(self, skeleton, config, joints=None, ctx=None, skeleton_json=None, reference_selection="average_time_line", frame_time=None,
                 gmm_trainer=None):
        """skeleton: a _capi.Skeleton; config: the reference's (n_spatial_basis_factor, n_components, fraction,
        n_basis_functions_temporal, npc_temporal, precision_temporal); joints: the joints (names or indices) whose global
        positions make a frame's point cloud, None: all; reference_selection: how the reference motion is chosen without a
        mean_key, "average_time_line" (get_average_time_line) or dtw's "least_mean_cost"; gmm_trainer: an object with fit and
        convert_model_to_json, None: HipGMMTrainer."""
        if reference_selection not in dtw.REFERENCE_SELECTIONS:
            raise ValueError("reference_selection %r (one of %r)" % (reference_selection, dtw.REFERENCE_SELECTIONS))
        self._skeleton = self.skeleton = skeleton
        self.config = config
        self.joints = list(skeleton.names) if joints is None else list(joints)
        self.ctx = ctx
        self.skeleton_json = skeleton_json
        self.reference_selection = reference_selection
        self.frame_time = frame_time
        self.gmm_trainer = gmm_trainer
        self.ref_orientation = [0, -1]  # look into -z direction in 2d
        self._input_motions = dict()
        self._dtw_sections = None
        self._keyframes = dict()
        self._temporal_data = None
        self._aligned_frames = None
        self._aligned_dev = None        # the (N, F, D) device copy of _aligned_frames, between _align_frames and the fPCA
        self._spatial_fpca_data = None
        self._temporal_fpca_data = None
        self._gmm_data = None

    # ---- the reference's setters ---------------------------------------------------------------------------------------------
    def set_motions(self, motions):
        self._input_motions = motions

    def set_dtw_sections(self, dtw_sections):
        self._dtw_sections = dtw_sections
        self._keyframes = dict()

    def set_aligned_frames(self, motions, keyframes=None):
        self._drop_device_frames()
        self._aligned_frames = motions
        if keyframes is not None:
            self._keyframes = keyframes

    def set_timewarping(self, temporal_data):
        self._temporal_data = temporal_data

    def construct_model(self, name, version=1, save_skeleton=False, mean_key=None, align_frames=True):
        if save_skeleton and self.skeleton_json is None:
            raise ValueError("save_skeleton=True needs the skeleton_json given at construction (skeleton.to_json() is anim_utils')")
        try:
            if align_frames or self._temporal_data is None or self._aligned_frames is None:
                self._align_frames(mean_key)
            self.run_dimension_reduction()
        finally:
            self._drop_device_frames()
        self.learn_statistical_model()
        return self.convert_motion_model_to_json(name, version, save_skeleton)

    # ---- alignment -----------------------------------------------------------------------------------------------------------
    def _context(self):
        return _capi.default_context(self.ctx)

    def _drop_device_frames(self):
        if self._aligned_dev is not None:
            self._aligned_dev.free()
        self._aligned_dev = None

    def _align_frames(self, mean_key=None):
        self._drop_device_frames()
        aligned_frames = self._align_frames_spatially(self._input_motions)
        try:
            if self._temporal_data is not None:
                self._aligned_frames = _host_motions(aligned_frames)
                if isinstance(aligned_frames, _DeviceMotions) and len(set(aligned_frames.lengths().values())) == 1:
                    self._aligned_dev = aligned_frames       # equally long: the table is the (N, F, D) input of the fPCA
                temp = _OrderedDict()
                for key in self._aligned_frames.keys():
                    if key in self._temporal_data:
                        temp[key] = self._temporal_data[key]
                self._temporal_data = temp
            elif self._dtw_sections is not None:
                self._aligned_frames, self._temporal_data = self._align_frames_temporally_split(aligned_frames, self._dtw_sections, mean_key=mean_key)
            else:
                self._aligned_frames, self._temporal_data = self._align_frames_temporally(aligned_frames, mean_key)
        finally:
            if isinstance(aligned_frames, _DeviceMotions) and aligned_frames is not self._aligned_dev:
                aligned_frames.free()

    def _align_frames_spatially(self, input_motions):
        """The captures' one upload; the aligned frames stay on the device (a _DeviceMotions)."""
        ctx = self._context()
        with ctx.buffers() as bufs:
            out_dev, off, n_dim, _ = spatial_alignment.upload_and_align(ctx, bufs, input_motions, 0, self.ref_orientation)
            return _DeviceMotions(ctx, input_motions.keys(), bufs.release(out_dev), off, n_dim)

    def get_average_time_line(self, input_motions):
        lengths = input_motions.lengths() if isinstance(input_motions, _DeviceMotions) else _OrderedDict((k, len(m)) for k, m in input_motions.items())
        return dtw.get_average_time_line(_OrderedDict((k, range(n)) for k, n in lengths.items()))

    def _align_frames_temporally(self, input_motions, mean_key=None):
        ctx = self._context()
        if not isinstance(input_motions, _DeviceMotions):
            return dtw.align_frames_temporally(self._skeleton, self.joints, input_motions, mean_key=mean_key, ctx=ctx,
                                               reference_selection=self.reference_selection)
        keys, lengths = input_motions.keys(), input_motions.lengths()
        if mean_key is None and self.reference_selection == "average_time_line":
            mean_key = self.get_average_time_line(input_motions)
        if mean_key is not None and mean_key not in lengths:
            raise KeyError("the reference motion %r is not among the motions" % (mean_key,))
        idx = self._skeleton.indices(self.joints)
        dtw._check_limits(1 if mean_key is None else lengths[mean_key], lengths.values(), len(idx))
        with ctx.buffers() as bufs:
            o_dev, warps, ref_index = dtw._align_section_dev(ctx, bufs, self._skeleton, idx, input_motions.buf, input_motions.offsets, input_motions.n_dim,
                                                             None if mean_key is None else keys.index(mean_key))
            fr = lengths[keys[ref_index]]
            warped = ctx.download(o_dev, (len(keys), fr, input_motions.n_dim), np.float64)
            self._aligned_dev = _DeviceMotions(ctx, keys, bufs.release(o_dev), np.arange(len(keys) + 1, dtype=np.int64) * fr, input_motions.n_dim)
        return (_OrderedDict((k, warped[m]) for m, k in enumerate(keys)), _OrderedDict((k, [int(v) for v in warps[m]]) for m, k in enumerate(keys)))

    def _align_frames_temporally_split(self, input_motions, sections=None, mean_key=None):
        motions = _host_motions(input_motions)       # the sections are cut on the host
        ctx = self._context()
        if mean_key is None:
            mean_key = self.get_average_time_line(motions) if self.reference_selection == "average_time_line" else dtw.select_reference_motion(
                self._skeleton, self.joints, motions, ctx=ctx)[0]
        if sections is not None:
            for i, s in enumerate(sections[mean_key]):     # use segment end as keyframe
                self._keyframes["contact" + str(i)] = s["end_idx"]
        return dtw.align_frames_temporally(self._skeleton, self.joints, motions, mean_key=mean_key, sections=sections, ctx=ctx)

    # ---- dimension reduction ---------------------------------------------------------------------------------------------------
    def run_dimension_reduction(self):
        self.run_spatial_dimension_reduction()
        self.run_temporal_dimension_reduction()

    def run_spatial_dimension_reduction(self):
        ctx = self._context()
        keys = list(self._aligned_frames.keys())
        n_frames = len(self._aligned_frames[keys[0]])
        n_basis = int(n_frames * self.config["n_spatial_basis_factor"])
        n_joints = len(self._skeleton.animated_joints)
        with ctx.buffers() as bufs:
            resident = self._aligned_dev is not None and self._aligned_dev.keys() == keys
            if resident:
                m_dev, n_dims = self._aligned_dev.buf, self._aligned_dev.n_dim
            else:
                table = np.ascontiguousarray([np.asarray(self._aligned_frames[k], dtype=np.float64) for k in keys])
                m_dev, n_dims = bufs.upload(table), table.shape[2]
            n = len(keys)
            if n_basis > fpca.MAX_BASIS or n_frames > fpca.MAX_FRAMES:
                raise ValueError("spline fit: n_basis = %d (at most %d), n_frames = %d (at most %d)" % (n_basis, fpca.MAX_BASIS, n_frames, fpca.MAX_FRAMES))
            operator, _ = fpca.spline_fit_operator(n_basis, n_frames)
            c_dev = bufs.malloc(8 * n * n_basis * n_dims)
            with ctx.buffers() as inputs:
                p_dev = inputs.malloc(8 * n * n_frames * n_dims)
                scale_vec = _capi.prepare_aligned_frames(ctx, m_dev, n, n_frames, n_dims, n_joints, p_dev)
                self._drop_device_frames()
                _capi.spline_fit_batch(ctx, p_dev, n, n_frames, n_dims, inputs.upload(operator), n_basis, c_dev)
            pca = fpca._DevicePCA(ctx, c_dev, n, n_basis * n_dims)      # the flat index coeff * D + d is the table's own
        try:
            fit = pca.fit
            k, npc = fpca.npc_from_singular_values(fit["singular_values"], (n, n_basis * n_dims), self.config["fraction"])
            vt = fit["vt"][:k]
            eigenvectors = vt[:npc] if self.config["n_components"] is None else vt[:self.config["n_components"]]
            pca.use(eigenvectors)
            parameters = pca.project(pca.centred_dev, n)
        finally:
            pca.close()
        result = {'parameters': parameters, 'file_order': keys, 'n_basis': n_basis, 'n_coeffs': n_basis, 'n_dim': n_dims, 'scale_vec': [1, 1, 1]}
        result['mean'], result['eigenvectors'] = fpca.scale_root_translation_in_fpca_data(fit["mean"], eigenvectors, scale_vec, n_basis, n_dims)
        self._spatial_fpca_data = result

    def run_temporal_dimension_reduction(self):
        ft = fpca.HipFPCATimeSemantic(self.config["n_basis_functions_temporal"], n_components_temporal=self.config["npc_temporal"],
                                      precision_temporal=self.config["precision_temporal"], ctx=self.ctx)
        ft.temporal_semantic_data = np.array([self._temporal_data[k] for k in self._temporal_data.keys()], dtype=np.float64)
        ft.functional_pca()
        self._temporal_fpca_data = {'eigenvectors': ft.eigenvectors, 'mean': ft.mean_vec, 'parameters': ft.lowVs, 'n_basis': ft.n_basis, 'n_dim': 1,
                                    'semantic_annotation': []}

    def learn_statistical_model(self):
        if self._temporal_fpca_data is not None:
            motion_parameters = np.concatenate((self._spatial_fpca_data["parameters"], self._temporal_fpca_data["parameters"]), axis=1)
        else:
            motion_parameters = self._spatial_fpca_data["parameters"]
        trainer = self.gmm_trainer
        if trainer is None:
            from .gmm_trainer import HipGMMTrainer
            trainer = HipGMMTrainer(ctx=self.ctx)
        trainer.fit(motion_parameters)
        self._gmm_data = trainer.convert_model_to_json()

    def convert_motion_model_to_json(self, name="", version=1, save_skeleton=False):
        if save_skeleton and self.skeleton_json is None:
            raise ValueError("save_skeleton=True needs the skeleton_json given at construction (skeleton.to_json() is anim_utils')")
        key = list(self._aligned_frames.keys())[0]
        n_frames = len(self._aligned_frames[key])
        data = fpca.model_to_json(self._spatial_fpca_data, self._temporal_fpca_data, self._gmm_data, n_frames, self.config,
                                  list(self._skeleton.animated_joints), self.frame_time, name, version, self._keyframes)
        if save_skeleton:
            data["skeleton"] = self.skeleton_json
        return data

    def back_project_sample(self, alpha):
        """MotionModel.back_project_sample: the control points (n_basis, n_dim) of the latent spatial vector alpha."""
        coeffs = np.dot(np.asarray(self._spatial_fpca_data["eigenvectors"]).T, alpha)
        coeffs += self._spatial_fpca_data["mean"]
        coeffs = coeffs.reshape((self._spatial_fpca_data["n_basis"], self._spatial_fpca_data["n_dim"]))
        translation_maxima = self._spatial_fpca_data["scale_vec"]        # undo the scaling on the translation
        coeffs[:, 0] *= translation_maxima[0]
        coeffs[:, 1] *= translation_maxima[1]
        coeffs[:, 2] *= translation_maxima[2]
        return coeffs
