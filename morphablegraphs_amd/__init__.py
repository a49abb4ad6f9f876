"""MI355X-native motion-primitive back-projection / GMM scoring behind the morphablegraphs plugin surface.
Importing the package does not load the HIP library; the first backend object does (and fails loudly
if libmg_hip.so or a gfx950 device is missing -- there is no CPU fallback)."""
from .dtw import align_frames_temporally, all_pairs_costs, reference_from_costs, select_reference_motion  # noqa: F401
from .fpca import (HipFPCASpatialData, HipFPCATimeSemantic, HipFunctionalData, HipPCAFunctionalData,  # noqa: F401
                   construct_motion_primitive_model)
from .gaussian_mixture import HipGaussianMixture, sample_like_sklearn  # noqa: F401
from .motion_primitive import HipMotionPrimitive, get_context  # noqa: F401
from .motion_primitive_wrapper import (HipMotionPrimitiveModelWrapper, HipStaticMotionPrimitive,  # noqa: F401
                                       mgrd_json_to_legacy)
from .motion_spline import HipMotionSpline  # noqa: F401
from .random_walks import RandomWalks, assemble_walks_mixed_host, choose_random_walks  # noqa: F401
from .scaled_fpca import HipScaledFunctionalPCA, sfpca_objective_func  # noqa: F401
from .segmentation import KeyframeDetector, Segmentation  # noqa: F401

__all__ = ["HipFPCASpatialData", "HipFPCATimeSemantic", "HipFunctionalData", "HipGaussianMixture", "HipMotionPrimitive",
           "HipMotionPrimitiveModelWrapper", "HipMotionSpline", "HipPCAFunctionalData", "HipScaledFunctionalPCA", "HipStaticMotionPrimitive", "KeyframeDetector",
           "RandomWalks", "Segmentation", "align_frames_temporally", "assemble_walks_mixed_host", "choose_random_walks", "construct_motion_primitive_model", "get_context", "mgrd_json_to_legacy", "sample_like_sklearn",
           "sfpca_objective_func"]
