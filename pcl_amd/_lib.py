"""ctypes binding of the C ABI in include/pclhip.h (the drop-in boundary).

The shared library is built in-tree by `__graft_entry__.build()` / `make -C pcl_amd/csrc`.  There is
deliberately NO CPU fallback: if the HIP library cannot be loaded, importing the product API fails
loudly with PclHipUnavailable.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCLHIP_LIB") or os.path.join(_HERE, "libpclhip.so")  # PCLHIP_LIB: A/B runs of two builds

NSUMS = 32
POINT_TO_POINT = 0
POINT_TO_PLANE = 1
SYMMETRIC = 2

CONVERGENCE_STATES = ("NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE",
                      "NO_CORRESPONDENCES", "FAILURE_AFTER_MAX_ITERATIONS")


class PclHipUnavailable(RuntimeError):
    pass


class PclHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("pclhip status %d: %s" % (status, message))
        self.status = status


class IcpParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("max_correspondence_distance", C.c_double),
                ("transformation_epsilon", C.c_double),
                ("transformation_rotation_epsilon", C.c_double),
                ("euclidean_fitness_epsilon", C.c_double), ("min_number_correspondences", C.c_int),
                ("mode", C.c_int), ("failure_after_max_iterations", C.c_int),
                ("max_iterations_similar_transforms", C.c_int),
                ("mse_threshold_absolute", C.c_double)]


class IcpResult(C.Structure):
    _fields_ = [("final_transformation", C.c_float * 16), ("last_transformation", C.c_float * 16),
                ("nr_iterations", C.c_int), ("converged", C.c_int), ("convergence_state", C.c_int),
                ("num_correspondences", C.c_uint64), ("mse", C.c_double), ("gpu_ms", C.c_double),
                ("gpu_ms_search_kernel", C.c_double)]


class IcpStep(C.Structure):
    _fields_ = [("iteration", C.c_int), ("convergence_state", C.c_int), ("converged", C.c_int),
                ("alignment_ended", C.c_int), ("num_correspondences", C.c_uint64), ("mse", C.c_double),
                ("search_ms", C.c_float), ("kernels_ms", C.c_float), ("step_ms", C.c_float),
                ("final_transformation", C.c_float * 16)]


class GicpParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("transformation_epsilon", C.c_double), ("rotation_epsilon", C.c_double),
                ("max_correspondence_distance", C.c_double), ("min_number_correspondences", C.c_int),
                ("k_correspondences", C.c_int), ("gicp_epsilon", C.c_double), ("max_inner_iterations", C.c_int),
                ("translation_gradient_tolerance", C.c_double), ("rotation_gradient_tolerance", C.c_double)]


class GicpResult(C.Structure):
    _fields_ = [("final_transformation", C.c_float * 16), ("last_transformation", C.c_float * 16),
                ("nr_iterations", C.c_int), ("converged", C.c_int), ("num_correspondences", C.c_uint64),
                ("newton_iterations", C.c_int), ("newton_steps", C.c_int), ("newton_steps_alpha_one", C.c_int),
                ("eval_passes", C.c_int), ("trace_count", C.c_int), ("reserved", C.c_int),
                ("covariance_ms", C.c_double), ("search_ms", C.c_double), ("pack_ms", C.c_double),
                ("eval_ms", C.c_double), ("total_ms", C.c_double)]


class GicpTrace(C.Structure):
    _fields_ = [("correspondences", C.c_uint64), ("inner_iterations", C.c_int), ("reserved", C.c_int),
                ("f", C.c_double), ("transformation", C.c_float * 16)]


class NdtParams(C.Structure):
    _fields_ = [("resolution", C.c_float), ("max_iterations", C.c_int), ("step_size", C.c_double),
                ("outlier_ratio", C.c_double), ("transformation_epsilon", C.c_double),
                ("transformation_rotation_epsilon", C.c_double), ("min_covar_eigvalue_mult", C.c_double),
                ("min_points_per_voxel", C.c_int), ("neighborhood_search_method", C.c_int)]


class NdtResult(C.Structure):
    _fields_ = [("final_transformation", C.c_float * 16), ("last_transformation", C.c_float * 16),
                ("nr_iterations", C.c_int), ("converged", C.c_int), ("score", C.c_double),
                ("transformation_likelihood", C.c_double), ("num_cells", C.c_uint64), ("num_pairs", C.c_uint64),
                ("evaluations_full", C.c_int), ("evaluations_gradient", C.c_int), ("evaluations_hessian", C.c_int),
                ("trace_count", C.c_int), ("cells_ms", C.c_double), ("eval_ms_full", C.c_double),
                ("eval_ms_gradient", C.c_double), ("eval_ms_hessian", C.c_double), ("total_ms", C.c_double)]


class NdtTrace(C.Structure):
    _fields_ = [("step_length", C.c_double), ("line_search_trials", C.c_int), ("reserved", C.c_int),
                ("score", C.c_double), ("transformation", C.c_float * 16)]


class ScpParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("nr_samples", C.c_int), ("k_correspondences", C.c_int),
                ("similarity_threshold", C.c_float), ("inlier_fraction", C.c_float),
                ("max_correspondence_distance", C.c_double), ("seed", C.c_uint64), ("batch_size", C.c_int)]


class ScpResult(C.Structure):
    _fields_ = [("final_transformation", C.c_float * 16), ("converged", C.c_int), ("iterations", C.c_int),
                ("rejected", C.c_int), ("best_iteration", C.c_int), ("best_error", C.c_float), ("best_count", C.c_uint32),
                ("trace_count", C.c_int), ("knn_rows", C.c_uint32), ("knn_ms", C.c_double), ("hypothesis_ms", C.c_double),
                ("fitness_ms", C.c_double), ("total_ms", C.c_double)]


class ScpTrace(C.Structure):
    _fields_ = [("iteration", C.c_int), ("rejected", C.c_int), ("samples", C.c_int * 8), ("matches", C.c_int * 8),
                ("transformation", C.c_float * 16), ("inliers", C.c_uint32), ("error", C.c_float)]


class SacPlaneParams(C.Structure):
    _fields_ = [("distance_threshold", C.c_double), ("max_iterations", C.c_int), ("probability", C.c_double),
                ("optimize_coefficients", C.c_int), ("seed", C.c_uint64), ("batch_size", C.c_int)]


class SacPlaneStats(C.Structure):
    _fields_ = [("trials", C.c_uint64), ("iterations", C.c_int), ("skipped", C.c_uint32), ("batches", C.c_int),
                ("best_trial", C.c_int), ("best_count", C.c_uint32), ("refined", C.c_int), ("count_ms", C.c_double),
                ("total_ms", C.c_double)]


class SacPlaneTrace(C.Structure):
    _fields_ = [("samples", C.c_int * 3), ("skipped", C.c_int), ("coefficients", C.c_float * 4), ("count", C.c_uint32)]


class SacModelParams(C.Structure):
    _fields_ = [("model_type", C.c_int), ("axis", C.c_float * 3), ("eps_angle", C.c_double),
                ("normal_distance_weight", C.c_double), ("distance_from_origin", C.c_double), ("eps_dist", C.c_double)]


class SacModelTrace(C.Structure):
    _fields_ = [("samples", C.c_int * 3), ("skipped", C.c_int), ("coefficients", C.c_float * 4), ("count", C.c_uint32),
                ("valid", C.c_int)]


class SacCylinderParams(C.Structure):
    _fields_ = [("normal_distance_weight", C.c_double), ("radius_min", C.c_double), ("radius_max", C.c_double),
                ("axis", C.c_float * 3), ("eps_angle", C.c_double)]


class SacCylinderTrace(C.Structure):
    _fields_ = [("samples", C.c_int * 2), ("skipped", C.c_int), ("coefficients", C.c_float * 7), ("count", C.c_uint32),
                ("valid", C.c_int)]


class RejectorSacParams(C.Structure):
    _fields_ = [("inlier_threshold", C.c_double), ("max_iterations", C.c_int), ("probability", C.c_double),
                ("seed", C.c_uint64), ("batch_size", C.c_int), ("refine", C.c_int)]


class RejectorSacStats(C.Structure):
    _fields_ = [("trials", C.c_uint64), ("iterations", C.c_int), ("best_trial", C.c_int), ("best_count", C.c_uint32),
                ("remaining", C.c_uint32), ("has_model", C.c_int), ("no_sample", C.c_int), ("n", C.c_uint32),
                ("reserved", C.c_uint32), ("sample_dist_thresh", C.c_double)]


class RejectorSacTrace(C.Structure):
    _fields_ = [("samples", C.c_int * 3), ("attempts", C.c_int), ("no_sample", C.c_int), ("transformation", C.c_float * 16),
                ("count", C.c_uint32)]


SACMODEL_PLANE = 0   # sample_consensus/model_types.h:47
SACMODEL_PERPENDICULAR_PLANE = 9
SACMODEL_NORMAL_PLANE = 11
SACMODEL_PARALLEL_PLANE = 15
SACMODEL_NORMAL_PARALLEL_PLANE = 16
SAC_RANSAC = 0       # sample_consensus/method_types.h:45

NDT_RADIUS, NDT_DIRECT27, NDT_DIRECT26, NDT_DIRECT7, NDT_DIRECT1 = 0, 1, 2, 3, 4


class ConvergenceState(C.Structure):
    _fields_ = [("prev_mse", C.c_double), ("iterations_similar_transforms", C.c_int), ("convergence_state", C.c_int)]


class VoxelGridDims(C.Structure):
    _fields_ = [("min_b", C.c_int32 * 3), ("max_b", C.c_int32 * 3), ("div_b", C.c_int32 * 3), ("divb_mul", C.c_int32 * 3)]


class SorStats(C.Structure):
    _fields_ = [("mean", C.c_double), ("stddev", C.c_double), ("threshold", C.c_double), ("sum", C.c_double),
                ("sq_sum", C.c_double), ("valid", C.c_uint64)]


class RegionGrowingParams(C.Structure):
    _fields_ = [("number_of_neighbours", C.c_int), ("smoothness_threshold", C.c_float), ("curvature_threshold", C.c_float),
                ("curvature_test", C.c_int), ("smooth_mode", C.c_int), ("residual_test", C.c_int),
                ("residual_threshold", C.c_float), ("min_cluster_size", C.c_uint32), ("max_cluster_size", C.c_uint32)]


COMM_ID_BYTES = 128


class Rejector(C.Structure):
    _fields_ = [("kind", C.c_int), ("param", C.c_double), ("min_correspondences", C.c_uint32),
                ("reserved", C.c_uint32)]


class PcdInfo(C.Structure):
    _fields_ = [("points", C.c_uint64), ("width", C.c_uint32), ("height", C.c_uint32), ("data_type", C.c_int),
                ("version", C.c_int), ("point_step", C.c_uint32), ("num_fields", C.c_uint32),
                ("has_xyz", C.c_int), ("has_normals", C.c_int), ("has_curvature", C.c_int),
                ("has_intensity", C.c_int), ("has_rgb", C.c_int), ("viewpoint", C.c_float * 7),
                ("data_offset", C.c_uint64)]


PCD_ASCII, PCD_BINARY, PCD_BINARY_COMPRESSED = 0, 1, 2

REJ_DISTANCE, REJ_MEDIAN_DISTANCE, REJ_ONE_TO_ONE, REJ_TRIMMED, REJ_SAMPLE_CONSENSUS = 0, 1, 2, 3, 4

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)

# every symbol include/pclhip.h declares: (restype, argtypes)
_vp, _sz, _u64 = C.c_void_p, C.c_size_t, C.c_uint64
SIGNATURES = {
    "pclhip_version": (C.c_char_p, []),
    "pclhip_last_error": (C.c_char_p, [_vp]),
    "pclhip_ctx_create": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "pclhip_ctx_create_on_stream": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "pclhip_ctx_stream": (_vp, [_vp]),
    "pclhip_ctx_destroy": (None, [_vp]),
    "pclhip_ctx_synchronize": (C.c_int, [_vp]),
    "pclhip_ctx_reserve": (C.c_int, [_vp, C.c_uint64]),
    "pclhip_ctx_set_option": (C.c_int, [_vp, C.c_char_p, C.c_double]),
    "pclhip_ctx_stats": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64)]),
    "pclhip_index_build": (C.c_int, [_vp, _vp, _sz, _u64, _vp, _u64, C.POINTER(_vp)]),
    "pclhip_index_build_scaled": (C.c_int, [_vp, _vp, _sz, _u64, _vp, _u64, C.POINTER(C.c_float), C.POINTER(_vp)]),
    "pclhip_index_build_ex": (C.c_int, [_vp, _vp, _sz, _u64, _vp, _u64, C.POINTER(C.c_float), _sz, C.POINTER(_vp)]),
    "pclhip_icp_transform_source": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int, _vp, _vp, _sz, _u64, _sz]),
    "pclhip_index_destroy": (None, [_vp]),
    "pclhip_index_size": (_u64, [_vp]),
    "pclhip_index_build_ms": (C.c_double, [_vp]),
    "pclhip_index_order": (C.c_int, [_vp, _vp]),
    "pclhip_index_cells": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "pclhip_knn": (C.c_int, [_vp, _vp, _sz, _u64, C.c_int, _vp, _vp]),
    "pclhip_radius_search": (C.c_int, [_vp, _vp, _sz, _u64, C.c_double, C.c_uint32, C.POINTER(_u64), _vp, _vp, _u64,
                                       C.POINTER(_u64)]),
    "pclhip_normals": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_float), _vp, _sz, C.POINTER(_u64)]),
    "pclhip_normals_records": (C.c_int, [_vp, C.c_int, C.c_double, C.POINTER(C.c_float), _vp, _sz, _sz, _sz, C.POINTER(_u64)]),
    "pclhip_normals_radius": (C.c_int, [_vp, C.c_double, C.POINTER(C.c_float), _vp, _sz, C.POINTER(_u64)]),
    "pclhip_normals_at": (C.c_int, [_vp, _vp, _sz, _u64, _vp, _u64, C.c_int, C.c_double, C.POINTER(C.c_float), _vp, _sz,
                                    C.POINTER(_u64)]),
    "pclhip_gicp_covariances": (C.c_int, [_vp, C.c_int, C.c_double, _vp]),
    "pclhip_index_set_normals": (C.c_int, [_vp, _vp, _sz]),
    "pclhip_gicp_params_default": (None, [C.POINTER(GicpParams)]),
    "pclhip_gicp_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "pclhip_gicp_destroy": (None, [_vp]),
    "pclhip_gicp_set_source": (C.c_int, [_vp, _vp, _sz, _u64]),
    "pclhip_gicp_set_source_covariances": (C.c_int, [_vp, _vp, _u64]),
    "pclhip_gicp_set_target_covariances": (C.c_int, [_vp, _vp, _u64]),
    "pclhip_gicp_set_trace": (C.c_int, [_vp, C.POINTER(GicpTrace), C.c_int]),
    "pclhip_gicp_align": (C.c_int, [_vp, C.POINTER(GicpParams), C.POINTER(C.c_float), C.POINTER(GicpResult)]),
    "pclhip_gicp_evaluate": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double)]),
    "pclhip_gicp_mahalanobis": (C.c_int, [_vp, _vp]),
    "pclhip_gicp_fitness_score": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_double, C.POINTER(C.c_double),
                                            C.POINTER(_u64)]),
    "pclhip_ndt_params_default": (None, [C.POINTER(NdtParams)]),
    "pclhip_ndt_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "pclhip_ndt_destroy": (None, [_vp]),
    "pclhip_ndt_set_target": (C.c_int, [_vp, _vp, _sz, _u64]),
    "pclhip_ndt_set_source": (C.c_int, [_vp, _vp, _sz, _u64]),
    "pclhip_ndt_set_trace": (C.c_int, [_vp, C.POINTER(NdtTrace), C.c_int]),
    "pclhip_ndt_align": (C.c_int, [_vp, C.POINTER(NdtParams), C.POINTER(C.c_float), C.POINTER(NdtResult)]),
    "pclhip_ndt_evaluate": (C.c_int, [_vp, C.POINTER(NdtParams), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_u64)]),
    "pclhip_ndt_cells": (C.c_int, [_vp, C.POINTER(NdtParams), C.POINTER(_u64), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64]),
    "pclhip_ndt_fitness_score": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_double, C.POINTER(C.c_double),
                                           C.POINTER(_u64)]),
    "pclhip_feature_knn": (C.c_int, [_vp, _vp, _sz, _u64, _vp, _sz, _u64, C.c_int, C.c_int, _vp, _vp, _vp]),
    "pclhip_scp_params_default": (None, [C.POINTER(ScpParams)]),
    "pclhip_scp_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "pclhip_scp_destroy": (None, [_vp]),
    "pclhip_scp_set_source": (C.c_int, [_vp, _vp, _sz, _u64]),
    "pclhip_scp_set_source_features": (C.c_int, [_vp, _vp, _sz, _u64, C.c_int]),
    "pclhip_scp_set_target_features": (C.c_int, [_vp, _vp, _sz, _u64, C.c_int]),
    "pclhip_scp_set_trace": (C.c_int, [_vp, C.POINTER(ScpTrace), C.c_int]),
    "pclhip_scp_evaluate": (C.c_int, [_vp, C.POINTER(ScpParams), C.POINTER(C.c_float), C.c_int, _vp, _vp]),
    "pclhip_scp_align": (C.c_int, [_vp, C.POINTER(ScpParams), C.POINTER(C.c_float), C.POINTER(ScpResult)]),
    "pclhip_scp_inliers": (C.c_int, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "pclhip_scp_fitness_score": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_double, C.POINTER(C.c_double),
                                           C.POINTER(_u64)]),
    "pclhip_scp_last_ms": (None, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pclhip_sac_plane_params_default": (None, [C.POINTER(SacPlaneParams)]),
    "pclhip_sac_segment_plane": (C.c_int, [_vp, _vp, _u64, _sz, _vp, _u64, C.POINTER(SacPlaneParams), C.POINTER(C.c_float),
                                           _vp, _u64, C.POINTER(_u64), _vp, _u64, C.POINTER(_u64),
                                           C.POINTER(SacPlaneStats)]),
    "pclhip_sac_plane_evaluate": (C.c_int, [_vp, _vp, _u64, _sz, _vp, _u64, C.c_double, C.POINTER(C.c_float), C.c_int, _vp]),
    "pclhip_sac_last_trace": (C.c_int, [_vp, C.POINTER(SacPlaneTrace), _u64, C.POINTER(_u64)]),
    "pclhip_sac_model_params_default": (None, [C.POINTER(SacModelParams)]),
    "pclhip_sac_segment_model": (C.c_int, [_vp, _vp, _u64, _sz, _vp, _sz, _vp, _u64, C.POINTER(SacPlaneParams),
                                           C.POINTER(SacModelParams), C.POINTER(C.c_float), _vp, _u64, C.POINTER(_u64), _vp,
                                           _u64, C.POINTER(_u64), C.POINTER(SacPlaneStats)]),
    "pclhip_sac_model_evaluate": (C.c_int, [_vp, _vp, _u64, _sz, _vp, _sz, _vp, _u64, C.c_double, C.POINTER(SacModelParams),
                                            C.POINTER(C.c_float), C.c_int, _vp, _vp]),
    "pclhip_sac_last_model_trace": (C.c_int, [_vp, C.POINTER(SacModelTrace), _u64, C.POINTER(_u64)]),
    "pclhip_sac_cylinder_params_default": (None, [C.POINTER(SacCylinderParams)]),
    "pclhip_sac_cylinder_segment": (C.c_int, [_vp, _vp, _u64, _sz, _vp, _sz, _vp, _u64, C.POINTER(SacPlaneParams),
                                              C.POINTER(SacCylinderParams), C.POINTER(C.c_float), _vp, _u64, C.POINTER(_u64),
                                              _vp, _u64, C.POINTER(_u64), C.POINTER(SacPlaneStats)]),
    "pclhip_sac_cylinder_model": (C.c_int, [_vp, _vp, _u64, _sz, _vp, _sz, C.POINTER(C.c_int32), C.POINTER(SacCylinderParams),
                                            C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "pclhip_sac_cylinder_evaluate": (C.c_int, [_vp, _vp, _u64, _sz, _vp, _sz, _vp, _u64, C.c_double,
                                               C.POINTER(SacCylinderParams), C.POINTER(C.c_float), C.c_int, _vp, _vp]),
    "pclhip_sac_cylinder_select": (C.c_int, [_vp, _vp, _u64, _sz, _vp, _sz, _vp, _u64, C.c_double,
                                             C.POINTER(SacCylinderParams), C.POINTER(C.c_float), _vp, _u64, C.POINTER(_u64)]),
    "pclhip_sac_cylinder_distances": (C.c_int, [_vp, _vp, _u64, _sz, _vp, _sz, _vp, _u64, C.POINTER(SacCylinderParams),
                                                C.POINTER(C.c_float), _vp, _u64, C.POINTER(_u64)]),
    "pclhip_sac_cylinder_optimize": (C.c_int, [_vp, _vp, _u64, _sz, _vp, _u64, C.POINTER(SacCylinderParams),
                                               C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int),
                                               C.POINTER(C.c_int)]),
    "pclhip_sac_last_cylinder_trace": (C.c_int, [_vp, C.POINTER(SacCylinderTrace), _u64, C.POINTER(_u64)]),
    "pclhip_icp_params_default": (None, [C.POINTER(IcpParams)]),
    "pclhip_icp_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "pclhip_icp_destroy": (None, [_vp]),
    "pclhip_icp_set_source": (C.c_int, [_vp, _vp, _sz, _u64]),
    "pclhip_icp_set_source_indexed": (C.c_int, [_vp, _vp, _sz, _u64, _vp, _u64]),
    "pclhip_icp_set_source_normals": (C.c_int, [_vp, _vp, _sz]),
    "pclhip_icp_set_enforce_same_direction_normals": (C.c_int, [_vp, C.c_int]),
    "pclhip_icp_set_allreduce": (C.c_int, [_vp, ALLREDUCE_FN, _vp]),
    "pclhip_icp_reset": (C.c_int, [_vp]),
    "pclhip_icp_set_rejectors": (C.c_int, [_vp, C.POINTER(Rejector), C.c_int]),
    "pclhip_icp_last_median_distance": (C.c_double, [_vp]),
    "pclhip_icp_set_reciprocal": (C.c_int, [_vp, C.c_int]),
    "pclhip_rejector_sac_params_default": (None, [C.POINTER(RejectorSacParams)]),
    "pclhip_correspondence_rejector_sample_consensus": (C.c_int, [_vp, _vp, _u64, _sz, _vp, _u64, _sz, _vp, _vp, _u64,
                                                                  C.POINTER(RejectorSacParams), _vp, _u64, C.POINTER(_u64),
                                                                  C.POINTER(C.c_float), C.POINTER(RejectorSacStats)]),
    "pclhip_rejector_sac_evaluate": (C.c_int, [_vp, _vp, _u64, _sz, _vp, _u64, _sz, _vp, _vp, _u64, C.c_double,
                                               C.POINTER(C.c_float), C.c_int, _vp]),
    "pclhip_rejector_sac_last_trace": (C.c_int, [_vp, C.POINTER(RejectorSacTrace), _u64, C.POINTER(_u64)]),
    "pclhip_icp_last_sac_transformation": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "pclhip_icp_last_sac_stats": (C.c_int, [_vp, C.POINTER(RejectorSacStats)]),
    "pclhip_icp_iterate": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_double, C.c_int,
                                     C.POINTER(C.c_double)]),
    "pclhip_icp_last_kernel_ms": (C.c_double, [_vp]),
    "pclhip_icp_last_search_ms": (C.c_double, [_vp]),
    "pclhip_icp_source_order_ms": (C.c_double, [_vp]),
    "pclhip_index_last_kernel_ms": (C.c_double, [_vp]),
    "pclhip_statistical_outlier_removal": (C.c_int, [_vp, _vp, _u64, C.c_int, C.c_double, C.c_int, _vp,
                                                     C.POINTER(_u64), _vp, C.POINTER(_u64), _vp, C.POINTER(SorStats)]),
    "pclhip_radius_outlier_removal": (C.c_int, [_vp, _vp, _u64, C.c_double, C.c_int, C.c_int, C.c_int, _vp,
                                                C.POINTER(_u64), _vp, C.POINTER(_u64)]),
    "pclhip_fpfh": (C.c_int, [_vp, _vp, _u64, C.c_double, _vp, _sz, C.POINTER(C.c_float), C.POINTER(_u64)]),
    "pclhip_index_last_fpfh_ms": (None, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pclhip_iss_keypoints": (C.c_int, [_vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, _vp, _u64,
                                       C.POINTER(_u64), _vp, _vp]),
    "pclhip_index_last_iss_ms": (None, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pclhip_mls_process": (C.c_int, [_vp, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _u64, C.POINTER(_u64),
                                     _vp]),
    "pclhip_index_last_mls_ms": (None, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pclhip_boundary": (C.c_int, [_vp, _vp, _u64, C.c_double, C.c_int, C.c_double, C.c_int, _vp, C.POINTER(_u64)]),
    "pclhip_index_last_boundary_ms": (None, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pclhip_index_last_boundary_resolved": (_u64, [_vp]),
    "pclhip_euclidean_clusters": (C.c_int, [_vp, C.c_double, C.c_uint32, C.c_uint32, _vp, C.POINTER(_u64), _u64, _vp, _u64,
                                            C.POINTER(_u64), C.POINTER(_u64)]),
    "pclhip_index_last_cluster_stats": (None, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_u64)]),
    "pclhip_region_growing_params_default": (None, [C.POINTER(RegionGrowingParams)]),
    "pclhip_region_growing": (C.c_int, [_vp, _vp, _sz, C.POINTER(RegionGrowingParams), _vp, C.POINTER(_u64), _u64, _vp, _u64,
                                        C.POINTER(_u64), C.POINTER(_u64)]),
    "pclhip_index_last_region_growing_stats": (None, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                      C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                      C.POINTER(_u64), C.POINTER(_u64)]),
    "pclhip_solve_transformation": (C.c_int, [C.POINTER(C.c_double), C.c_int,
                                              C.POINTER(C.c_float)]),
    "pclhip_icp_align": (C.c_int, [_vp, C.POINTER(IcpParams), C.POINTER(C.c_float),
                                   C.POINTER(IcpResult)]),
    "pclhip_convergence_init": (None, [C.POINTER(ConvergenceState)]),
    "pclhip_convergence_has_converged": (C.c_int, [C.POINTER(IcpParams), C.POINTER(ConvergenceState), C.c_int,
                                                   C.POINTER(C.c_float), C.c_double]),
    "pclhip_icp_run_steps": (C.c_int, [_vp, C.POINTER(IcpParams), C.POINTER(C.c_float), C.c_int, C.POINTER(IcpStep)]),
    "pclhip_comm_get_unique_id": (C.c_int, [C.POINTER(C.c_ubyte)]),
    "pclhip_comm_create": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(_vp)]),
    "pclhip_comm_destroy": (None, [_vp]),
    "pclhip_comm_rank": (C.c_int, [_vp]),
    "pclhip_comm_size": (C.c_int, [_vp]),
    "pclhip_comm_allreduce_sum_f64": (C.c_int, [_vp, _vp, C.c_int]),
    "pclhip_icp_set_comm": (C.c_int, [_vp, _vp]),
    "pclhip_partition_slabs": (C.c_int, [_vp, _sz, _u64, C.c_int, C.POINTER(C.c_float)]),
    "pclhip_select_region": (C.c_int, [_vp, _sz, _u64, C.POINTER(C.c_float), C.c_double, _vp, _u64, C.POINTER(_u64)]),
    "pclhip_region_owner": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float)]),
    "pclhip_icp_set_region": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "pclhip_index_kth_distance_max": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_double)]),
    "pclhip_icp_fitness_score": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_double, C.POINTER(C.c_double),
                                           C.POINTER(_u64)]),
    "pclhip_icp_fetch_correspondence_records": (C.c_int, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "pclhip_icp_fetch_correspondences": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    "pclhip_estimate_rigid_transformation": (C.c_int, [_vp, C.c_int, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _u64,
                                                       C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_double)]),
    "pclhip_estimate_rigid_transformation_weighted": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _u64,
                                                                C.POINTER(C.c_float), C.POINTER(C.c_double)]),
    "pclhip_transform_cloud": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int, _vp, _vp, _sz, _u64,
                                         _sz]),
    "pclhip_pcd_read_header": (C.c_int, [C.c_char_p, C.POINTER(PcdInfo)]),
    "pclhip_pcd_read": (C.c_int, [C.c_char_p, _vp, _sz, _sz, _u64, C.POINTER(_u64), C.POINTER(C.c_int)]),
    "pclhip_pcd_write": (C.c_int, [C.c_char_p, _vp, _sz, _sz, _u64, C.c_int, C.c_int]),
    "pclhip_pcd_write_organized": (C.c_int, [C.c_char_p, _vp, _sz, _sz, C.c_uint32, C.c_uint32, C.POINTER(C.c_float),
                                             C.c_int, C.c_int]),
    "pclhip_pcd_read_field": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint32, _vp, _u64, C.POINTER(_u64)]),
    "pclhip_voxelgrid_ex": (C.c_int, [_vp, _vp, _sz, _u64, C.POINTER(C.c_float), C.c_uint32, C.c_int, C.c_double,
                                      C.c_double, C.c_int, _sz, _vp, _sz, C.POINTER(_u64)]),
    "pclhip_voxelgrid_ex2": (C.c_int, [_vp, _vp, _sz, _u64, C.POINTER(C.c_float), C.c_uint32, C.c_int, C.c_double,
                                       C.c_double, C.c_int, _sz, _vp, _sz, C.POINTER(_u64), _vp, _u64,
                                       C.POINTER(VoxelGridDims)]),
    "pclhip_voxelgrid_grid": (C.c_int, [_vp, _vp, _sz, _u64, C.POINTER(C.c_float), C.c_int, C.c_double, C.c_double,
                                        C.POINTER(VoxelGridDims)]),
    "pclhip_voxelgrid": (C.c_int, [_vp, _vp, _sz, _u64, C.POINTER(C.c_float), C.c_uint32, C.c_int,
                                   C.c_double, C.c_double, _vp, C.POINTER(_u64)]),
}

_lib = None


def load():
    """dlopen libpclhip.so and bind every declared symbol (no compute, works without a GPU)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PclHipUnavailable(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C pcl_amd/csrc`).  There is no CPU fallback." % LIB_PATH)
    try:
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # missing libamdhip64 etc.
        raise PclHipUnavailable("cannot load %s: %s" % (LIB_PATH, e)) from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    # tests/wavesim builds the same sources for the host (a lane-accurate emulation of the wavefront, used by the CPU test
    # tier to check kernels against the oracle).  It is test infrastructure: the product never runs on it.
    if b"wavesim" in (lib.pclhip_version() or b"") and os.environ.get("PCLHIP_ALLOW_WAVESIM") != "1":
        raise PclHipUnavailable("%s is the CPU emulation of the test tier (tests/wavesim), not the HIP library; only "
                                "tests/test_wavesim.py loads it (PCLHIP_ALLOW_WAVESIM=1).  There is no CPU fallback." % LIB_PATH)
    _lib = lib
    return lib


def check(status, ctx_handle=None):
    if status != 0:
        msg = load().pclhip_last_error(ctx_handle)
        raise PclHipError(status, msg.decode() if msg else "")
