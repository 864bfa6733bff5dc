"""Python host-side mirror of nano_gicp::NanoGICP<PointXYZI,PointXYZI> on top of the C ABI.

Same public method names, argument meaning and failure behaviour as the reference class
(/root/reference/include/nano_gicp/nano_gicp.hpp:79-125, lsq_registration.hpp:75-89 and the
pcl::Registration setters DLO uses, /root/reference/src/dlo/odom.cc:100-120), so parity tests read
like tests of the reference.  All compute goes through libngicp_hip.so (hand-written HIP, gfx950);
there is NO CPU fallback: a missing library or GPU raises.

Clouds are numpy float32 arrays of shape (N, C), C >= 3 (C = 8 is the 32-byte pcl::PointXYZI layout);
4x4 matrices are numpy row-major on this side and converted to Eigen's column-major at the boundary;
covariances are (N, 4, 4) float64 like std::vector<Eigen::Matrix4d>.
"""
from __future__ import annotations

import ctypes as C
import enum
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("NGICP_LIB") or os.path.join(_HERE, "libngicp_hip.so")  # NGICP_LIB: another build of the same HIP library (tuning experiments)

c_f32p = C.POINTER(C.c_float)
c_f64p = C.POINTER(C.c_double)
c_i32p = C.POINTER(C.c_int)

FLT_MAX = float(np.finfo(np.float32).max)


class RegularizationMethod(enum.IntEnum):  # gicp/gicp_settings.hpp:47
    NONE = 0
    MIN_EIG = 1
    NORMALIZED_MIN_EIG = 2
    PLANE = 3
    FROBENIUS = 4


class LSQ_OPTIMIZER_TYPE(enum.IntEnum):  # lsq_registration.hpp:54
    GaussNewton = 0
    LevenbergMarquardt = 1


class NeighborSearchMethod(enum.IntEnum):  # voxelized GICP: voxels a source point is matched against (include/ngicp.h NGICP_VOX_*)
    DIRECT1 = 1
    DIRECT7 = 7
    DIRECT27 = 27


class RobustKernel(enum.IntEnum):  # robust kernel on every term (include/ngicp.h NGICP_ROBUST_*)
    NONE = 0
    HUBER = 1
    CAUCHY = 2
    GEMAN_MCCLURE = 3


class NgicpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ngicp error {code}: {msg}")
        self.code = code


class Stats(C.Structure):
    _fields_ = [("align_ms", C.c_double), ("loop_ms", C.c_double), ("pass_ms_total", C.c_double), ("passes", C.c_int),
                ("outer_iterations", C.c_int), ("lm_trials", C.c_int), ("mean_candidates", C.c_double), ("valid_fraction", C.c_double),
                ("index_build_ms", C.c_double), ("covariance_ms", C.c_double), ("upload_ms", C.c_double), ("voxel_size", C.c_double),
                ("grid_dims", C.c_int * 3), ("lanes_per_query", C.c_int), ("passes_timed", C.c_int), ("n_src", C.c_longlong), ("n_tgt", C.c_longlong), ("staged_fraction", C.c_double), ("submap_ms", C.c_double),
                ("device_allocs", C.c_longlong), ("host_wait_spins", C.c_longlong), ("query_ms", C.c_double),
                ("voxelmap_ms", C.c_double), ("search_passes", C.c_int)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["grid_dims"] = list(self.grid_dims)
        return d


# every symbol include/ngicp.h declares (tests check the library exports them all)
EXPORTS = [
    "ngicp_create", "ngicp_destroy", "ngicp_last_error", "ngicp_version", "ngicp_set_params", "ngicp_set_tuning",
    "ngicp_set_source", "ngicp_register_source", "ngicp_set_target", "ngicp_clear_source", "ngicp_clear_target",
    "ngicp_share_source_index", "ngicp_swap_source_target", "ngicp_compute_source_covs", "ngicp_compute_target_covs",
    "ngicp_copy_source_covs", "ngicp_clear_source_covs", "ngicp_clear_target_covs", "ngicp_source_covs_size",
    "ngicp_target_covs_size", "ngicp_get_source_covs", "ngicp_get_target_covs", "ngicp_set_source_covs",
    "ngicp_set_target_covs", "ngicp_align", "ngicp_linearize", "ngicp_compute_error", "ngicp_get_correspondences",
    "ngicp_target_knn", "ngicp_get_lm_trace", "ngicp_get_stats", "ngicp_set_profiling", "ngicp_sharded_begin",
    "ngicp_sharded_pass", "ngicp_sharded_step", "ngicp_sharded_finish",
    "ngicp_keyframe_add", "ngicp_keyframe_add_transformed", "ngicp_keyframe_add_transformed_filtered", "ngicp_keyframe_count", "ngicp_keyframe_size", "ngicp_keyframe_clear",
    "ngicp_submap_set", "ngicp_get_target_points", "ngicp_transform_source", "ngicp_transform_cloud", "ngicp_measure_copy_bandwidth",
    "ngicp_preprocess_scan", "ngicp_set_source_preprocessed", "ngicp_map_add", "ngicp_map_voxel_filter", "ngicp_map_size", "ngicp_map_get",
    "ngicp_map_clear", "ngicp_math_selftest", "ngicp_step_selftest", "ngicp_set_host_wait", "ngicp_covs_shard_begin", "ngicp_covs_shard_compute", "ngicp_covs_shard_commit",
    "ngicp_knn_search", "ngicp_radius_search", "ngicp_radius_fetch", "ngicp_fitness_score",
    "ngicp_align_batch", "ngicp_batch_get_lm_trace", "ngicp_fitness_score_batch",
    "ngicp_range_select", "ngicp_range_median",
    "ngicp_set_voxel_resolution", "ngicp_voxelmap_size", "ngicp_voxelmap_get",
    "ngicp_set_voxel_neighbors", "ngicp_get_voxel_neighbors", "ngicp_voxel_correspondences", "ngicp_voxelmap_builds",
    "ngicp_voxel_align_batch",
    "ngicp_set_voxel_submap_merge", "ngicp_get_voxel_submap_merge", "ngicp_voxelmap_merge_stats", "ngicp_keyframe_voxelmap_get",
    "ngicp_set_voxel_rolling", "ngicp_get_voxel_rolling", "ngicp_voxel_rolling_insert", "ngicp_voxel_rolling_evict", "ngicp_voxel_rolling_clear",
    "ngicp_voxel_rolling_get", "ngicp_voxel_rolling_stats",
    "ngicp_voxel_rolling_set", "ngicp_voxel_rolling_insert_voxels", "ngicp_voxel_rolling_insert_map", "ngicp_voxel_rolling_transform",
    "ngicp_voxel_rolling_ray_clear", "ngicp_voxel_rolling_ray_counts",
    "ngicp_voxel_rolling_insert_gated", "ngicp_voxel_rolling_insert_classes",
    "ngicp_set_robust_kernel", "ngicp_get_robust_kernel", "ngicp_robust_terms",
    "ngicp_set_pose_prior", "ngicp_get_pose_prior", "ngicp_pose_prior_terms",
    "ngicp_deskew_cloud", "ngicp_preprocess_scan_deskewed",
    "ngicp_voxel_fitness", "ngicp_voxel_fitness_batch", "ngicp_voxel_fitness_points", "ngicp_voxel_fitness_kernel_ms",
    "ngicp_scan_context_set_params", "ngicp_scan_context_get_params", "ngicp_scan_context_tables", "ngicp_scan_context_compute",
    "ngicp_scan_context_add", "ngicp_scan_context_add_descriptor", "ngicp_scan_context_count", "ngicp_scan_context_get", "ngicp_scan_context_clear",
    "ngicp_scan_context_distances", "ngicp_scan_context_match", "ngicp_scan_context_kernel_ms",
    "ngicp_voxel_pose_search", "ngicp_voxel_pose_search_scores", "ngicp_voxel_pose_search_kernel_ms",
    "ngicp_keyframe_get", "ngicp_keyframe_transform", "ngicp_keyframe_transform_kernel_ms",
    "ngicp_pose_graph_clear", "ngicp_pose_graph_size", "ngicp_pose_graph_add_nodes", "ngicp_pose_graph_add_edges", "ngicp_pose_graph_get_edges",
    "ngicp_pose_graph_set_fixed", "ngicp_pose_graph_get_fixed", "ngicp_pose_graph_set_robust", "ngicp_pose_graph_get_poses", "ngicp_pose_graph_set_poses",
    "ngicp_pose_graph_linearize", "ngicp_pose_graph_multiply", "ngicp_pose_graph_optimize", "ngicp_pose_graph_corrections", "ngicp_pose_graph_kernel_ms",
]


class RayClearOptions(C.Structure):
    """ngicp_ray_clear_options (include/ngicp.h, "rolling voxel map: clearing along rays")."""
    _fields_ = [("near_cells", C.c_int), ("back_cells", C.c_int), ("max_steps", C.c_int), ("min_miss", C.c_int), ("radius_cells", C.c_double),
                ("keep_stamp", C.c_longlong), ("dry_run", C.c_int)]
    DEFAULTS = dict(near_cells=1, back_cells=2, max_steps=4096, min_miss=2, radius_cells=0.25, keep_stamp=0, dry_run=0)


class RayClearResult(C.Structure):
    """ngicp_ray_clear_result."""
    _fields_ = [("n_removed", C.c_size_t), ("steps", C.c_longlong), ("occupied", C.c_longlong), ("misses", C.c_longlong), ("kernel_ms", C.c_double)]


class GateOptions(C.Structure):
    """ngicp_gate_options (include/ngicp.h, "rolling voxel map: gated insert"); max_mahalanobis has no default."""
    _fields_ = [("max_mahalanobis", C.c_double), ("min_voxel_count", C.c_int), ("insert_new", C.c_int), ("insert_unjudged", C.c_int), ("dry_run", C.c_int)]
    DEFAULTS = dict(min_voxel_count=1, insert_new=1, insert_unjudged=1, dry_run=0)


class GateResult(C.Structure):
    """ngicp_gate_result."""
    _fields_ = [("n_points", C.c_size_t), ("n_class", C.c_size_t * 4), ("n_kept", C.c_size_t), ("n_new", C.c_size_t), ("n_touched", C.c_size_t),
                ("kernel_ms", C.c_double)]


GATE_NEW, GATE_EXPLAINED, GATE_CONFLICT, GATE_UNJUDGED = 0, 1, 2, 3  # NGICP_GATE_*: the classes of a gated insert

PG_TRACE_CAP = 256  # NGICP_PG_TRACE_CAP


class PgOptions(C.Structure):
    """ngicp_pg_options (include/ngicp.h, "pose graph")."""
    _fields_ = [("max_iterations", C.c_int), ("rot_eps", C.c_double), ("trans_eps", C.c_double), ("cg_tol", C.c_double), ("cg_max_iterations", C.c_int)]


class PgResult(C.Structure):
    """ngicp_pg_result."""
    _fields_ = [("initial_chi2", C.c_double), ("final_chi2", C.c_double), ("iterations", C.c_int), ("accepted", C.c_int), ("cg_iterations", C.c_longlong),
                ("converged", C.c_int), ("n_trace", C.c_int), ("trace", C.c_double * (PG_TRACE_CAP * 5))]


PG_DEFAULTS = dict(max_iterations=64, rot_eps=2e-3, trans_eps=5e-4, cg_tol=1e-8, cg_max_iterations=1000)


class VoxelFitness(C.Structure):
    """ngicp_voxel_fitness_t (include/ngicp.h, "voxel fitness")."""
    _fields_ = [("mahalanobis", C.c_double), ("sqdist", C.c_double), ("n_inliers", C.c_size_t), ("n_matched", C.c_size_t)]


class Deskew(C.Structure):
    """ngicp_deskew_t (include/ngicp.h, "motion deskew")."""
    _fields_ = [("times", C.c_void_p), ("time_stride_bytes", C.c_size_t), ("time_offset_bytes", C.c_long), ("time_format", C.c_int),
                ("time_offset", C.c_double), ("n_poses", C.c_size_t), ("pose_times", c_f64p), ("poses_colmajor", c_f64p),
                ("T_ref_colmajor", c_f64p)]


TIME_F32_S, TIME_F64_S, TIME_U32_NS = 0, 1, 2  # NGICP_TIME_*
DESKEW_MAX_POSES = 256                          # NGICP_DESKEW_MAX_POSES
_TIME_FORMAT_OF = {np.dtype(np.float32): TIME_F32_S, np.dtype(np.float64): TIME_F64_S, np.dtype(np.uint32): TIME_U32_NS}

BATCH_MAX_LANES = 64  # NGICP_BATCH_MAX_LANES (include/ngicp.h): guesses per alignBatch call

_lib = None


def load_library() -> C.CDLL:
    """Load the HIP extension.  Fails loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64; importing torch first makes
    # this extension bind to that same runtime (loading /opt/rocm's copy first leaves torch without GPUs).
    import torch  # noqa: F401  (plumbing: streams, device memory for collectives, torch.distributed)
    if not os.path.exists(_LIB_PATH):
        raise ImportError(f"{_LIB_PATH} not found: build it with `python -m direct_lidar_odometry_amd.build` "
                          "(or __graft_entry__.build()); this package has no CPU fallback")
    L = C.CDLL(_LIB_PATH)
    vp = C.c_void_p
    L.ngicp_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.ngicp_destroy.argtypes = [vp]
    L.ngicp_last_error.argtypes = [vp]
    L.ngicp_last_error.restype = C.c_char_p
    L.ngicp_version.restype = C.c_char_p
    L.ngicp_set_params.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int]
    L.ngicp_set_tuning.argtypes = [vp, C.c_double, C.c_int]
    L.ngicp_set_host_wait.argtypes = [vp, C.c_int]
    L.ngicp_covs_shard_begin.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.ngicp_covs_shard_compute.argtypes = [vp, C.c_int, C.c_size_t, C.c_size_t, vp]
    L.ngicp_covs_shard_commit.argtypes = [vp, C.c_int]
    for n in ("ngicp_set_source", "ngicp_register_source", "ngicp_set_target"):
        getattr(L, n).argtypes = [vp, c_f32p, C.c_size_t, C.c_size_t, C.c_uint64]
    for n in ("ngicp_clear_source", "ngicp_clear_target", "ngicp_swap_source_target", "ngicp_compute_source_covs",
              "ngicp_compute_target_covs", "ngicp_clear_source_covs", "ngicp_clear_target_covs"):
        getattr(L, n).argtypes = [vp]
    L.ngicp_share_source_index.argtypes = [vp, vp]
    L.ngicp_copy_source_covs.argtypes = [vp, vp]
    L.ngicp_source_covs_size.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.ngicp_target_covs_size.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.ngicp_get_source_covs.argtypes = [vp, c_f64p]
    L.ngicp_get_target_covs.argtypes = [vp, c_f64p]
    L.ngicp_set_source_covs.argtypes = [vp, c_f64p, C.c_size_t]
    L.ngicp_set_target_covs.argtypes = [vp, c_f64p, C.c_size_t]
    L.ngicp_align.argtypes = [vp, c_f32p, c_f32p, c_i32p, c_i32p, c_f64p, c_f32p, C.c_size_t]
    L.ngicp_linearize.argtypes = [vp, c_f64p, c_f64p, c_f64p, c_f64p]
    L.ngicp_compute_error.argtypes = [vp, c_f64p, c_f64p]
    L.ngicp_get_correspondences.argtypes = [vp, c_i32p, c_f32p]
    L.ngicp_target_knn.argtypes = [vp, c_f32p, C.c_size_t, C.c_size_t, C.c_int, c_i32p, c_f32p]
    L.ngicp_knn_search.argtypes = [vp, C.c_int, c_f32p, C.c_size_t, C.c_size_t, C.c_int, c_i32p, c_f32p]
    L.ngicp_radius_search.argtypes = [vp, C.c_int, c_f32p, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.ngicp_radius_fetch.argtypes = [vp, c_i32p, c_f32p, C.c_size_t]
    L.ngicp_fitness_score.argtypes = [vp, c_f32p, C.c_double, c_f64p, C.POINTER(C.c_size_t)]
    L.ngicp_range_select.argtypes = [vp, C.c_int, C.c_size_t, c_f32p, C.POINTER(C.c_size_t)]
    L.ngicp_range_median.argtypes = [vp, C.c_int, c_f32p, C.POINTER(C.c_size_t)]
    L.ngicp_get_lm_trace.argtypes = [vp, c_f64p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ngicp_align_batch.argtypes = [vp, C.c_size_t, c_f32p, c_f32p, c_i32p, c_i32p, c_f64p]
    L.ngicp_voxel_align_batch.argtypes = [vp, C.c_size_t, c_f32p, c_f32p, c_i32p, c_i32p, c_f64p]
    L.ngicp_batch_get_lm_trace.argtypes = [vp, C.c_size_t, c_f64p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ngicp_fitness_score_batch.argtypes = [vp, C.c_size_t, c_f32p, C.c_double, c_f64p, C.POINTER(C.c_size_t)]
    L.ngicp_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.ngicp_set_profiling.argtypes = [vp, C.c_int]
    L.ngicp_sharded_begin.argtypes = [vp, c_f32p]
    L.ngicp_sharded_pass.argtypes = [vp, vp, vp]
    L.ngicp_sharded_step.argtypes = [vp, vp, vp, c_i32p]
    L.ngicp_sharded_finish.argtypes = [vp, c_f32p, c_i32p, c_i32p, c_f64p]
    L.ngicp_keyframe_add.argtypes = [vp, vp, c_i32p]
    L.ngicp_keyframe_add_transformed.argtypes = [vp, vp, c_f32p, c_i32p]
    L.ngicp_keyframe_add_transformed_filtered.argtypes = [vp, vp, c_f32p, C.c_float, c_i32p]
    L.ngicp_keyframe_count.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.ngicp_keyframe_size.argtypes = [vp, C.c_int, C.POINTER(C.c_size_t)]
    L.ngicp_keyframe_clear.argtypes = [vp]
    L.ngicp_keyframe_get.argtypes = [vp, C.c_int, c_f32p, C.c_size_t, c_f64p, C.POINTER(C.c_size_t)]
    L.ngicp_keyframe_transform.argtypes = [vp, c_i32p, C.c_size_t, c_f32p, c_i32p]
    L.ngicp_keyframe_transform_kernel_ms.argtypes = [vp, c_f64p]
    L.ngicp_submap_set.argtypes = [vp, c_i32p, C.c_size_t, c_i32p]
    L.ngicp_get_target_points.argtypes = [vp, c_f32p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ngicp_transform_source.argtypes = [vp, c_f32p, c_f32p, C.c_size_t]
    L.ngicp_transform_cloud.argtypes = [vp, c_f32p, C.c_size_t, C.c_size_t, c_f32p, c_f32p, C.c_size_t]
    L.ngicp_measure_copy_bandwidth.argtypes = [vp, C.c_size_t, C.c_int, c_f64p]
    L.ngicp_preprocess_scan.argtypes = [vp, c_f32p, C.c_size_t, C.c_size_t, C.c_long, C.c_int, C.c_float, C.c_float, c_f32p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ngicp_set_source_preprocessed.argtypes = [vp, C.c_uint64]
    L.ngicp_deskew_cloud.argtypes = [vp, c_f32p, C.c_size_t, C.c_size_t, C.POINTER(Deskew), c_f32p, C.c_size_t]
    L.ngicp_preprocess_scan_deskewed.argtypes = [vp, c_f32p, C.c_size_t, C.c_size_t, C.c_long, C.POINTER(Deskew), C.c_int, C.c_float, C.c_float, c_f32p,
                                                 C.c_size_t, C.POINTER(C.c_size_t)]
    L.ngicp_map_add.argtypes = [vp, c_f32p, C.c_size_t, C.c_size_t, C.c_long]
    L.ngicp_map_voxel_filter.argtypes = [vp, C.c_float, C.POINTER(C.c_size_t)]
    L.ngicp_map_size.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.ngicp_map_get.argtypes = [vp, c_f32p, C.c_size_t]
    L.ngicp_map_clear.argtypes = [vp]
    L.ngicp_math_selftest.argtypes = [vp, C.c_int, c_f64p, C.c_size_t, c_f64p]
    L.ngicp_step_selftest.argtypes = [vp, c_f64p, C.c_size_t, C.POINTER(C.c_ubyte), C.POINTER(C.c_size_t)]
    L.ngicp_set_voxel_resolution.argtypes = [vp, C.c_double]
    L.ngicp_voxelmap_size.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.ngicp_voxelmap_get.argtypes = [vp, c_i32p, c_f64p, c_f64p, c_i32p]
    L.ngicp_set_voxel_neighbors.argtypes = [vp, C.c_int]
    L.ngicp_get_voxel_neighbors.argtypes = [vp, c_i32p]
    L.ngicp_voxel_correspondences.argtypes = [vp, c_i32p, C.c_size_t, c_i32p]
    L.ngicp_voxelmap_builds.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.ngicp_set_voxel_submap_merge.argtypes = [vp, C.c_int]
    L.ngicp_get_voxel_submap_merge.argtypes = [vp, c_i32p]
    L.ngicp_voxelmap_merge_stats.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), c_f64p, c_f64p]
    L.ngicp_keyframe_voxelmap_get.argtypes = [vp, C.c_int, C.POINTER(C.c_size_t), c_i32p, c_f64p, c_f64p, c_i32p]
    c_i64p, c_szp = C.POINTER(C.c_longlong), C.POINTER(C.c_size_t)
    L.ngicp_set_voxel_rolling.argtypes = [vp, C.c_int]
    L.ngicp_get_voxel_rolling.argtypes = [vp, c_i32p]
    L.ngicp_voxel_rolling_insert.argtypes = [vp, vp, c_f32p, c_szp, c_szp]
    L.ngicp_voxel_rolling_evict.argtypes = [vp, c_f32p, C.c_double, C.c_longlong, c_szp]
    L.ngicp_voxel_rolling_clear.argtypes = [vp]
    L.ngicp_voxel_rolling_get.argtypes = [vp, c_szp, c_i32p, c_f64p, c_f64p, c_i32p, c_i64p]
    L.ngicp_voxel_rolling_stats.argtypes = [vp, c_i64p, c_szp, c_szp, c_szp, c_f64p, c_f64p]
    L.ngicp_voxel_rolling_set.argtypes = [vp, C.c_size_t, c_i32p, c_f64p, c_f64p, c_i32p, c_i64p, C.c_longlong]
    L.ngicp_voxel_rolling_insert_voxels.argtypes = [vp, C.c_size_t, c_f64p, c_f64p, c_i32p, c_f32p, c_szp, c_szp]
    L.ngicp_voxel_rolling_insert_map.argtypes = [vp, vp, c_f32p, c_szp, c_szp]
    L.ngicp_voxel_rolling_transform.argtypes = [vp, c_f32p, c_szp]
    c_u32p = C.POINTER(C.c_uint32)
    L.ngicp_voxel_rolling_ray_clear.argtypes = [vp, vp, c_f32p, c_f32p, C.POINTER(RayClearOptions), C.POINTER(RayClearResult)]
    L.ngicp_voxel_rolling_ray_counts.argtypes = [vp, c_u32p, c_u32p, C.c_size_t, c_szp]
    L.ngicp_voxel_rolling_insert_gated.argtypes = [vp, vp, c_f32p, C.POINTER(GateOptions), C.POINTER(GateResult)]
    L.ngicp_voxel_rolling_insert_classes.argtypes = [vp, C.POINTER(C.c_uint8), C.c_size_t, c_szp]
    L.ngicp_set_robust_kernel.argtypes = [vp, C.c_int, C.c_double]
    L.ngicp_get_robust_kernel.argtypes = [vp, c_i32p, c_f64p]
    L.ngicp_robust_terms.argtypes = [vp, c_f64p, c_f64p, c_f64p, C.c_size_t, c_i32p]
    L.ngicp_set_pose_prior.argtypes = [vp, c_f64p, c_f64p]
    L.ngicp_get_pose_prior.argtypes = [vp, c_i32p, c_f64p, c_f64p]
    L.ngicp_pose_prior_terms.argtypes = [vp, c_f64p, c_f64p, c_f64p, c_f64p, c_f64p]
    L.ngicp_voxel_fitness.argtypes = [vp, c_f32p, C.c_double, C.POINTER(VoxelFitness)]
    L.ngicp_voxel_fitness_batch.argtypes = [vp, C.c_size_t, c_f32p, C.c_double, C.POINTER(VoxelFitness)]
    L.ngicp_voxel_fitness_points.argtypes = [vp, c_f32p, c_f64p, c_f64p, c_i32p, C.c_size_t]
    L.ngicp_voxel_fitness_kernel_ms.argtypes = [vp, c_f64p]
    L.ngicp_scan_context_set_params.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_float]
    L.ngicp_scan_context_get_params.argtypes = [vp, c_i32p, c_i32p, c_f32p, c_f32p]
    L.ngicp_scan_context_tables.argtypes = [vp, c_f32p, c_f32p]
    L.ngicp_scan_context_compute.argtypes = [vp, C.c_int, c_f32p]
    L.ngicp_scan_context_add.argtypes = [vp, C.c_int, c_i32p]
    L.ngicp_scan_context_add_descriptor.argtypes = [vp, c_f32p, c_i32p]
    L.ngicp_scan_context_count.argtypes = [vp, c_szp]
    L.ngicp_scan_context_get.argtypes = [vp, C.c_int, c_f32p]
    L.ngicp_scan_context_clear.argtypes = [vp]
    L.ngicp_scan_context_distances.argtypes = [vp, C.c_int, c_f32p, C.c_size_t, C.c_size_t, c_f64p, c_i32p]
    L.ngicp_scan_context_match.argtypes = [vp, C.c_int, c_f32p, C.c_size_t, C.c_size_t, C.c_int, c_i32p, c_f64p, c_i32p, c_szp]
    L.ngicp_scan_context_kernel_ms.argtypes = [vp, c_f64p]
    L.ngicp_voxel_pose_search.argtypes = [vp, C.c_size_t, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_i32p, c_i32p, c_i32p, c_szp]
    L.ngicp_voxel_pose_search_scores.argtypes = [vp, c_i32p, C.c_size_t]
    L.ngicp_voxel_pose_search_kernel_ms.argtypes = [vp, c_f64p]
    c_u8p = C.POINTER(C.c_ubyte)
    L.ngicp_pose_graph_clear.argtypes = [vp]
    L.ngicp_pose_graph_size.argtypes = [vp, c_szp, c_szp]
    L.ngicp_pose_graph_add_nodes.argtypes = [vp, c_f64p, c_u8p, C.c_size_t, c_i32p]
    L.ngicp_pose_graph_add_edges.argtypes = [vp, c_i32p, c_f64p, c_f64p, c_u8p, C.c_size_t, c_i32p]
    L.ngicp_pose_graph_get_edges.argtypes = [vp, C.c_int, C.c_size_t, c_i32p, c_f64p, c_f64p, c_u8p]
    L.ngicp_pose_graph_set_fixed.argtypes = [vp, c_i32p, c_u8p, C.c_size_t]
    L.ngicp_pose_graph_get_fixed.argtypes = [vp, C.c_int, C.c_size_t, c_u8p]
    L.ngicp_pose_graph_set_robust.argtypes = [vp, C.c_int, C.c_double]
    L.ngicp_pose_graph_get_poses.argtypes = [vp, C.c_int, C.c_size_t, c_f64p]
    L.ngicp_pose_graph_set_poses.argtypes = [vp, C.c_int, C.c_size_t, c_f64p]
    L.ngicp_pose_graph_linearize.argtypes = [vp, c_f64p, c_f64p, c_f64p, c_f64p, c_f64p]
    L.ngicp_pose_graph_multiply.argtypes = [vp, C.c_double, c_f64p, c_f64p]
    L.ngicp_pose_graph_optimize.argtypes = [vp, C.POINTER(PgOptions), C.POINTER(PgResult)]
    L.ngicp_pose_graph_corrections.argtypes = [vp, c_i32p, C.c_size_t, c_f64p, c_f32p]
    L.ngicp_pose_graph_kernel_ms.argtypes = [vp, c_f64p]
    _lib = L
    return L


def _p(a: np.ndarray, ty):
    return a.ctypes.data_as(ty)


def _cloud(a) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] < 3 or not a.flags.c_contiguous:
        a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("cloud must have shape (N, C>=3)")
    return a


def _colmajor16(T, dtype) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(T, dtype=dtype).T.reshape(16))


class NanoGICP:
    """Drop-in mirror of nano_gicp::NanoGICP on one MI355X (see module docstring)."""

    def __init__(self, device: int = 0):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.ngicp_create(device, C.byref(h))
        if rc != 0:
            raise NgicpError(rc, (self._L.ngicp_last_error(None) or b"").decode())
        self._h = h
        self.device = device
        # defaults: impl/nano_gicp_impl.hpp:50-64, impl/lsq_registration_impl.hpp:50-63
        self._p = dict(k=20, max_corr_dist=FLT_MAX, max_iter=64, trans_eps=5e-4, rot_eps=2e-3,
                       optimizer=int(LSQ_OPTIMIZER_TYPE.LevenbergMarquardt), lm_max_iter=10, lm_init_lambda_factor=1e-9,
                       regularization=int(RegularizationMethod.PLANE), num_threads=0)
        self._src = None
        self._tgt = None
        self.final_transformation_ = np.eye(4, dtype=np.float32)
        self.converged_ = False
        self.nr_iterations_ = 0
        self.final_hessian_ = np.eye(6)

    def close(self):
        if getattr(self, "_h", None):
            self._L.ngicp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- plumbing ----
    def _ck(self, rc: int):
        if rc != 0:
            raise NgicpError(rc, (self._L.ngicp_last_error(self._h) or b"").decode())

    def _push(self):
        p = self._p
        self._ck(self._L.ngicp_set_params(self._h, p["k"], p["max_corr_dist"], p["max_iter"], p["trans_eps"], p["rot_eps"], p["optimizer"],
                                          p["lm_max_iter"], p["lm_init_lambda_factor"], p["regularization"], p["num_threads"]))

    # ---- NanoGICP / LsqRegistration / pcl::Registration setters ----
    def setNumThreads(self, n: int): self._p["num_threads"] = int(n); self._push()                  # impl/nano_gicp_impl.hpp:70-78
    def setCorrespondenceRandomness(self, k: int): self._p["k"] = int(k); self._push()              # :81-83
    def setRegularizationMethod(self, m): self._p["regularization"] = int(m); self._push()          # :86-88
    def setMaxCorrespondenceDistance(self, d: float): self._p["max_corr_dist"] = float(d); self._push()
    def setMaximumIterations(self, n: int): self._p["max_iter"] = int(n); self._push()
    def setTransformationEpsilon(self, e: float): self._p["trans_eps"] = float(e); self._push()
    def setRotationEpsilon(self, e: float): self._p["rot_eps"] = float(e); self._push()             # impl/lsq_registration_impl.hpp:69-71
    def setInitialLambdaFactor(self, f: float): self._p["lm_init_lambda_factor"] = float(f); self._push()  # :74-76
    def setOptimizer(self, t): self._p["optimizer"] = int(t); self._push()
    def setLMMaxIterations(self, n: int): self._p["lm_max_iter"] = int(n); self._push()
    # accepted and ignored, like the reference (odom.cc:104-106,112-120)
    def setEuclideanFitnessEpsilon(self, e): pass
    def setRANSACIterations(self, n): pass
    def setRANSACOutlierRejectionThreshold(self, t): pass
    def setSearchMethodSource(self, tree=None, force_no_recompute=True): pass
    def setSearchMethodTarget(self, tree=None, force_no_recompute=True): pass
    def setDebugPrint(self, on: bool): self._debug = bool(on)

    def setHostWaitMode(self, mode: int):
        """0: the calling thread polls the device without giving its core up (default); 1: it yields between polls."""
        self._ck(self._L.ngicp_set_host_wait(self._h, int(mode)))

    def setVoxelResolution(self, res: float):
        """res > 0: voxelized GICP - align against one Gaussian per occupied target voxel of edge `res` (include/ngicp.h "voxelized GICP");
        0 (the default): exact GICP.  In this mode setMaxCorrespondenceDistance is not consulted (voxel membership is the gate),
        correspondences() returns voxel numbers, and alignBatch / the sharded entries raise."""
        self._ck(self._L.ngicp_set_voxel_resolution(self._h, float(res)))
        self._voxel_res = float(res)

    def getVoxelResolution(self) -> float: return getattr(self, "_voxel_res", 0.0)

    def getVoxelMapSize(self) -> int: return self._covs_size("ngicp_voxelmap_size")

    def setNeighborSearchMethod(self, method):
        """DIRECT1 (default): a source point is matched against the voxel it falls into; DIRECT7: that voxel and its 6 face neighbours;
        DIRECT27: all 27.  Remembered while the voxel mode is off; a change keeps the voxel map and drops the correspondences."""
        self._ck(self._L.ngicp_set_voxel_neighbors(self._h, int(method)))

    def getNeighborSearchMethod(self) -> NeighborSearchMethod:
        m = C.c_int(0)
        self._ck(self._L.ngicp_get_voxel_neighbors(self._h, C.byref(m)))
        return NeighborSearchMethod(m.value)

    def voxel_correspondences(self) -> np.ndarray:
        """-> (n, K) int32: the voxel number of every slot of the last linearisation per source point (original order), -1 where empty."""
        n, K = self._src.shape[0], int(self.getNeighborSearchMethod())
        out = np.empty((n, K), dtype=np.int32); k = C.c_int(0)
        self._ck(self._L.ngicp_voxel_correspondences(self._h, _p(out, c_i32p), out.size, C.byref(k)))
        assert k.value == K
        return out

    def voxelMapBuilds(self) -> int:
        """Voxel maps built on this handle so far (only a build counts)."""
        b = C.c_longlong(0)
        self._ck(self._L.ngicp_voxelmap_builds(self._h, C.byref(b)))
        return b.value

    def voxelMap(self):
        """-> (ijk (V, 3) int32, mean (V, 3), cov (V, 3, 3), count (V,) int32) of the target's voxel map, voxels in ascending (iz, iy, ix)."""
        n = self.getVoxelMapSize()
        ijk = np.empty((n, 3), dtype=np.int32); mean = np.empty((n, 3)); c6 = np.empty((n, 6)); cnt = np.empty(n, dtype=np.int32)
        self._ck(self._L.ngicp_voxelmap_get(self._h, _p(ijk, c_i32p), _p(mean, c_f64p), _p(c6, c_f64p), _p(cnt, c_i32p)))
        cov = c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(n, 3, 3)
        return ijk, mean, cov, cnt

    def setVoxelSubmapMerge(self, on: bool):
        """Off (the default): the voxel map of every target is summed over its points.  On: the map of a submap assembled by
        setSubmapKeyframes is merged from per-keyframe voxel sums, built once per keyframe and resolution (include/ngicp.h "merged voxel
        map": the same voxels and counts, means and covariances that differ in rounding only).  Remembered while the voxel mode is off."""
        self._ck(self._L.ngicp_set_voxel_submap_merge(self._h, 1 if on else 0))

    def getVoxelSubmapMerge(self) -> bool:
        on = C.c_int(0)
        self._ck(self._L.ngicp_get_voxel_submap_merge(self._h, C.byref(on)))
        return bool(on.value)

    def voxelMapMergeStats(self) -> dict:
        """{merged_builds, parts_built: since the handle was created; last_parts_ms, last_merge_ms: device time of the last merged build}."""
        mb, pb, tp, tm = C.c_longlong(0), C.c_longlong(0), C.c_double(0), C.c_double(0)
        self._ck(self._L.ngicp_voxelmap_merge_stats(self._h, C.byref(mb), C.byref(pb), C.byref(tp), C.byref(tm)))
        return dict(merged_builds=mb.value, parts_built=pb.value, last_parts_ms=tp.value, last_merge_ms=tm.value)

    def keyframeVoxelMap(self, kid: int):
        """-> (ijk (V, 3) int32, sum (V, 3), covsum (V, 3, 3), count (V,) int32): the voxel part of keyframe `kid` at the current
        resolution (sums, not means), voxels in ascending (iz, iy, ix); built if absent."""
        nv = C.c_size_t(0)
        self._ck(self._L.ngicp_keyframe_voxelmap_get(self._h, int(kid), C.byref(nv), None, None, None, None))
        n = nv.value
        ijk = np.empty((n, 3), dtype=np.int32); s = np.empty((n, 3)); c6 = np.empty((n, 6)); cnt = np.empty(n, dtype=np.int32)
        self._ck(self._L.ngicp_keyframe_voxelmap_get(self._h, int(kid), C.byref(nv), _p(ijk, c_i32p), _p(s, c_f64p), _p(c6, c_f64p), _p(cnt, c_i32p)))
        return ijk, s, c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(n, 3, 3), cnt

    # ---- the rolling voxel map (include/ngicp.h "rolling voxel map") ----
    def setVoxelRolling(self, on: bool):
        """Off (the default): the voxel map is that of the target.  On (with setVoxelResolution > 0): align / linearize / compute_error /
        alignBatchVoxel / voxelMap use a map that insertIntoVoxelMap and evictVoxelMap maintain across frames; the target is not read at
        all.  Remembered while the voxel mode is off; switching off keeps the rolling map for the next time it is switched on."""
        self._ck(self._L.ngicp_set_voxel_rolling(self._h, 1 if on else 0))

    def getVoxelRolling(self) -> bool:
        on = C.c_int(0)
        self._ck(self._L.ngicp_get_voxel_rolling(self._h, C.byref(on)))
        return bool(on.value)

    def insertIntoVoxelMap(self, producer: "NanoGICP", T) -> tuple:
        """Add the producer's source cloud (the producer may be this object), transformed by the float pose T, to the rolling map with
        its source covariances (computed if missing, as addKeyframe does).  -> (voxels created, voxels of the scan).  A scan with a
        transformed point that has no voxel raises and changes nothing."""
        t = _colmajor16(T, np.float32); n_new, n_touched = C.c_size_t(0), C.c_size_t(0)
        self._ck(self._L.ngicp_voxel_rolling_insert(self._h, producer._h, _p(t, c_f32p), C.byref(n_new), C.byref(n_touched)))
        return n_new.value, n_touched.value

    def evictVoxelMap(self, centre=(0.0, 0.0, 0.0), max_dist: float = 0.0, min_stamp: int = 0) -> int:
        """Remove the voxels whose centre lies farther than max_dist from `centre` (max_dist > 0) or whose last insert is older than
        min_stamp (min_stamp > 0; inserts count from 1).  Survivors keep their order.  -> voxels removed."""
        c = np.ascontiguousarray(centre, dtype=np.float32).reshape(3); n = C.c_size_t(0)
        self._ck(self._L.ngicp_voxel_rolling_evict(self._h, _p(c, c_f32p), float(max_dist), int(min_stamp), C.byref(n)))
        return n.value

    def clearVoxelMap(self): self._ck(self._L.ngicp_voxel_rolling_clear(self._h))

    def rollingVoxelMap(self):
        """-> (ijk (V, 3) int32, sum (V, 3), covsum (V, 3, 3), count (V,) int32, stamp (V,) int64): the rolling map's state, voxels in
        order of first insertion (voxelMap() gives the means and covariances in the same numbering while the setting is on)."""
        nv = C.c_size_t(0)
        self._ck(self._L.ngicp_voxel_rolling_get(self._h, C.byref(nv), None, None, None, None, None))
        n = nv.value
        ijk = np.empty((n, 3), dtype=np.int32); s = np.empty((n, 3)); c6 = np.empty((n, 6)); cnt = np.empty(n, dtype=np.int32)
        st = np.empty(n, dtype=np.int64)
        self._ck(self._L.ngicp_voxel_rolling_get(self._h, C.byref(nv), _p(ijk, c_i32p), _p(s, c_f64p), _p(c6, c_f64p), _p(cnt, c_i32p),
                                                 _p(st, C.POINTER(C.c_longlong))))
        return ijk, s, c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(n, 3, 3), cnt, st

    def voxelRollingStats(self) -> dict:
        """{inserts: accepted since the last clear; n_vox, capacity_vox, table_slots; last_insert_ms, last_evict_ms: device event times}."""
        ins, nv, cap, sl = C.c_longlong(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        ti, te = C.c_double(0), C.c_double(0)
        self._ck(self._L.ngicp_voxel_rolling_stats(self._h, C.byref(ins), C.byref(nv), C.byref(cap), C.byref(sl), C.byref(ti), C.byref(te)))
        return dict(inserts=ins.value, n_vox=nv.value, capacity_vox=cap.value, table_slots=sl.value, last_insert_ms=ti.value, last_evict_ms=te.value)

    # ---- the rolling map from voxel records (include/ngicp.h "rolling voxel map: records") ----
    @staticmethod
    def _records(S, Cm, count):
        """(S (n, 3), C (n, 3, 3) or (n, 6), count (n,)) as the contiguous arrays of the C ABI"""
        s = np.ascontiguousarray(S, dtype=np.float64).reshape(-1, 3)
        c = np.asarray(Cm, dtype=np.float64)
        c6 = np.ascontiguousarray(c.reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]] if c.ndim == 3 else c.reshape(-1, 6))
        cnt = np.asarray(count)
        if cnt.size and (cnt.min() < -2**31 or cnt.max() > 2**31 - 1):
            raise ValueError("a count outside the int range")
        cnt = np.ascontiguousarray(cnt, dtype=np.int32).reshape(-1)
        if not (len(s) == len(c6) == len(cnt)):
            raise ValueError(f"{len(s)} sums, {len(c6)} covariance sums and {len(cnt)} counts")
        return s, c6, cnt

    def setRollingVoxelMap(self, ijk, S, C_, count, stamp, inserts: int):
        """The rolling map becomes exactly the given state (what rollingVoxelMap() and voxelRollingStats()['inserts'] return): voxel v
        has key ijk[v], sums S[v], C[v], count[v] and stamp[v], numbered in array order; the insert counter becomes `inserts`.  A bad
        argument (an index of 2^20 or more, a count below 1, a stamp outside 1..inserts, two equal ijk rows) raises and changes nothing."""
        s, c6, cnt = self._records(S, C_, count)
        k = np.ascontiguousarray(ijk, dtype=np.int32).reshape(-1, 3)
        st = np.ascontiguousarray(stamp, dtype=np.int64).reshape(-1)
        if not (len(k) == len(st) == len(s)):
            raise ValueError(f"{len(k)} ijk rows, {len(st)} stamps and {len(s)} sums")
        self._ck(self._L.ngicp_voxel_rolling_set(self._h, len(s), _p(k, c_i32p), _p(s, c_f64p), _p(c6, c_f64p), _p(cnt, c_i32p),
                                                 _p(st, C.POINTER(C.c_longlong)), int(inserts)))

    def insertVoxelsIntoVoxelMap(self, S, C_, count, T) -> tuple:
        """Add voxel records (sums S (n, 3), covariance sums C (n, 3, 3) or (n, 6), counts) to the rolling map at the float pose T: every
        record lands, whole, in the voxel of its moved mean.  -> (voxels created, destination voxels).  A refused insert raises and
        changes nothing."""
        s, c6, cnt = self._records(S, C_, count)
        t = _colmajor16(T, np.float32); n_new, n_touched = C.c_size_t(0), C.c_size_t(0)
        self._ck(self._L.ngicp_voxel_rolling_insert_voxels(self._h, len(s), _p(s, c_f64p), _p(c6, c_f64p), _p(cnt, c_i32p), _p(t, c_f32p),
                                                           C.byref(n_new), C.byref(n_touched)))
        return n_new.value, n_touched.value

    def insertVoxelMapFrom(self, other: "NanoGICP", T) -> tuple:
        """insertVoxelsIntoVoxelMap of the other handle's rolling map, read on the device (it never passes through the host).  The other
        handle need neither have the rolling setting on nor this handle's resolution; it is left unchanged."""
        t = _colmajor16(T, np.float32); n_new, n_touched = C.c_size_t(0), C.c_size_t(0)
        self._ck(self._L.ngicp_voxel_rolling_insert_map(self._h, other._h, _p(t, c_f32p), C.byref(n_new), C.byref(n_touched)))
        return n_new.value, n_touched.value

    def transformVoxelMap(self, T) -> int:
        """Move the rolling map by the float pose T in place: its former records inserted into an empty map.  The insert counter stays
        and a voxel keeps the largest stamp of the records that landed in it.  -> voxels after the move."""
        t = _colmajor16(T, np.float32); n = C.c_size_t(0)
        self._ck(self._L.ngicp_voxel_rolling_transform(self._h, _p(t, c_f32p), C.byref(n)))
        return n.value

    # ---- clearing the rolling map along a scan's rays (include/ngicp.h "rolling voxel map: clearing along rays") ----
    def clearVoxelMapAlongRays(self, producer: "NanoGICP", T, origin=None, **options) -> dict:
        """Count, per voxel of the rolling map, the rays of the producer's source cloud at the float pose T that pass through it (miss)
        and that end in it (hit) - from `origin` (three floats in the map frame; None: T's translation) - and remove the voxels with
        at least min_miss misses, no hit and (keep_stamp > 0) a stamp below keep_stamp.  Options (defaults): near_cells (1), back_cells
        (2), max_steps (4096), min_miss (2), radius_cells (0.25), keep_stamp (0), dry_run (0: count and remove; else count only).
        -> {n_removed, steps, occupied, misses, kernel_ms}.  A refused call raises and changes nothing."""
        unknown = set(options) - set(RayClearOptions.DEFAULTS)
        if unknown:
            raise TypeError(f"clearVoxelMapAlongRays: unknown options {sorted(unknown)}")
        o = {**RayClearOptions.DEFAULTS, **options}
        opt = RayClearOptions(int(o["near_cells"]), int(o["back_cells"]), int(o["max_steps"]), int(o["min_miss"]), float(o["radius_cells"]),
                              int(o["keep_stamp"]), int(o["dry_run"]))
        t = _colmajor16(T, np.float32)
        org = None if origin is None else np.ascontiguousarray(origin, dtype=np.float32).reshape(3)
        res = RayClearResult()
        self._ck(self._L.ngicp_voxel_rolling_ray_clear(self._h, producer._h, _p(t, c_f32p), None if org is None else _p(org, c_f32p), C.byref(opt), C.byref(res)))
        return dict(n_removed=res.n_removed, steps=res.steps, occupied=res.occupied, misses=res.misses, kernel_ms=res.kernel_ms)

    def voxelMapRayCounts(self) -> tuple:
        """-> (miss (V,) uint32, hit (V,) uint32) of the last clearVoxelMapAlongRays, in the numbering from before its removal.  Raises
        (NGICP_ERR_STATE) when no call has been accepted or anything else has changed the map since."""
        nv = C.c_size_t(0)
        self._ck(self._L.ngicp_voxel_rolling_ray_counts(self._h, None, None, 0, C.byref(nv)))
        n = nv.value
        miss = np.zeros(n, dtype=np.uint32); hit = np.zeros(n, dtype=np.uint32)
        c_u32p = C.POINTER(C.c_uint32)
        self._ck(self._L.ngicp_voxel_rolling_ray_counts(self._h, _p(miss, c_u32p), _p(hit, c_u32p), n, C.byref(nv)))
        return miss, hit

    # ---- the gated insert into the rolling map (include/ngicp.h "rolling voxel map: gated insert") ----
    def insertIntoVoxelMapGated(self, producer: "NanoGICP", T, max_mahalanobis: float, **options) -> dict:
        """insertIntoVoxelMap of the points the rolling map does not contradict: every point of the producer's source cloud is classified
        against the map at the float pose T - NEW (0, no occupied slot), EXPLAINED (1, best m <= max_mahalanobis), CONFLICT (2, best m
        above it), UNJUDGED (3, occupied slots but no voxel of at least min_voxel_count points gave a finite m) - and the EXPLAINED
        points, the NEW ones (insert_new) and the UNJUDGED ones (insert_unjudged) are inserted exactly as insertIntoVoxelMap would insert
        them alone.  m is voxel_fitness_points' (no voxel-count factor: a chi-square-like value with 3 degrees of freedom).  Options
        (defaults): min_voxel_count (1), insert_new (1), insert_unjudged (1), dry_run (0: classify and insert; else classify only).
        -> {n_points, n_class (4 ints), n_kept, n_new, n_touched, kernel_ms}.  A refused call raises and changes nothing."""
        unknown = set(options) - set(GateOptions.DEFAULTS)
        if unknown:
            raise TypeError(f"insertIntoVoxelMapGated: unknown options {sorted(unknown)}")
        o = {**GateOptions.DEFAULTS, **options}
        opt = GateOptions(float(max_mahalanobis), int(o["min_voxel_count"]), int(o["insert_new"]), int(o["insert_unjudged"]), int(o["dry_run"]))
        t = _colmajor16(T, np.float32)
        res = GateResult()
        self._ck(self._L.ngicp_voxel_rolling_insert_gated(self._h, producer._h, _p(t, c_f32p), C.byref(opt), C.byref(res)))
        return dict(n_points=res.n_points, n_class=[int(c) for c in res.n_class], n_kept=res.n_kept, n_new=res.n_new, n_touched=res.n_touched,
                    kernel_ms=res.kernel_ms)

    def voxelMapInsertClasses(self) -> np.ndarray:
        """-> (n,) uint8: the classes of the last insertIntoVoxelMapGated, dry or not, in the scan's original order.  Raises
        (NGICP_ERR_STATE) before the first such call and after clearVoxelMap."""
        nv = C.c_size_t(0)
        self._ck(self._L.ngicp_voxel_rolling_insert_classes(self._h, None, 0, C.byref(nv)))
        cls = np.zeros(nv.value, dtype=np.uint8)
        self._ck(self._L.ngicp_voxel_rolling_insert_classes(self._h, _p(cls, C.POINTER(C.c_uint8)), nv.value, C.byref(nv)))
        return cls

    def setRobustKernel(self, kind, width: float = 1.0):
        """A robust kernel on every term of the cost (include/ngicp.h "robust kernel"): HUBER, CAUCHY or GEMAN_MCCLURE of the given width
        on s = e^T M e, or NONE (the default).  It holds for align, linearize and compute_error on every route (exact, DIRECT1 / 7 / 27,
        rolling map) and is remembered across mode switches; alignBatch, alignBatchVoxel and the sharded entries raise while it is set."""
        self._ck(self._L.ngicp_set_robust_kernel(self._h, int(kind), float(width)))

    def getRobustKernel(self):
        """-> (RobustKernel, width)"""
        k = C.c_int(0); w = C.c_double(0)
        self._ck(self._L.ngicp_get_robust_kernel(self._h, C.byref(k), C.byref(w)))
        return RobustKernel(k.value), w.value

    def robust_terms(self, T=None):
        """-> (s, w), each (n, K) float64 in original source order: per term s = e^T M e at the pose T (None: the final transformation)
        under the correspondences and matrices of the last linearisation, and the weight the kernel gives it.  K is 1 on the exact route,
        else the neighbourhood's.  No correspondence: s = -1, w = 0."""
        t = _colmajor16(self.final_transformation_ if T is None else T, np.float64)
        n = self._src.shape[0]
        K = int(self.getNeighborSearchMethod()) if self.getVoxelResolution() > 0.0 else 1
        s = np.empty((n, K)); w = np.empty((n, K)); k = C.c_int(0)
        self._ck(self._L.ngicp_robust_terms(self._h, _p(t, c_f64p), _p(s, c_f64p), _p(w, c_f64p), s.size, C.byref(k)))
        assert k.value == K
        return s, w

    def setPosePrior(self, T, info):
        """A Gaussian prior on the pose (include/ngicp.h "pose prior"): the cost gains r^T info r with r = (log_SO3(R R_p^T), t - t_p),
        T = (R_p, t_p) a 4x4 pose and info a symmetric 6x6 information matrix (rotation first).  It holds for align, alignBatch,
        alignBatchVoxel, linearize and compute_error on every route and is remembered across mode switches; the sharded entries and an
        align under NGICP_HEAD raise while it is set."""
        t = _colmajor16(T, np.float64)
        i = np.ascontiguousarray(np.asarray(info, dtype=np.float64).reshape(6, 6).T.reshape(36))
        self._ck(self._L.ngicp_set_pose_prior(self._h, _p(t, c_f64p), _p(i, c_f64p)))

    def clearPosePrior(self):
        self._ck(self._L.ngicp_set_pose_prior(self._h, None, None))

    def getPosePrior(self):
        """-> (T (4, 4), info (6, 6)), or None when no prior is set"""
        k = C.c_int(0); t = np.empty(16); i = np.empty(36)
        self._ck(self._L.ngicp_get_pose_prior(self._h, C.byref(k), _p(t, c_f64p), _p(i, c_f64p)))
        return (t.reshape(4, 4).T.copy(), i.reshape(6, 6).T.copy()) if k.value else None

    def pose_prior_terms(self, T):
        """-> (r (6,), cost, H (6, 6), b (6,)): the prior's share alone at the pose T, evaluated on the device by the solver's functions."""
        t = _colmajor16(T, np.float64)
        r = np.empty(6); H = np.empty(36); b = np.empty(6); c = C.c_double(0)
        self._ck(self._L.ngicp_pose_prior_terms(self._h, _p(t, c_f64p), _p(r, c_f64p), C.byref(c), _p(H, c_f64p), _p(b, c_f64p)))
        return r, c.value, H.reshape(6, 6).T.copy(), b

    def setTuning(self, voxel_size: float = 0.0, lanes_per_query: int = 0):
        self._ck(self._L.ngicp_set_tuning(self._h, float(voxel_size), int(lanes_per_query)))

    # ---- clouds ----
    def _set(self, fn, cloud, identity):
        c = _cloud(cloud)
        ident = int(identity) if identity is not None else int(c.ctypes.data)
        self._ck(getattr(self._L, fn)(self._h, _p(c, c_f32p), c.shape[0], c.strides[0], ident))
        return c

    def setInputSource(self, cloud, identity=None): self._src = self._set("ngicp_set_source", cloud, identity)         # impl/nano_gicp_impl.hpp:121-129
    def registerInputSource(self, cloud, identity=None): self._src = self._set("ngicp_register_source", cloud, identity)  # :113-118
    def setInputTarget(self, cloud, identity=None): self._tgt = self._set("ngicp_set_target", cloud, identity)         # :132-139

    def clearSource(self):
        self._ck(self._L.ngicp_clear_source(self._h)); self._src = None

    def clearTarget(self):
        self._ck(self._L.ngicp_clear_target(self._h)); self._tgt = None

    def swapSourceAndTarget(self):                                                                                      # :91-98
        self._ck(self._L.ngicp_swap_source_target(self._h))
        self._src, self._tgt = self._tgt, self._src

    def shareSourceIndexFrom(self, other: "NanoGICP"):
        """`this.source_kdtree_ = other.source_kdtree_` (odom.cc:525)."""
        self._ck(self._L.ngicp_share_source_index(self._h, other._h))

    # ---- covariances ----
    def calculateSourceCovariances(self) -> bool:
        self._ck(self._L.ngicp_compute_source_covs(self._h)); return True

    def calculateTargetCovariances(self) -> bool:
        self._ck(self._L.ngicp_compute_target_covs(self._h)); return True

    def copySourceCovariancesFrom(self, other: "NanoGICP"):
        """`this.source_covs_ = other.source_covs_` (odom.cc:815) — stays on the device."""
        self._ck(self._L.ngicp_copy_source_covs(self._h, other._h))

    def clearSourceCovariances(self): self._ck(self._L.ngicp_clear_source_covs(self._h))
    def clearTargetCovariances(self): self._ck(self._L.ngicp_clear_target_covs(self._h))

    def _covs_size(self, fn) -> int:
        n = C.c_size_t(0)
        self._ck(getattr(self._L, fn)(self._h, C.byref(n)))
        return n.value

    def sourceCovariancesSize(self) -> int: return self._covs_size("ngicp_source_covs_size")
    def targetCovariancesSize(self) -> int: return self._covs_size("ngicp_target_covs_size")

    def _get_covs(self, fn, n):
        out = np.empty((n, 16), dtype=np.float64)
        if n:
            self._ck(getattr(self._L, fn)(self._h, _p(out, c_f64p)))
        return out.reshape(n, 4, 4).transpose(0, 2, 1).copy()

    def getSourceCovariances(self): return self._get_covs("ngicp_get_source_covs", self.sourceCovariancesSize())
    def getTargetCovariances(self): return self._get_covs("ngicp_get_target_covs", self.targetCovariancesSize())

    @staticmethod
    def _covs_in(covs):
        c = np.asarray(covs, dtype=np.float64)
        if c.ndim != 3 or c.shape[1:] != (4, 4):
            raise ValueError("covariances must have shape (N,4,4)")
        return np.ascontiguousarray(c.transpose(0, 2, 1).reshape(-1, 16))

    def setSourceCovariances(self, covs):
        c = self._covs_in(covs); self._ck(self._L.ngicp_set_source_covs(self._h, _p(c, c_f64p), c.shape[0]))

    def setTargetCovariances(self, covs):
        c = self._covs_in(covs); self._ck(self._L.ngicp_set_target_covs(self._h, _p(c, c_f64p), c.shape[0]))

    # ---- registration ----
    def align(self, guess=None, want_aligned: bool = False):
        """pcl::Registration::align(output[, guess]).  Returns the aligned cloud (N,3) when asked, else None."""
        g = _colmajor16(np.eye(4) if guess is None else guess, np.float32)
        T = np.empty(16, dtype=np.float32)
        H = np.empty(36, dtype=np.float64)
        conv, nit = C.c_int(0), C.c_int(0)
        aligned, ap, stride = None, None, 0
        if want_aligned:
            if self._src is None:
                raise NgicpError(-3, "no source cloud")
            aligned = np.empty((self._src.shape[0], 3), dtype=np.float32)
            ap, stride = _p(aligned, c_f32p), 12
        rc = self._L.ngicp_align(self._h, _p(g, c_f32p), _p(T, c_f32p), C.byref(conv), C.byref(nit), _p(H, c_f64p), ap, stride)
        self.final_transformation_ = T.reshape(4, 4).T.copy()
        self.converged_ = bool(conv.value)
        self.nr_iterations_ = nit.value
        self.final_hessian_ = H.reshape(6, 6).T.copy()
        self._ck(rc)
        if getattr(self, "_debug", False):
            self._print_lm_table()
        return aligned

    def _print_lm_table(self):
        """setDebugPrint(true): the reference's banner and per-trial table (impl/lsq_registration_impl.hpp:95-99,183-189), printed
        from the engine's trace after the device-resident loop has returned."""
        print("********************************************\n***************** optimize *****************\n********************************************")
        for it, trial, y0, yi, rho, lam, dn, _acc in self.lm_trace():
            if int(trial) == 0:
                print("--- LM optimization ---\n%5s %15s %15s %15s %15s %15s %5s" % ("i", "y0", "yi", "rho", "lambda", "|delta|", "dec"))
            print("%5d %15g %15g %15g %15g %15g %5c" % (int(trial), y0, yi, rho, lam, dn, "x" if rho > 0.0 else " "))

    def alignBatch(self, guesses):
        """Several initial guesses on the current source / target pair in the same launches (ngicp_align_batch; no counterpart in
        the reference).  guesses: (B, 4, 4).  -> (T (B, 4, 4) float32, converged (B,) bool, iterations (B,) int32, H (B, 6, 6) float64);
        lane g is bit for bit what align(guesses[g]) gives.  Leaves final_transformation_ and the other results of align() alone."""
        return self._align_batch(self._L.ngicp_align_batch, "alignBatch", guesses)

    def alignBatchVoxel(self, guesses):
        """alignBatch against the voxelized target (ngicp_voxel_align_batch; setVoxelResolution > 0, any neighbourhood): the same
        arguments and the same return tuple; lane g is bit for bit what align(guesses[g]) gives with the voxel mode on.  alignBatch
        itself stays refused in that mode.  lm_trace(lane=g) serves its lanes afterwards."""
        return self._align_batch(self._L.ngicp_voxel_align_batch, "alignBatchVoxel", guesses)

    def _align_batch(self, entry, name, guesses):
        g = np.asarray(guesses)
        if g.ndim != 3 or g.shape[1:] != (4, 4):
            raise NgicpError(-2, f"{name}: guesses must be (B, 4, 4)")
        B = g.shape[0]
        gc = np.ascontiguousarray(np.transpose(g, (0, 2, 1)), dtype=np.float32).reshape(B, 16)  # column-major per lane
        T = np.empty((B, 16), dtype=np.float32)
        H = np.empty((B, 36), dtype=np.float64)
        conv = np.zeros(B, dtype=np.int32)
        nit = np.zeros(B, dtype=np.int32)
        self._ck(entry(self._h, B, _p(gc, c_f32p) if B else None, _p(T, c_f32p) if B else None,
                       _p(conv, c_i32p) if B else None, _p(nit, c_i32p) if B else None, _p(H, c_f64p) if B else None))
        return (np.ascontiguousarray(np.transpose(T.reshape(B, 4, 4), (0, 2, 1))), conv.astype(bool), nit,
                np.ascontiguousarray(np.transpose(H.reshape(B, 6, 6), (0, 2, 1))))

    def fitnessBatch(self, Ts, max_range: float = sys.float_info.max):
        """fitness() for every transform of Ts (B, 4, 4) in one launch -> (scores (B,) float64, n_inliers (B,) int64), bit for bit
        what B calls of fitness(max_range, T) give."""
        t = np.asarray(Ts)
        if t.ndim != 3 or t.shape[1:] != (4, 4):
            raise NgicpError(-2, "fitnessBatch: Ts must be (B, 4, 4)")
        B = t.shape[0]
        tc = np.ascontiguousarray(np.transpose(t, (0, 2, 1)), dtype=np.float32).reshape(B, 16)
        scores = np.empty(B, dtype=np.float64)
        cnt = np.zeros(B, dtype=np.uint64)
        self._ck(self._L.ngicp_fitness_score_batch(self._h, B, _p(tc, c_f32p) if B else None, float(max_range), _p(scores, c_f64p) if B else None,
                                                   cnt.ctypes.data_as(C.POINTER(C.c_size_t))))
        return scores, cnt.astype(np.int64)

    # ---- voxel fitness (include/ngicp.h "voxel fitness"): poses scored against the voxel map this handle aligns against ----
    _VFIT_DTYPE = np.dtype([("mahalanobis", np.float64), ("sqdist", np.float64), ("n_inliers", np.uint64), ("n_matched", np.uint64)])

    def voxelFitness(self, max_mahalanobis: float = sys.float_info.max, T=None) -> dict:
        """-> {"mahalanobis", "sqdist", "n_inliers", "n_matched"} of the pose T (None: the last align's final transformation) against the
        voxel map in force - the target's, the merged one or the rolling one; no target cloud is needed on a rolling map.  Per source
        point the best slot's e^T (cov_v + R C_a R^T)^-1 e (no n_v factor) and squared distance to the voxel mean; a point is an inlier
        iff that term is <= max_mahalanobis; the two scores are means over the inliers (DBL_MAX without any); n_matched / n_src is the
        overlap."""
        t = None if T is None else _colmajor16(T, np.float32)
        r = VoxelFitness()
        self._ck(self._L.ngicp_voxel_fitness(self._h, None if t is None else _p(t, c_f32p), float(max_mahalanobis), C.byref(r)))
        return {"mahalanobis": r.mahalanobis, "sqdist": r.sqdist, "n_inliers": int(r.n_inliers), "n_matched": int(r.n_matched)}

    def voxelFitnessBatch(self, Ts, max_mahalanobis: float = sys.float_info.max):
        """voxelFitness() for every pose of Ts (B, 4, 4), B poses per launch -> (mahalanobis (B,) float64, sqdist (B,) float64,
        n_inliers (B,) int64, n_matched (B,) int64), bit for bit what B calls of voxelFitness(max_mahalanobis, T) give."""
        t = np.asarray(Ts)
        if t.ndim != 3 or t.shape[1:] != (4, 4):
            raise NgicpError(-2, "voxelFitnessBatch: Ts must be (B, 4, 4)")
        B = t.shape[0]
        tc = np.ascontiguousarray(np.transpose(t, (0, 2, 1)), dtype=np.float32).reshape(B, 16)
        out = np.zeros(B, dtype=self._VFIT_DTYPE)
        self._ck(self._L.ngicp_voxel_fitness_batch(self._h, B, _p(tc, c_f32p) if B else None, float(max_mahalanobis),
                                                   out.ctypes.data_as(C.POINTER(VoxelFitness)) if B else None))
        return (out["mahalanobis"].copy(), out["sqdist"].copy(), out["n_inliers"].astype(np.int64), out["n_matched"].astype(np.int64))

    def voxel_fitness_points(self, T=None):
        """-> (m (n,) float64, sqd (n,) float64, voxel (n,) int32) in original source order: every point's value at the pose T (None: the
        final transformation) - the winning slot's term, squared distance and voxel number; -1 / -1 / -1 where the map has no voxel for
        the point (unmatched), +inf / +inf / -1 where it has one but no term is finite."""
        t = None if T is None else _colmajor16(T, np.float32)
        n = 0 if self._src is None else self._src.shape[0]  # (no source: the engine says so)
        m = np.empty(max(n, 1)); d = np.empty(max(n, 1)); v = np.empty(max(n, 1), dtype=np.int32)
        self._ck(self._L.ngicp_voxel_fitness_points(self._h, None if t is None else _p(t, c_f32p), _p(m, c_f64p), _p(d, c_f64p), _p(v, c_i32p), n))
        return m[:n], d[:n], v[:n]

    def voxelFitnessKernelMs(self) -> float:
        """device time of the kernels of the last voxelFitness / voxelFitnessBatch / voxel_fitness_points call (stats() is left alone)"""
        ms = C.c_double(0)
        self._ck(self._L.ngicp_voxel_fitness_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    # ---- scan context (include/ngicp.h "scan context"): which earlier keyframe a scan revisits, and at what yaw ----
    SCAN_CONTEXT_MAX_TOP_K = 64

    def _sc_which(self, which) -> int:
        """a slot as a number (0 source, 1 target, 2 the preprocessed scan) or by rangeSelect's names"""
        if isinstance(which, str):
            return self._range_which(which)
        if isinstance(which, (int, np.integer)) and not isinstance(which, bool):
            return int(which)  # (a number outside 0..2: the engine says so)
        raise NgicpError(-2, f"which must be a slot number or one of {sorted(self._RANGE_WHICH)}, not {which!r}")

    def _sc_query(self, query):
        """-> (which, descriptor pointer or None, the array kept alive): a slot number / name, or an (R, S) descriptor"""
        if isinstance(query, (str, int, np.integer)) and not isinstance(query, bool):
            return self._sc_which(query), None, None
        R, S, _, _ = self.getScanContextParams()
        d = np.ascontiguousarray(query, dtype=np.float32)
        if d.shape != (R, S):
            raise NgicpError(-2, f"a scan context descriptor must be ({R}, {S}), not {d.shape}")
        return -1, _p(d, c_f32p), d

    def setScanContextParams(self, n_rings: int = 20, n_sectors: int = 60, max_radius: float = 80.0, z_offset: float = 2.0):
        """rings 1..64, sectors even 2..64, max_radius > 0, z_offset finite.  A change clears the descriptor database."""
        self._ck(self._L.ngicp_scan_context_set_params(self._h, int(n_rings), int(n_sectors), float(max_radius), float(z_offset)))

    def getScanContextParams(self):
        """-> (n_rings, n_sectors, max_radius, z_offset)"""
        R, S, L, z0 = C.c_int(0), C.c_int(0), C.c_float(0), C.c_float(0)
        self._ck(self._L.ngicp_scan_context_get_params(self._h, C.byref(R), C.byref(S), C.byref(L), C.byref(z0)))
        return R.value, S.value, np.float32(L.value), np.float32(z0.value)

    def scanContextTables(self):
        """-> (E2 (R + 1,) float32: the squared ring edges; b (S / 2, 2) float32: the sector boundary directions) as the engine uses them"""
        R, S, _, _ = self.getScanContextParams()
        E2 = np.empty(R + 1, dtype=np.float32); b = np.empty(S, dtype=np.float32)
        self._ck(self._L.ngicp_scan_context_tables(self._h, _p(E2, c_f32p), _p(b, c_f32p)))
        return E2, b.reshape(S // 2, 2)

    def computeScanContext(self, which=0) -> np.ndarray:
        """-> the (R, S) float32 descriptor of a slot's cloud (0 source, 1 target, 2 the preprocessed scan), built on the device"""
        R, S, _, _ = self.getScanContextParams()
        d = np.empty((R, S), dtype=np.float32)
        self._ck(self._L.ngicp_scan_context_compute(self._h, self._sc_which(which), _p(d, c_f32p)))
        return d

    def addScanContext(self, which=0) -> int:
        """append the descriptor of a slot's cloud to the database without leaving the device -> its id (dense, in insertion order)"""
        i = C.c_int(-1)
        self._ck(self._L.ngicp_scan_context_add(self._h, self._sc_which(which), C.byref(i)))
        return i.value

    def addScanContextDescriptor(self, desc) -> int:
        """append a host descriptor (R, S), finite and >= 0 -> its id"""
        _, p, keep = self._sc_query(np.asarray(desc))
        i = C.c_int(-1)
        self._ck(self._L.ngicp_scan_context_add_descriptor(self._h, p, C.byref(i)))
        return i.value

    def numScanContexts(self) -> int:
        n = C.c_size_t(0)
        self._ck(self._L.ngicp_scan_context_count(self._h, C.byref(n)))
        return n.value

    def scanContext(self, id: int) -> np.ndarray:
        R, S, _, _ = self.getScanContextParams()
        d = np.empty((R, S), dtype=np.float32)
        self._ck(self._L.ngicp_scan_context_get(self._h, int(id), _p(d, c_f32p)))
        return d

    def clearScanContexts(self):
        self._ck(self._L.ngicp_scan_context_clear(self._h))

    def _sc_range(self, begin, end):
        end = self.numScanContexts() if end is None else int(end)
        begin = int(begin)
        if begin < 0 or end < 0:
            raise NgicpError(-2, "a scan context id range must not be negative")
        return begin, end

    def scanContextDistances(self, query, begin: int = 0, end=None):
        """-> (dist (n,) float64, shift (n,) int32) of the query - a slot number or an (R, S) descriptor - to the entries [begin, end) (end
        None: every entry from begin), each the minimum over all S column shifts and the smallest shift that attains it."""
        which, p, keep = self._sc_query(query)
        begin, end = self._sc_range(begin, end)
        n = max(end - begin, 0)
        dist = np.empty(max(n, 1)); shift = np.empty(max(n, 1), dtype=np.int32)
        self._ck(self._L.ngicp_scan_context_distances(self._h, which, p, begin, end, _p(dist, c_f64p), _p(shift, c_i32p)))
        return dist[:n], shift[:n]

    def matchScanContext(self, query, begin: int = 0, end=None, top_k: int = 1):
        """-> (ids (m,) int32, dist (m,) float64, shift (m,) int32): the first m = min(top_k, end - begin) entries of [begin, end) in
        ascending (distance, id) order, selected on the device.  top_k 1..64."""
        which, p, keep = self._sc_query(query)
        begin, end = self._sc_range(begin, end)
        k = int(top_k)
        cap = min(max(k, 1), self.SCAN_CONTEXT_MAX_TOP_K)
        ids = np.empty(cap, dtype=np.int32); dist = np.empty(cap); shift = np.empty(cap, dtype=np.int32)
        m = C.c_size_t(0)
        self._ck(self._L.ngicp_scan_context_match(self._h, which, p, begin, end, k, _p(ids, c_i32p), _p(dist, c_f64p), _p(shift, c_i32p), C.byref(m)))
        return ids[:m.value].copy(), dist[:m.value].copy(), shift[:m.value].copy()

    def scanContextGuess(self, shift: int) -> np.ndarray:
        """-> the 4x4 float32 rotation about z by shift * 2 pi / n_sectors: the guess that carries the query scan into the matched entry's
        frame when both were taken at about the same place (for align / alignBatch)."""
        _, S, _, _ = self.getScanContextParams()
        a = float(shift) * (2.0 * np.pi / S)
        T = np.eye(4, dtype=np.float32)
        T[0, 0] = T[1, 1] = np.float32(np.cos(a))
        T[1, 0] = np.float32(np.sin(a))
        T[0, 1] = -T[1, 0]
        return T

    def scanContextKernelMs(self) -> float:
        """device time of the kernels of the last scan context call (stats() is left alone)"""
        ms = C.c_double(0)
        self._ck(self._L.ngicp_scan_context_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    # ---- voxel pose search (include/ngicp.h "voxel pose search"): the translation, and the best of several orientations, on the voxel map ----
    POSE_SEARCH_MAX_TOP_K = 64

    @staticmethod
    def yawLattice(T0, n: int, step_rad: float) -> np.ndarray:
        """-> (n, 4, 4) float32: T0 . Rz(k * step_rad), k = 0..n-1, the product taken in float64 and rounded once.  Base poses for
        voxelPoseSearch; they are INPUT to the engine and to any host restatement alike, so how this helper rounds shows in no result."""
        T0 = np.asarray(T0, np.float64)
        if T0.shape != (4, 4):
            raise NgicpError(-2, "yawLattice: T0 must be (4, 4)")
        out = np.empty((max(int(n), 0), 4, 4), dtype=np.float32)
        for k in range(out.shape[0]):
            a = k * float(step_rad)
            Rz = np.eye(4)
            Rz[0, 0] = Rz[1, 1] = np.cos(a)
            Rz[1, 0] = np.sin(a)
            Rz[0, 1] = -Rz[1, 0]
            out[k] = (T0 @ Rz).astype(np.float32)
        return out

    @staticmethod
    def poseSearchCandidate(T, shift, res: float) -> np.ndarray:
        """-> the 4x4 float32 candidate pose of a base pose T and a shift (sx, sy, sz) in voxels: T with its translation replaced, per
        axis, by (float)((double)t + (double)s * res)."""
        out = np.array(T, dtype=np.float32)
        t = out[:3, 3].astype(np.float64) + np.asarray(shift, np.float64) * np.float64(res)
        out[:3, 3] = t.astype(np.float32)
        return out

    def voxelPoseSearch(self, Ts, extent, top_k: int = 8):
        """Score every pose of the lattice {Ts[b] shifted by (sx, sy, sz) voxels, |s| <= extent = (ex, ey, ez)} by the number of source
        points that land in occupied voxels of the map in force, and return the first m = min(top_k, B |S|) of the ranking (descending
        score, then ascending pose, then ascending shift index) -> (pose (m,) int32, shift (m, 3) int32, score (m,) int32,
        T (m, 4, 4) float32: the candidate poses, for alignBatchVoxel).  The score is defined on cells (include/ngicp.h): the float
        candidate pose may put a point near a cell border into another cell.  ex, ey <= 31, ez <= 7, |S| <= 12288, B |S| <= 2^24."""
        t = np.asarray(Ts)
        if t.ndim != 3 or t.shape[1:] != (4, 4):
            raise NgicpError(-2, "voxelPoseSearch: Ts must be (B, 4, 4)")
        ext = tuple(int(v) for v in extent)
        if len(ext) != 3:
            raise NgicpError(-2, "voxelPoseSearch: extent must be (ex, ey, ez)")
        B = t.shape[0]
        tf = np.ascontiguousarray(t, dtype=np.float32)
        tc = np.ascontiguousarray(np.transpose(tf, (0, 2, 1))).reshape(B, 16)
        k = int(top_k)
        cap = min(max(k, 1), self.POSE_SEARCH_MAX_TOP_K)
        pose = np.empty(cap, dtype=np.int32); shift = np.empty((cap, 3), dtype=np.int32); score = np.empty(cap, dtype=np.int32)
        m = C.c_size_t(0)
        self._ck(self._L.ngicp_voxel_pose_search(self._h, B, _p(tc, c_f32p) if B else None, ext[0], ext[1], ext[2], k, _p(pose, c_i32p), _p(shift, c_i32p),
                                                 _p(score, c_i32p), C.byref(m)))
        self._ps_shape = (B, 2 * ext[2] + 1, 2 * ext[1] + 1, 2 * ext[0] + 1)
        n = m.value
        res = self.getVoxelResolution()
        cand = np.empty((n, 4, 4), dtype=np.float32)
        for i in range(n):
            cand[i] = self.poseSearchCandidate(tf[pose[i]], shift[i], res)
        return pose[:n].copy(), shift[:n].copy(), score[:n].copy(), cand

    def voxelPoseSearchScores(self) -> np.ndarray:
        """-> the full score volume of the last voxelPoseSearch, (B, 2 ez + 1, 2 ey + 1, 2 ex + 1) int32; refused (NGICP_ERR_STATE) when
        there has been no search or the map has changed since"""
        shape = getattr(self, "_ps_shape", (1, 1, 1, 1))
        out = np.empty(shape, dtype=np.int32)
        self._ck(self._L.ngicp_voxel_pose_search_scores(self._h, _p(out, c_i32p), out.size))
        return out

    def voxelPoseSearchKernelMs(self) -> float:
        """device time of the kernels of the last voxelPoseSearch (stats() is left alone)"""
        ms = C.c_double(0)
        self._ck(self._L.ngicp_voxel_pose_search_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def getFinalTransformation(self): return self.final_transformation_
    def hasConverged(self) -> bool: return self.converged_
    def getFinalHessian(self): return self.final_hessian_

    # ---- parity hooks ----
    def linearize(self, T):
        t = _colmajor16(T, np.float64)
        H = np.empty(36); b = np.empty(6); e = C.c_double(0)
        self._ck(self._L.ngicp_linearize(self._h, _p(t, c_f64p), _p(H, c_f64p), _p(b, c_f64p), C.byref(e)))
        return H.reshape(6, 6).T.copy(), b, e.value

    def compute_error(self, T) -> float:
        t = _colmajor16(T, np.float64)
        e = C.c_double(0)
        self._ck(self._L.ngicp_compute_error(self._h, _p(t, c_f64p), C.byref(e)))
        return e.value

    def correspondences(self):
        n = self._src.shape[0]
        corr = np.empty(n, dtype=np.int32); sqd = np.empty(n, dtype=np.float32)
        self._ck(self._L.ngicp_get_correspondences(self._h, _p(corr, c_i32p), _p(sqd, c_f32p)))
        return corr, sqd

    def target_knn(self, queries, k: int):
        q = _cloud(queries)
        idx = np.empty((q.shape[0], k), dtype=np.int32); d2 = np.empty((q.shape[0], k), dtype=np.float32)
        self._ck(self._L.ngicp_target_knn(self._h, _p(q, c_f32p), q.shape[0], q.strides[0], k, _p(idx, c_i32p), _p(d2, c_f32p)))
        return idx, d2

    # ---- the search surface of the reference's trees and of pcl::Registration (include/ngicp.h "queries") ----
    _WHICH = {"source": 0, "target": 1}

    def fitness(self, max_range: float = sys.float_info.max, T=None):
        """-> (score, n_inliers): pcl::Registration::getFitnessScore(max_range) over the source transformed by T (None: the last
        align's final_transformation_, identity before any).  max_range is a SQUARED distance; score is DBL_MAX when no point counts."""
        t = None if T is None else _colmajor16(T, np.float32)
        score, n = C.c_double(0), C.c_size_t(0)
        self._ck(self._L.ngicp_fitness_score(self._h, None if t is None else _p(t, c_f32p), float(max_range), C.byref(score), C.byref(n)))
        return score.value, n.value

    def getFitnessScore(self, max_range: float = sys.float_info.max, T=None) -> float:
        return self.fitness(max_range, T)[0]

    def nearestKSearch(self, queries, k: int, which: str = "target"):
        """source_kdtree_ / target_kdtree_ ->nearestKSearch for every row of `queries`: (idx (nq, k), d2 (nq, k)), ascending."""
        q = _cloud(queries)
        idx = np.empty((q.shape[0], k), dtype=np.int32); d2 = np.empty((q.shape[0], k), dtype=np.float32)
        self._ck(self._L.ngicp_knn_search(self._h, self._WHICH[which], _p(q, c_f32p), q.shape[0], q.strides[0], k, _p(idx, c_i32p), _p(d2, c_f32p)))
        return idx, d2

    def radiusSearch(self, queries, radius: float, which: str = "target"):
        """->radiusSearch for every row of `queries`: (offsets (nq + 1,), idx, d2); query i's hits are [offsets[i], offsets[i+1]),
        d2 < float(radius) (radius is a SQUARED distance), in ascending (d2, index) order."""
        q = _cloud(queries)
        nq = q.shape[0]
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        total = C.c_size_t(0)
        self._ck(self._L.ngicp_radius_search(self._h, self._WHICH[which], _p(q, c_f32p), nq, q.strides[0], float(radius),
                                             offsets.ctypes.data_as(C.POINTER(C.c_size_t)), C.byref(total)))
        idx = np.empty(total.value, dtype=np.int32); d2 = np.empty(total.value, dtype=np.float32)
        self._ck(self._L.ngicp_radius_fetch(self._h, _p(idx, c_i32p), _p(d2, c_f32p), total.value))
        return offsets.astype(np.int64), idx, d2

    # ---- range select: DLO's spaciousness median without downloading the scan (include/ngicp.h "range select") ----
    _RANGE_WHICH = {"source": 0, "target": 1, "preprocessed": 2}

    def _range_which(self, which) -> int:
        if which not in self._RANGE_WHICH:
            raise NgicpError(-2, f"which must be one of {sorted(self._RANGE_WHICH)}, not {which!r}")
        return self._RANGE_WHICH[which]

    def rangeSelect(self, rank: int, which: str = "source") -> np.float32:
        """The range (float)sqrt((double)x*x + y*y + z*z) of 0-based rank `rank` among the cloud's ranges in ascending order, NaN after
        +inf.  which: "source" | "target" | "preprocessed" (the scan preprocessScan left on the device)."""
        w = self._range_which(which)
        if rank < 0:
            raise NgicpError(-2, "rank must not be negative")
        v = C.c_float(0)
        self._ck(self._L.ngicp_range_select(self._h, w, int(rank), C.byref(v), None))
        return np.float32(v.value)

    def medianRange(self, which: str = "source") -> np.float32:
        """rangeSelect(n // 2): the median_curr of computeSpaciousness (odom.cc:1000-1002)."""
        v = C.c_float(0)
        self._ck(self._L.ngicp_range_median(self._h, self._range_which(which), C.byref(v), None))
        return np.float32(v.value)

    def lm_trace(self, lane=None) -> np.ndarray:
        """LM trace of the last align() (lane None), or of lane `lane` of the last alignBatch() / alignBatchVoxel()."""
        n = C.c_size_t(0)
        if lane is not None:
            self._ck(self._L.ngicp_batch_get_lm_trace(self._h, int(lane), None, 0, C.byref(n)))
            out = np.empty((n.value, 8))
            if n.value:
                self._ck(self._L.ngicp_batch_get_lm_trace(self._h, int(lane), _p(out, c_f64p), n.value, C.byref(n)))
            return out
        self._ck(self._L.ngicp_get_lm_trace(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 8))
        if n.value:
            self._ck(self._L.ngicp_get_lm_trace(self._h, _p(out, c_f64p), n.value, C.byref(n)))
        return out

    def setProfiling(self, on):
        """False/0: off; True/1: HIP events around every pass launch; N > 1: around every N-th launch."""
        self._ck(self._L.ngicp_set_profiling(self._h, int(on)))

    def stats(self) -> dict:
        s = Stats()
        self._ck(self._L.ngicp_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    # ---- device-resident keyframes + submap (replaces odom.cc:1174 and :830-833) ----
    def addKeyframe(self, producer: "NanoGICP") -> int:
        kid = C.c_int(-1)
        self._ck(self._L.ngicp_keyframe_add(self._h, producer._h, C.byref(kid)))
        return kid.value

    def addKeyframeTransformed(self, producer: "NanoGICP", T) -> int:
        kid = C.c_int(-1)
        t = _colmajor16(T, np.float32)
        self._ck(self._L.ngicp_keyframe_add_transformed(self._h, producer._h, _p(t, c_f32p), C.byref(kid)))
        return kid.value

    def addKeyframeTransformedFiltered(self, producer: "NanoGICP", T, leaf: float) -> int:
        """DLO's shipped configuration (voxelFilter.submap.use, cfg/params.yaml:33-35): odom.cc:971-974 + 1160-1174 on the device."""
        t = _colmajor16(T, np.float32); kid = C.c_int(-1)
        self._ck(self._L.ngicp_keyframe_add_transformed_filtered(self._h, producer._h, _p(t, c_f32p), float(leaf), C.byref(kid)))
        return kid.value

    def numKeyframes(self) -> int: return self._covs_size("ngicp_keyframe_count")

    def keyframeSize(self, kid: int) -> int:
        n = C.c_size_t(0)
        self._ck(self._L.ngicp_keyframe_size(self._h, int(kid), C.byref(n)))
        return n.value

    def clearKeyframes(self): self._ck(self._L.ngicp_keyframe_clear(self._h))

    # ---- moving keyframes after a loop closure (include/ngicp.h "moving keyframes") ----
    def getKeyframe(self, kid: int):
        """-> (points (n, 3) float32, covs (n, 4, 4)) of keyframe `kid`, both in its ORIGINAL point order."""
        n = C.c_size_t(0)
        self._ck(self._L.ngicp_keyframe_get(self._h, int(kid), None, 0, None, C.byref(n)))
        pts = np.empty((n.value, 3), dtype=np.float32)
        c16 = np.empty((n.value, 16), dtype=np.float64)
        if n.value:
            self._ck(self._L.ngicp_keyframe_get(self._h, int(kid), _p(pts, c_f32p), 12, _p(c16, c_f64p), C.byref(n)))
        return pts, c16.reshape(n.value, 4, 4).transpose(0, 2, 1).copy()

    def transformKeyframes(self, ids, Ts) -> bool:
        """Keyframe ids[j] := Ts[j] applied to it (points by the float matrix as pcl::transformPointCloud, covariances rotated by its 3x3
        block, nothing recomputed), for all j in one launch on the device; all or nothing.  The current target is left as it is.  True
        when a moved keyframe belongs to the submap that is the target: the next setSubmapKeyframes rebuilds it, even with the same list."""
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        t = np.asarray(Ts, dtype=np.float32)
        if t.ndim != 3 or t.shape[1:] != (4, 4) or t.shape[0] != a.shape[0]:
            raise ValueError("Ts must have shape (len(ids), 4, 4)")
        t = np.ascontiguousarray(t.transpose(0, 2, 1)).reshape(-1)  # column-major, one matrix after the other
        stale = C.c_int(0)
        self._ck(self._L.ngicp_keyframe_transform(self._h, _p(a, c_i32p), a.shape[0], _p(t, c_f32p), C.byref(stale)))
        return bool(stale.value)

    def keyframeTransformKernelMs(self) -> float:
        ms = C.c_double(0.0)
        self._ck(self._L.ngicp_keyframe_transform_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    # ---- pose graph (include/ngicp.h "pose graph") ----
    @staticmethod
    def _poses16(T) -> np.ndarray:
        """(n, 4, 4) or (4, 4) row-major as numpy holds them -> n x 16 column-major doubles"""
        t = np.asarray(T, dtype=np.float64)
        if t.ndim == 2:
            t = t[None]
        if t.ndim != 3 or t.shape[1:] != (4, 4):
            raise ValueError("poses must have shape (n, 4, 4)")
        return np.ascontiguousarray(t.transpose(0, 2, 1)).reshape(-1)

    def poseGraphClear(self): self._ck(self._L.ngicp_pose_graph_clear(self._h))

    def poseGraphSize(self):
        """-> (nodes, edges)"""
        n, m = C.c_size_t(0), C.c_size_t(0)
        self._ck(self._L.ngicp_pose_graph_size(self._h, C.byref(n), C.byref(m)))
        return n.value, m.value

    def poseGraphAddNodes(self, T, fixed=None) -> int:
        """Append nodes at the world poses T (n, 4, 4); fixed: a flag per node (default: none).  -> the first new id.  All or nothing."""
        t = self._poses16(T)
        n = t.shape[0] // 16
        f = None if fixed is None else np.ascontiguousarray(np.broadcast_to(np.asarray(fixed, dtype=bool), (n,)), dtype=np.uint8)
        first = C.c_int(-1)
        self._ck(self._L.ngicp_pose_graph_add_nodes(self._h, _p(t, c_f64p), None if f is None else _p(f, C.POINTER(C.c_ubyte)), n, C.byref(first)))
        return first.value

    def poseGraphAddEdges(self, ij, Z, info, robust=None) -> int:
        """Append edges (i, j) with measurements Z (n, 4, 4) = T_i^-1 T_j and information matrices (n, 6, 6), exactly symmetric, rotation
        first; robust: a flag per edge (default: none).  -> the first new edge id.  All or nothing."""
        a = np.ascontiguousarray(ij, dtype=np.int32).reshape(-1, 2)
        z = self._poses16(Z)
        L = np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 36)
        n = a.shape[0]
        if z.shape[0] != 16 * n or L.shape[0] != n:
            raise ValueError("one Z and one information matrix per edge")
        f = None if robust is None else np.ascontiguousarray(np.broadcast_to(np.asarray(robust, dtype=bool), (n,)), dtype=np.uint8)
        first = C.c_int(-1)
        self._ck(self._L.ngicp_pose_graph_add_edges(self._h, _p(a, c_i32p), _p(z, c_f64p), _p(L, c_f64p), None if f is None else _p(f, C.POINTER(C.c_ubyte)), n,
                                                    C.byref(first)))
        return first.value

    def poseGraphEdges(self):
        """-> (ij (m, 2), Z (m, 4, 4), info (m, 6, 6), robust flags (m,)) as the graph holds them"""
        _, m = self.poseGraphSize()
        ij, z, L, f = np.zeros((m, 2), np.int32), np.zeros((m, 16)), np.zeros((m, 6, 6)), np.zeros(m, np.uint8)
        if m:
            self._ck(self._L.ngicp_pose_graph_get_edges(self._h, 0, m, _p(ij, c_i32p), _p(z, c_f64p), _p(L, c_f64p), _p(f, C.POINTER(C.c_ubyte))))
        return ij, z.reshape(m, 4, 4).transpose(0, 2, 1).copy(), L, f.astype(bool)

    def poseGraphSetFixed(self, ids, flags):
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        f = np.ascontiguousarray(np.broadcast_to(np.asarray(flags, dtype=bool), a.shape), dtype=np.uint8)
        self._ck(self._L.ngicp_pose_graph_set_fixed(self._h, _p(a, c_i32p), _p(f, C.POINTER(C.c_ubyte)), a.shape[0]))

    def poseGraphFixed(self) -> np.ndarray:
        n, _ = self.poseGraphSize()
        f = np.zeros(n, np.uint8)
        if n:
            self._ck(self._L.ngicp_pose_graph_get_fixed(self._h, 0, n, _p(f, C.POINTER(C.c_ubyte))))
        return f.astype(bool)

    def poseGraphSetRobust(self, kind: int, width: float = 1.0):
        """The kernel of the FLAGGED edges: ROBUST_NONE / HUBER / CAUCHY / GEMAN_MCCLURE with a width (in the residual's whitened units)."""
        self._ck(self._L.ngicp_pose_graph_set_robust(self._h, int(kind), float(width)))

    def poseGraphPoses(self, first: int = 0, n: int = None) -> np.ndarray:
        """-> (n, 4, 4) float64 poses of the nodes first .. first + n (default: all)"""
        if n is None:
            n = self.poseGraphSize()[0] - first
        out = np.zeros((n, 16))
        if n:
            self._ck(self._L.ngicp_pose_graph_get_poses(self._h, int(first), n, _p(out, c_f64p)))
        return out.reshape(n, 4, 4).transpose(0, 2, 1).copy()

    def poseGraphSetPoses(self, first: int, T):
        t = self._poses16(T)
        self._ck(self._L.ngicp_pose_graph_set_poses(self._h, int(first), t.shape[0] // 16, _p(t, c_f64p)))

    def poseGraphLinearize(self) -> dict:
        """Test hook: the linearisation at the current poses, which stay.  -> dict(chi2, r (m, 6), s (m,), w (m,), grad (n, 6), diag (n, 6, 6));
        gradient and diagonal blocks of fixed nodes are zero."""
        n, m = self.poseGraphSize()
        chi2 = C.c_double(0.0)
        r, sw, grad, diag = np.zeros((m, 6)), np.zeros((m, 2)), np.zeros((n, 6)), np.zeros((n, 6, 6))
        self._ck(self._L.ngicp_pose_graph_linearize(self._h, C.byref(chi2), _p(r, c_f64p), _p(sw, c_f64p), _p(grad, c_f64p), _p(diag, c_f64p)))
        return dict(chi2=chi2.value, r=r, s=sw[:, 0].copy(), w=sw[:, 1].copy(), grad=grad, diag=diag)

    def poseGraphMultiply(self, lam: float, x) -> np.ndarray:
        """Test hook: (H + lam I) x at the current poses' linearisation, (n, 6); rows of fixed nodes are zero."""
        n, _ = self.poseGraphSize()
        xa = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if xa.shape[0] != 6 * n:
            raise ValueError("x must have 6 entries per node")
        y = np.zeros((n, 6))
        self._ck(self._L.ngicp_pose_graph_multiply(self._h, float(lam), _p(xa, c_f64p), _p(y, c_f64p)))
        return y

    def poseGraphOptimize(self, **options) -> dict:
        """Levenberg-Marquardt on the whole graph, on the device.  Options: max_iterations, rot_eps, trans_eps, cg_tol, cg_max_iterations
        (PG_DEFAULTS).  -> dict(initial_chi2, final_chi2, iterations, accepted, cg_iterations, converged, trace (tries, 5): chi2 of the
        try, lambda, gain ratio, CG iterations, accepted)."""
        unknown = set(options) - set(PG_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown options {sorted(unknown)}")
        o = dict(PG_DEFAULTS)
        o.update(options)
        opt = PgOptions(int(o["max_iterations"]), float(o["rot_eps"]), float(o["trans_eps"]), float(o["cg_tol"]), int(o["cg_max_iterations"]))
        res = PgResult()
        self._ck(self._L.ngicp_pose_graph_optimize(self._h, C.byref(opt), C.byref(res)))
        trace = np.array(res.trace[:res.n_trace * 5], dtype=np.float64).reshape(res.n_trace, 5)
        return dict(initial_chi2=res.initial_chi2, final_chi2=res.final_chi2, iterations=res.iterations, accepted=res.accepted,
                    cg_iterations=int(res.cg_iterations), converged=bool(res.converged), trace=trace)

    def poseGraphCorrections(self, ids, T_old=None) -> np.ndarray:
        """-> (len(ids), 4, 4) float32: C_k = T_k * T_k_old^-1, what transformKeyframes / transformVoxelMap take.  T_old: (len(ids), 4, 4),
        or None for the poses the last poseGraphOptimize started from."""
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        old = None if T_old is None else self._poses16(T_old)
        if old is not None and old.shape[0] != 16 * a.shape[0]:
            raise ValueError("one T_old per id")
        out = np.zeros((a.shape[0], 16), np.float32)
        self._ck(self._L.ngicp_pose_graph_corrections(self._h, _p(a, c_i32p), a.shape[0], None if old is None else _p(old, c_f64p), _p(out, c_f32p)))
        return out.reshape(-1, 4, 4).transpose(0, 2, 1).copy()

    def poseGraphKernelMs(self) -> float:
        ms = C.c_double(0.0)
        self._ck(self._L.ngicp_pose_graph_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    @staticmethod
    def edgeFromAlignment(T_i, T_aligned, H):
        """The edge an alignment yields: scan j aligned against keyframe i, which is held in the world frame at T_i, ended at the world pose
        T_aligned with getFinalHessian() = H (in the aligner's left perturbation of the world pose).  -> (Z, Lambda): Z = T_i^-1 T_aligned and
        Lambda = J^-T H J^-1, H in the edge's residual coordinates (r = J d at the measurement, J = [[A, 0], [-A [t]x, A]] with A = R_aligned^T,
        t = t_aligned), symmetrised exactly."""
        Ti, Ta, Hm = np.asarray(T_i, np.float64), np.asarray(T_aligned, np.float64), np.asarray(H, np.float64)
        Ri, ti = Ti[:3, :3], Ti[:3, 3]
        Z = np.eye(4)
        Z[:3, :3] = Ri.T @ Ta[:3, :3]
        Z[:3, 3] = Ri.T @ (Ta[:3, 3] - ti)
        At, t = Ta[:3, :3], Ta[:3, 3]
        S = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
        Jinv = np.zeros((6, 6))
        Jinv[:3, :3], Jinv[3:, :3], Jinv[3:, 3:] = At, S @ At, At
        Lam = Jinv.T @ Hm @ Jinv
        return Z, 0.5 * (Lam + Lam.T)

    def setSubmapKeyframes(self, ids) -> bool:
        """target := concatenation of the keyframes `ids` (cloud + covariances), on the device.  True when rebuilt."""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        changed = C.c_int(0)
        self._ck(self._L.ngicp_submap_set(self._h, _p(a, c_i32p), a.shape[0], C.byref(changed)))
        self._tgt = None
        return bool(changed.value)

    def targetPoints(self) -> np.ndarray:
        """The target cloud as the engine holds it (original point order; for a device submap: the concatenation)."""
        n = C.c_size_t(0)
        self._ck(self._L.ngicp_get_target_points(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 3), dtype=np.float32)
        if n.value:
            self._ck(self._L.ngicp_get_target_points(self._h, _p(out, c_f32p), 12, C.byref(n)))
        return out

    # ---- rigid transform of clouds (pcl::transformPointCloud with a float matrix) ----
    def transformSource(self, T) -> np.ndarray:
        if self._src is None:
            raise NgicpError(-3, "no source cloud")
        t = _colmajor16(T, np.float32)
        out = np.empty((self._src.shape[0], 3), dtype=np.float32)
        self._ck(self._L.ngicp_transform_source(self._h, _p(t, c_f32p), _p(out, c_f32p), 12))
        return out

    def transformCloud(self, cloud, T) -> np.ndarray:
        c = _cloud(cloud)
        t = _colmajor16(T, np.float32)
        out = np.empty((c.shape[0], 3), dtype=np.float32)
        self._ck(self._L.ngicp_transform_cloud(self._h, _p(c, c_f32p), c.shape[0], c.strides[0], _p(t, c_f32p), _p(out, c_f32p), 12))
        return out

    # ---- scan preprocessing (src/dlo/odom.cc:443-465) and map voxel filter (§8f-4; src/dlo/map.cc:100-131) ----
    @staticmethod
    def _intensity_offset(c: np.ndarray, intensity_col) -> int:
        return -1 if intensity_col is None or intensity_col < 0 else int(intensity_col) * 4

    def preprocessScan(self, cloud, remove_nan: bool = True, crop_size: float = 0.0, voxel_res: float = 0.0, intensity_col=None,
                       set_as_source: bool = False) -> np.ndarray:
        """removeNaN -> CropBox(negative, +-crop_size) -> VoxelGrid(voxel_res); returns (M, 4) {x, y, z, intensity}.  With
        set_as_source the filtered cloud (still on the device) also becomes the source: setInputSource without an upload."""
        c = np.asarray(cloud, dtype=np.float32)
        if c.ndim != 2 or c.shape[1] < 3 or not c.flags.c_contiguous:
            c = np.ascontiguousarray(c, dtype=np.float32)
        out = np.empty((c.shape[0], 4), dtype=np.float32)
        m = C.c_size_t(0)
        self._ck(self._L.ngicp_preprocess_scan(self._h, _p(c, c_f32p), c.shape[0], c.strides[0], self._intensity_offset(c, intensity_col),
                                               1 if remove_nan else 0, float(crop_size), float(voxel_res), _p(out, c_f32p), out.shape[0], C.byref(m)))
        out = out[:m.value].copy()
        if set_as_source:
            self._ck(self._L.ngicp_set_source_preprocessed(self._h, 0))
            self._src = np.ascontiguousarray(out[:, :3])
        return out

    # ---- motion deskew (include/ngicp.h "motion deskew") ----
    @staticmethod
    def _deskew_desc(n, times, pose_times, poses, T_ref, time_format, time_offset):
        """ngicp_deskew_t and the arrays it points into (to be kept alive over the call).  `times`: an array of n times (float32 or
        float64 seconds, uint32 nanoseconds; any positive stride), or an int: the float32 column of the cloud's rows at which every
        record holds its time (byte offset 4 * column; time_format says what lies there, float32 seconds by default)."""
        d = Deskew()
        keep = []
        if isinstance(times, (int, np.integer)):
            d.times, d.time_stride_bytes, d.time_offset_bytes = None, 0, 4 * int(times)
            d.time_format = TIME_F32_S if time_format is None else int(time_format)
        else:
            t = np.asarray(times)
            if t.dtype not in _TIME_FORMAT_OF:
                t = t.astype(np.float64)
            if t.ndim != 1 or t.shape[0] != n:
                raise ValueError("times must be one time per point")
            if n > 1 and t.strides[0] <= 0:
                t = np.ascontiguousarray(t)
            keep.append(t)
            d.times, d.time_stride_bytes, d.time_offset_bytes = t.ctypes.data, (t.strides[0] if n > 1 else t.itemsize), 0
            d.time_format = _TIME_FORMAT_OF[t.dtype] if time_format is None else int(time_format)
        d.time_offset = float(time_offset)
        pt = np.ascontiguousarray(pose_times, dtype=np.float64).reshape(-1)
        ps = np.asarray(poses, dtype=np.float64)
        if ps.ndim != 3 or ps.shape[1:] != (4, 4) or ps.shape[0] != pt.shape[0]:
            raise ValueError("poses must have shape (len(pose_times), 4, 4)")
        ps = np.ascontiguousarray(ps.transpose(0, 2, 1)).reshape(-1)
        keep += [pt, ps]
        d.n_poses, d.pose_times, d.poses_colmajor = pt.shape[0], _p(pt, c_f64p), _p(ps, c_f64p)
        if T_ref is not None:
            tr = _colmajor16(T_ref, np.float64)
            keep.append(tr)
            d.T_ref_colmajor = _p(tr, c_f64p)
        return d, keep

    def deskewCloud(self, cloud, times, pose_times, poses, T_ref=None, time_format=None, time_offset: float = 0.0) -> np.ndarray:
        """Every point moved by the trajectory's pose at its own time into T_ref's frame (None: identity), on the GPU; returns (N, 3).
        poses: (M, 4, 4) at pose_times (M, strictly ascending), geodesic in rotation and linear in translation between them, clamped at
        both ends.  `times`: see _deskew_desc."""
        c = _cloud(cloud)
        d, keep = self._deskew_desc(c.shape[0], times, pose_times, poses, T_ref, time_format, time_offset)
        out = np.empty((c.shape[0], 3), dtype=np.float32)
        self._ck(self._L.ngicp_deskew_cloud(self._h, _p(c, c_f32p), c.shape[0], c.strides[0], C.byref(d), _p(out, c_f32p), 12))
        del keep
        return out

    def preprocessScanDeskewed(self, cloud, times, pose_times, poses, T_ref=None, time_format=None, time_offset: float = 0.0, remove_nan: bool = True,
                               crop_size: float = 0.0, voxel_res: float = 0.0, intensity_col=None, set_as_source: bool = False) -> np.ndarray:
        """preprocessScan with the deskew (deskewCloud's arguments) applied where the scan is unpacked on the device: the deskewed scan
        never exists on the host.  Returns (M, 4) {x, y, z, intensity}; set_as_source as in preprocessScan."""
        c = np.asarray(cloud, dtype=np.float32)
        if c.ndim != 2 or c.shape[1] < 3 or not c.flags.c_contiguous:
            c = np.ascontiguousarray(c, dtype=np.float32)
        d, keep = self._deskew_desc(c.shape[0], times, pose_times, poses, T_ref, time_format, time_offset)
        out = np.empty((c.shape[0], 4), dtype=np.float32)
        m = C.c_size_t(0)
        self._ck(self._L.ngicp_preprocess_scan_deskewed(self._h, _p(c, c_f32p), c.shape[0], c.strides[0], self._intensity_offset(c, intensity_col), C.byref(d),
                                                        1 if remove_nan else 0, float(crop_size), float(voxel_res), _p(out, c_f32p), out.shape[0], C.byref(m)))
        del keep
        out = out[:m.value].copy()
        if set_as_source:
            self._ck(self._L.ngicp_set_source_preprocessed(self._h, 0))
            self._src = np.ascontiguousarray(out[:, :3])
        return out

    def mapAdd(self, cloud, intensity_col=None):
        c = np.asarray(cloud, dtype=np.float32)
        if c.ndim != 2 or c.shape[1] < 3 or not c.flags.c_contiguous:
            c = np.ascontiguousarray(c, dtype=np.float32)
        self._ck(self._L.ngicp_map_add(self._h, _p(c, c_f32p), c.shape[0], c.strides[0], self._intensity_offset(c, intensity_col)))

    def mapVoxelFilter(self, leaf: float) -> int:
        m = C.c_size_t(0)
        self._ck(self._L.ngicp_map_voxel_filter(self._h, float(leaf), C.byref(m)))
        return m.value

    def mapSize(self) -> int: return self._covs_size("ngicp_map_size")

    def mapGet(self) -> np.ndarray:
        n = self.mapSize()
        out = np.empty((n, 4), dtype=np.float32)
        if n:
            self._ck(self._L.ngicp_map_get(self._h, _p(out, c_f32p), n))
        return out

    def mapClear(self): self._ck(self._L.ngicp_map_clear(self._h))

    def mathSelftest(self, which: int, problems) -> np.ndarray:
        """ngicp_math.h on the device (0 so3_exp, 1 ldlt6_solve, 2 eig3_sym, 3 inv3_sym, 4 so3_log, 5 prior_row), one problem per row."""
        a = np.ascontiguousarray(problems, dtype=np.float64)
        out = np.empty((a.shape[0], (9, 6, 12, 6, 3, 28)[which]))
        self._ck(self._L.ngicp_math_selftest(self._h, int(which), _p(a, c_f64p), a.shape[0], _p(out, c_f64p)))
        return out

    def stepSelftest(self, problems) -> np.ndarray:
        """One optimiser step per row of `problems` (132 doubles, include/ngicp.h) in both forms -> uint8 [n][2][record]: the serial
        step, then the wave-level one.  A record is the state image, then 18 doubles: trace row 8, d 6, done, converged, lm_failed, trial."""
        a = np.ascontiguousarray(problems, dtype=np.float64)
        assert a.ndim == 2 and a.shape[1] == 132
        rec = C.c_size_t(0)
        self._ck(self._L.ngicp_step_selftest(self._h, None, 0, None, C.byref(rec)))
        out = np.zeros((a.shape[0], 2, rec.value), dtype=np.uint8)
        if a.shape[0]:
            self._ck(self._L.ngicp_step_selftest(self._h, _p(a, c_f64p), a.shape[0], _p(out, C.POINTER(C.c_ubyte)), C.byref(rec)))
        return out

    def measureCopyBandwidth(self, nbytes: int = 1 << 30, reps: int = 10) -> float:
        """Device float4 stream copy, (read + write) GB/s."""
        v = C.c_double(0)
        self._ck(self._L.ngicp_measure_copy_bandwidth(self._h, int(nbytes), int(reps), C.byref(v)))
        return v.value

    # ---- covariances sharded over ranks (K1 with an all-gather of the packed covariances) ----
    def covsShardBegin(self, which: int):
        """-> (device pointer of the packed [n][6] FP64 set, n).  which: 0 source, 1 target."""
        ptr = C.c_void_p(0); n = C.c_size_t(0)
        self._ck(self._L.ngicp_covs_shard_begin(self._h, int(which), C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def covsShardCompute(self, which: int, lo: int, hi: int, stream: int = 0):
        self._ck(self._L.ngicp_covs_shard_compute(self._h, int(which), int(lo), int(hi), C.c_void_p(stream) if stream else None))

    def covsShardCommit(self, which: int):
        self._ck(self._L.ngicp_covs_shard_commit(self._h, int(which)))

    # ---- point-sharded stepping; buffers are raw device pointers ----
    def sharded_begin(self, guess=None):
        g = _colmajor16(np.eye(4) if guess is None else guess, np.float32)
        self._ck(self._L.ngicp_sharded_begin(self._h, _p(g, c_f32p)))

    def sharded_pass(self, sums_dev_ptr: int, stream: int = 0):
        self._ck(self._L.ngicp_sharded_pass(self._h, C.c_void_p(sums_dev_ptr), C.c_void_p(stream) if stream else None))

    def sharded_step(self, sums_dev_ptr: int, stream: int = 0) -> bool:
        done = C.c_int(0)
        self._ck(self._L.ngicp_sharded_step(self._h, C.c_void_p(sums_dev_ptr), C.c_void_p(stream) if stream else None, C.byref(done)))
        return bool(done.value)

    def sharded_finish(self):
        T = np.empty(16, dtype=np.float32); H = np.empty(36); conv, nit = C.c_int(0), C.c_int(0)
        self._ck(self._L.ngicp_sharded_finish(self._h, _p(T, c_f32p), C.byref(conv), C.byref(nit), _p(H, c_f64p)))
        self.final_transformation_ = T.reshape(4, 4).T.copy()
        self.converged_ = bool(conv.value); self.nr_iterations_ = nit.value
        self.final_hessian_ = H.reshape(6, 6).T.copy()
        return self.final_transformation_


def keyframe_covariances(target, keyframe_sizes, k: int = 20, device: int = 0) -> np.ndarray:
    """Per-keyframe covariances of a submap that is a concatenation of keyframes, concatenated in the same order — DLO's
    `keyframe_normals` / `submap_normals` (src/dlo/odom.cc:1172-1174,1318-1325): each keyframe's covariances come from ITS OWN
    points only.  Used by tests and bench.py to prepare the scan-to-submap workloads."""
    e = NanoGICP(device=device)
    e.setCorrespondenceRandomness(k)
    out, lo = [], 0
    for n in keyframe_sizes:
        e.setInputSource(np.ascontiguousarray(target[lo:lo + n]))
        e.calculateSourceCovariances()
        out.append(e.getSourceCovariances())
        lo += n
    e.close()
    return np.concatenate(out)
