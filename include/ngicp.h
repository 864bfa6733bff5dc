/* =============================================================================
 * ngicp.h — C ABI of the MI355X-native NanoGICP scan-matching engine.
 *
 * One opaque handle per nano_gicp::NanoGICP<PointXYZI,PointXYZI> instance
 * (DLO holds two: include/dlo/odom.h:119-120).  Plain pointers and sizes only:
 * no C++/torch/PCL/Eigen types cross this boundary.  Paths below are relative to
 * the reference tree (/root/reference/).
 *
 * Conventions
 *  - every entry returns an int status: 0 = OK, <0 = error (ngicp_last_error()
 *    gives the text); nothing throws or aborts across the boundary;
 *  - a handle is single-caller at a time but may be called from any host thread
 *    (DLO's AsyncSpinner(0): src/dlo/odom_node.cc:27); each entry selects the
 *    handle's device and works on the handle's own HIP stream;
 *  - clouds are given as a pointer to the first float of the first point plus a
 *    byte stride (32 for pcl::PointXYZI, include/dlo/dlo.h:50; 12 for packed xyz);
 *    only x,y,z are read.  `host_identity` is the caller's stand-in for the
 *    reference's shared_ptr identity test (include/nano_gicp/impl/nano_gicp_impl.hpp:
 *    114,122,133): a call with the identity already set on that slot is a no-op;
 *    0 means "no identity, always re-upload";
 *  - 4x4 matrices are column-major (Eigen default); covariances travel as the
 *    reference's std::vector<Eigen::Matrix4d> memory image: N x 16 doubles,
 *    column-major, 3x3 block + zero 4th row/column, in the cloud's ORIGINAL point
 *    order (the engine keeps its own cell-sorted order internally).
 * ============================================================================= */
#ifndef NGICP_H
#define NGICP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ngicp ngicp_t;

/* status codes */
#define NGICP_OK 0
#define NGICP_ERR_HIP (-1)        /* a HIP runtime call failed (no device, OOM, ...) */
#define NGICP_ERR_ARG (-2)        /* bad argument */
#define NGICP_ERR_STATE (-3)      /* call sequence error (e.g. align() without target) */
#define NGICP_ERR_K_TOO_LARGE (-4)/* k > cloud size or k > 32: undefined in the reference, explicit error here */

/* regularisation (include/nano_gicp/gicp/gicp_settings.hpp:47).  NORMALIZED_MIN_EIG of a rank-0 neighbourhood (k = 1, or k
 * coincident points: every singular value is 0) is 1e-3 * I, as MIN_EIG gives; the reference leaves that case unspecified. */
#define NGICP_REG_NONE 0
#define NGICP_REG_MIN_EIG 1
#define NGICP_REG_NORMALIZED_MIN_EIG 2
#define NGICP_REG_PLANE 3
#define NGICP_REG_FROBENIUS 4

/* optimiser (include/nano_gicp/lsq_registration.hpp:54) */
#define NGICP_OPT_GAUSS_NEWTON 0
#define NGICP_OPT_LEVENBERG_MARQUARDT 1

/* --- lifetime ------------------------------------------------------------- */
/* NanoGICP::NanoGICP()  impl/nano_gicp_impl.hpp:50-64 (+ LsqRegistration ctor
 * impl/lsq_registration_impl.hpp:50-63): k=20, PLANE, LM, max_iter 64, rot_eps 2e-3,
 * trans_eps 5e-4, lm_max 10, lambda factor 1e-9, corr dist FLT_MAX. */
int ngicp_create(int device, ngicp_t** out);
int ngicp_destroy(ngicp_t* h);
const char* ngicp_last_error(const ngicp_t* h); /* h may be NULL: last create() error */
const char* ngicp_version(void);

/* --- parameters ----------------------------------------------------------- */
/* setCorrespondenceRandomness impl/nano_gicp_impl.hpp:81-83; setMaxCorrespondenceDistance /
 * setMaximumIterations / setTransformationEpsilon (PCL base; consumed at impl/nano_gicp_impl.hpp:195,
 * impl/lsq_registration_impl.hpp:101,124); setRotationEpsilon / setInitialLambdaFactor
 * impl/lsq_registration_impl.hpp:69-76; setRegularizationMethod impl/nano_gicp_impl.hpp:86-88;
 * setNumThreads impl/nano_gicp_impl.hpp:70-78 (accepted, meaningless on the GPU). */
int ngicp_set_params(ngicp_t* h, int k, double max_corr_dist, int max_iter, double trans_eps, double rot_eps,
                     int optimizer, int lm_max_iter, double lm_init_lambda_factor, int regularization, int num_threads);
/* engine knob with no reference counterpart: voxel edge of the search grid in metres (0 = automatic: sized so that a
 * point sees ~24 points in its own cell).  A pure performance knob: the search is exact for any grid, so results do not
 * depend on it beyond the summation order.  `lanes_per_query` is accepted for ABI stability (0, 1, 2, 4, 8 or 16) and
 * ignored: the per-iteration kernel is built for 32-query batches with 2 lanes per query. */
int ngicp_set_tuning(ngicp_t* h, double voxel_size, int lanes_per_query);
/* How the calling thread waits for the device inside ngicp_align(): 0 (default) polls the solver's progress word without giving
 * the core up (lowest latency: a 100k -> 500k alignment is ~1 ms); 1 yields the core between polls (sched_yield: for hosts
 * that run other work on the same core - the node's other callbacks in DLO's AsyncSpinner, src/dlo/odom_node.cc:27).
 * Results do not depend on it. */
int ngicp_set_host_wait(ngicp_t* h, int mode);

/* --- clouds --------------------------------------------------------------- */
/* setInputSource impl/nano_gicp_impl.hpp:121-129: store cloud, (re)build index, clear source covs. */
int ngicp_set_source(ngicp_t* h, const float* xyz, size_t n, size_t stride_bytes, uint64_t host_identity);
/* registerInputSource impl/nano_gicp_impl.hpp:113-118: store cloud only; covariances untouched.
 * The pointer must stay valid until the next set/register/clear of the source (the reference
 * holds a shared_ptr): upload is deferred so that ngicp_share_source_index can avoid it. */
int ngicp_register_source(ngicp_t* h, const float* xyz, size_t n, size_t stride_bytes, uint64_t host_identity);
/* setInputTarget impl/nano_gicp_impl.hpp:132-139 */
int ngicp_set_target(ngicp_t* h, const float* xyz, size_t n, size_t stride_bytes, uint64_t host_identity);
/* clearSource / clearTarget impl/nano_gicp_impl.hpp:101-110 */
int ngicp_clear_source(ngicp_t* h);
int ngicp_clear_target(ngicp_t* h);
/* `gicp.source_kdtree_ = gicp_s2s.source_kdtree_;`  src/dlo/odom.cc:525 — dst adopts src's
 * device-resident source cloud + index when it refers to the same host cloud. */
int ngicp_share_source_index(ngicp_t* dst, ngicp_t* src);
/* swapSourceAndTarget impl/nano_gicp_impl.hpp:91-98 */
int ngicp_swap_source_target(ngicp_t* h);

/* --- covariances ---------------------------------------------------------- */
/* calculateSourceCovariances / calculateTargetCovariances impl/nano_gicp_impl.hpp:152-159,300-357 */
int ngicp_compute_source_covs(ngicp_t* h);
int ngicp_compute_target_covs(ngicp_t* h);
/* `gicp.source_covs_ = gicp_s2s.source_covs_;` src/dlo/odom.cc:815 (device-to-device) */
int ngicp_copy_source_covs(ngicp_t* dst, ngicp_t* src);
/* `gicp.source_covs_.clear();` src/dlo/odom.cc:526 */
int ngicp_clear_source_covs(ngicp_t* h);
int ngicp_clear_target_covs(ngicp_t* h);
/* source_covs_.size() / target_covs_.size() */
int ngicp_source_covs_size(const ngicp_t* h, size_t* n);
int ngicp_target_covs_size(const ngicp_t* h, size_t* n);
/* getSourceCovariances / getTargetCovariances include/nano_gicp/nano_gicp.hpp:100-106 */
int ngicp_get_source_covs(ngicp_t* h, double* out_n16);
int ngicp_get_target_covs(ngicp_t* h, double* out_n16);
/* setSourceCovariances / setTargetCovariances impl/nano_gicp_impl.hpp:142-149 */
int ngicp_set_source_covs(ngicp_t* h, const double* in_n16, size_t n);
int ngicp_set_target_covs(ngicp_t* h, const double* in_n16, size_t n);

/* --- registration --------------------------------------------------------- */
/* pcl::Registration::align(output, guess) -> NanoGICP::computeTransformation
 * impl/nano_gicp_impl.hpp:162-171 -> LsqRegistration::computeTransformation
 * impl/lsq_registration_impl.hpp:89-115.  Outputs: final_transformation_ (float 4x4),
 * converged_, nr_iterations_ (index of the last iteration), final_hessian_ (6x6), and — when
 * aligned_xyz_or_null != NULL — the source cloud transformed by the float matrix
 * (pcl::transformPointCloud, impl/lsq_registration_impl.hpp:114), xyz written at out_stride_bytes. */
int ngicp_align(ngicp_t* h, const float guess_colmajor[16], float T_out_colmajor[16], int* converged, int* nr_iterations,
                double final_hessian_colmajor[36], float* aligned_xyz_or_null, size_t out_stride_bytes);

/* --- parity / test hooks --------------------------------------------------- */
/* NanoGICP::linearize impl/nano_gicp_impl.hpp:214-270 (includes update_correspondences :174-211) */
int ngicp_linearize(ngicp_t* h, const double T_colmajor[16], double H_colmajor[36], double b[6], double* err);
/* NanoGICP::compute_error impl/nano_gicp_impl.hpp:273-296 (stale correspondences of the last linearize) */
int ngicp_compute_error(ngicp_t* h, const double T_colmajor[16], double* err);
/* correspondences_ / sq_distances_ of the last linearize, mapped back to ORIGINAL source/target
 * point indices (-1 = gated out). sq_dist may be NULL.  Also valid after ngicp_align: then the indices are those of the
 * alignment's last linearisation (the reference's correspondences_ after align); sq_dist is only meaningful after
 * ngicp_linearize. */
int ngicp_get_correspondences(ngicp_t* h, int* corr_n, float* sq_dist_n_or_null);
/* exact k-NN of arbitrary query points in the TARGET cloud (KdTreeFLANN::nearestKSearch,
 * include/nano_gicp/nanoflann.hpp:141-152): original target indices + float squared distances, ascending. */
int ngicp_target_knn(ngicp_t* h, const float* queries_xyz, size_t nq, size_t stride_bytes, int k, int* idx_nq_k, float* sqd_nq_k);
/* --- queries on the indexed clouds (the public search surface of the reference's trees and of pcl::Registration) ---
 * which: 0 = source index, 1 = target index (as ngicp_covs_shard_*).  The index is always the slot's CURRENT cloud (a registered
 * source is uploaded and indexed first); the reference's source_kdtree_ can still index the previous cloud after registerInputSource
 * without a tree assignment (impl/nano_gicp_impl.hpp:113-118).  Exact searches (eps = 0, like the reference).
 *
 * ngicp_knn_search: source_kdtree_ / target_kdtree_ ->nearestKSearch (include/nano_gicp/nanoflann.hpp:141-152): ngicp_target_knn's
 * contract on either index (original indices + float squared distances, ascending; k <= 32 and k <= n, else NGICP_ERR_K_TOO_LARGE). */
int ngicp_knn_search(ngicp_t* h, int which, const float* queries_xyz, size_t nq, size_t stride_bytes, int k, int* idx_nq_k, float* sqd_nq_k);
/* ->radiusSearch (nanoflann.hpp:155-175): the points whose float squared distance is STRICTLY below (float)radius - radius is a
 * squared distance, as in RadiusResultSet<float,int> (impl/nanoflann_impl.hpp:239-262), so radius <= 0 finds nothing.  The reference's
 * trees are unsorted (nanoflann.hpp:68,113-117) and return kd-tree visiting order; the engine returns the same set in ascending
 * (d2, original index) order.  ngicp_radius_search runs the search and writes offsets[0..nq] (query i's results are
 * [offsets[i], offsets[i+1])) and *total = offsets[nq]; the results stay on the device until ngicp_radius_fetch copies them
 * (capacity >= total, else NGICP_ERR_ARG).  A result too large for the device is NGICP_ERR_HIP. */
int ngicp_radius_search(ngicp_t* h, int which, const float* queries_xyz, size_t nq, size_t stride_bytes, double radius,
                        size_t* offsets_nq_plus_1, size_t* total);
int ngicp_radius_fetch(ngicp_t* h, int* idx, float* sqd, size_t capacity);
/* pcl::Registration::getFitnessScore(max_range) (PCL, not under the reference tree; restated in csrc/ngicp_query.h): the source
 * transformed by T (pcl::transformPointCloud), each point's exact 1-NN squared distance d2 in the target, the mean of the d2 with
 * (double)d2 <= max_range (a SQUARED distance; DBL_MAX = PCL's default), DBL_MAX when none counts.
 * T_colmajor_or_null: NULL = final_transformation_ of the last align (identity before any, as PCL).  Where the reference would
 * dereference the null search tree DLO hands PCL (src/dlo/odom.cc:116-120), this returns what PCL computes with a built tree. */
int ngicp_fitness_score(ngicp_t* h, const float T_colmajor_or_null[16], double max_range, double* score, size_t* n_inliers_or_null);
/* --- range select: the spaciousness metric's median (dlo::OdomNode::computeSpaciousness, src/dlo/odom.cc:990-1010) -------------
 * The range of a point is d = (float) sqrt((double)x*x + (double)y*y + (double)z*z), summed left to right in double - odom.cc:996
 * bit for bit.  Ranges are ordered ascending by value; a NaN range (a NaN coordinate) sorts AFTER +inf and is returned as the quiet
 * NaN 0x7fc00000.  ngicp_range_select: *value = the range of 0-based rank `rank` of the cloud's n ranges, computed on the device by
 * an exact radix select (csrc/ngicp_range.h: integer counts only, so the result is deterministic); ngicp_range_median: the same for
 * rank n / 2, the element std::nth_element(ds.begin(), ds.begin() + ds.size() / 2, ds.end()) leaves at ds[ds.size() / 2].  (The
 * reference's loop runs `i <= size()`: it reads one point past the end and takes rank (n + 1) / 2 of n + 1 values, one of them
 * indeterminate.  The engine implements the n-value median the loop evidently intends: INTEGRATION.md, divergences.)
 * which: 0 = source, 1 = target (the slot's CURRENT cloud; a registered source is uploaded first, as for the queries above),
 *        2 = the preprocessed scan ngicp_preprocess_scan left on the device (non-finite rows that remove_nan = 0 left in it count).
 * *n_points_or_null = n, written as soon as the cloud is known (also when the rank is then refused).
 * Errors: NGICP_ERR_STATE for a missing or empty cloud - for which = 2 also once a later call has consumed the filter workspace,
 * exactly when ngicp_set_source_preprocessed would refuse; NGICP_ERR_ARG for rank >= n, which outside 0..2 or a null value.
 * One 4-byte read-back and one synchronisation per call.  Changes nothing any other getter returns (scratch of its own);
 * ngicp_stats.query_ms is the device time of its kernels. */
int ngicp_range_select(ngicp_t* h, int which, size_t rank, float* value, size_t* n_points_or_null);
int ngicp_range_median(ngicp_t* h, int which, float* value, size_t* n_points_or_null);
/* --- voxelized GICP: align against per-voxel target distributions (no counterpart in the reference; csrc/ngicp_voxel.h) ---
 * A MODE of the handle, selected like the regularisation method: res > 0 selects it, 0 (the default) selects exact GICP; a negative or
 * non-finite value is NGICP_ERR_ARG.  It is a different algorithm with different results, not a second route to the same answer.  The
 * definition is this project's own; no bit-fidelity to any outside library is claimed.
 *   voxel of a float point p   ijk = floorf(p * inv_res) per axis, inv_res = 1.0f / (float)res (one float multiply, nothing fused)
 *   voxel map of the target    per occupied voxel v, summed in ascending original target index: n_v, mean_v = (sum (double)p_j) / n_v,
 *                              cov_v = (sum C_j) / n_v over the target covariances (computed, or set through ngicp_set_target_covs / the
 *                              submap store).  Voxels are numbered in ascending (iz, iy, ix).  Memory is O(occupied voxels).  A target
 *                              with |i| >= 2^20 on any axis (or a non-finite point) is refused with NGICP_ERR_ARG when the map is built.
 *                              Built lazily, at the first align / linearize / compute_error / voxelmap call after the target, its
 *                              covariances or the resolution changed.
 *   correspondence (DIRECT1)   source point i at pose T: q = float(T) * a_i in float, ((c0 x + c1 y) + c2 z) + c3; it corresponds to the
 *                              voxel of q if that voxel is occupied, else to nothing.  max_corr_dist is NOT consulted in this mode:
 *                              voxel membership is the gate.
 *   terms (FP64)               e = mean_v - T a_i, M = (cov_v + R C_i R^T)^-1: err += n_v e^T M e, H += n_v J^T M J, b += n_v J^T M e.
 * The loop (LM / GN, lambda schedule, trial passes, convergence test, trace), the final Hessian, the convergence flag and the iteration
 * count are those of exact GICP.  While the mode is on, ngicp_get_correspondences returns the VOXEL NUMBER (or -1) per source point
 * and the float squared distance to (float)mean_v (inf without a voxel), and ngicp_align_batch, ngicp_sharded_* and ngicp_covs_shard_*
 * return NGICP_ERR_ARG ("not available with a voxelized target").  Queries, keyframes, the submap, filters and the range median are
 * unaffected.  ngicp_stats: mean_candidates counts hash-table slots looked at per source point and pass; voxelmap_ms is the build. */
int ngicp_set_voxel_resolution(ngicp_t* h, double res);
/* The neighbourhood of the correspondence rule: a fixed, ordered list of K integer voxel offsets (dx, dy, dz).
 *   NGICP_VOX_DIRECT1  (K = 1, the default)  (0,0,0): the rule above, bit for bit
 *   NGICP_VOX_DIRECT7  (K = 7)               slot 0 (0,0,0); slots 1-6 (+1,0,0) (-1,0,0) (0,+1,0) (0,-1,0) (0,0,+1) (0,0,-1)
 *   NGICP_VOX_DIRECT27 (K = 27)              every (dx,dy,dz) in {-1,0,1}^3 in ascending (dz, dy, dx), dx fastest - the order of the voxel
 *                                            key; the centre is slot 13
 * Source point i at pose T: c = floorf(q * inv_res) as above.  If c is out of range on any axis (|c| >= 2^20, or q is not finite) the
 * point has no correspondence in any slot.  Otherwise slot s corresponds to voxel c + off[s] if every component of c + off[s] is below
 * 2^20 in magnitude (tested on the integers, before any key is formed: nothing carries into the neighbouring key field) and that voxel is
 * occupied; else slot s is -1.  Every occupied slot contributes the terms above (e = mean_v - T a_i, M = (cov_v + R C_i R^T)^-1, weight
 * n_v); a point's terms are added in ascending slot, R C_i R^T is formed once per point.  The trial error uses the frozen n_v M and the
 * voxel of every slot of the previous linearisation.  max_corr_dist remains unconsulted.
 * ngicp_set_voxel_neighbors: any other value is NGICP_ERR_ARG.  It may be called whether or not the mode is on, and is remembered.
 * Setting the value already set does nothing.  A change keeps the voxel map (which does not depend on the neighbourhood) and drops the
 * correspondences and the hooks' state, as a change of resolution does: ngicp_compute_error, ngicp_get_correspondences and
 * ngicp_voxel_correspondences return NGICP_ERR_STATE until the next linearisation.  Per-slot state on the device: 2 * K * 52 bytes per
 * source point.  In DIRECT7 / DIRECT27 ngicp_get_correspondences keeps its shape and reports the CENTRE slot's voxel and the float
 * squared distance to its (float)mean_v.  ngicp_stats keeps its layout; two fields change meaning: mean_candidates counts hash-table
 * slots looked at per source point and pass over all K lookups, and valid_fraction counts PAIRS (occupied slots) per source point and
 * pass, so it can exceed 1.  ngicp_align_batch, ngicp_sharded_* and ngicp_covs_shard_* stay refused while the mode is on. */
#define NGICP_VOX_DIRECT1 1
#define NGICP_VOX_DIRECT7 7
#define NGICP_VOX_DIRECT27 27
int ngicp_set_voxel_neighbors(ngicp_t* h, int mode);
int ngicp_get_voxel_neighbors(const ngicp_t* h, int* mode);
/* the voxel numbers of every slot of the last linearisation, row-major n_src x K in original source order, -1 where a slot is empty.
 * *K_out (may be NULL) is the neighbourhood's K; capacity_ints < n_src * K is NGICP_ERR_ARG (K_out is set first).  Valid when
 * ngicp_get_correspondences is; NGICP_ERR_STATE while the voxel mode is off. */
int ngicp_voxel_correspondences(ngicp_t* h, int* corr_n_by_K, size_t capacity_ints, int* K_out);
/* how many voxel maps this handle has built since it was created: only a build adds to it (a stale map is rebuilt at its next use;
 * a change of neighbourhood does not make it stale) */
int ngicp_voxelmap_builds(const ngicp_t* h, long long* n_builds);
/* the number of occupied voxels (builds the map if it is stale; NGICP_ERR_STATE while the mode is off) */
int ngicp_voxelmap_size(ngicp_t* h, size_t* n_voxels);
/* the map, voxels in the numbering above: ijk (n x 3 ints), mean (n x 3), cov (n x 6: xx, xy, xz, yy, yz, zz), count (n).  Every
 * pointer may be NULL.  Builds the map if it is stale. */
int ngicp_voxelmap_get(ngicp_t* h, int* ijk_n3, double* mean_n3, double* cov_n6, int* count_n);
/* --- merged voxel map: a submap's map from per-keyframe voxel sums (csrc/ngicp_voxel.h) ---------------------------
 * A SETTING of the voxelized mode, OFF by default.  With it off nothing changes anywhere: the map of every target is the one defined
 * above, summed over the concatenation.  With it on, the map of a target that ngicp_submap_set assembled is formed from sums each
 * keyframe carries, built once per keyframe and resolution.  That adds per-keyframe partial sums and is therefore NOT the definition
 * above; it has this one of its own.
 *   voxel part of keyframe k   over the keyframe's points as the store holds them (world frame), with the voxel rule above
 *   at resolution res          (floorf(p * inv_res), |i| < 2^20): for every voxel v that holds a point of k, n_kv, s_kv = sum (double)p_j
 *                              (3 entries) and c_kv = sum C_j (6 entries).  Every sum starts at 0.0 and adds one term after the other in
 *                              ascending original index inside the keyframe.  Voxels in ascending (iz, iy, ix).  No division.  A point
 *                              2^20 voxels or more from the origin, or a non-finite one, refuses the build with NGICP_ERR_ARG; the
 *                              message names the keyframe id.  88 bytes of device memory per keyframe voxel.
 *   merged map of ids[0..m)    voxel v is occupied if any listed keyframe's part has it.  With i_1 < ... < i_r the positions in ids
 *                              whose part has v: S = s_{ids[i_1], v}, then S = S + s_{ids[i_t], v} for t = 2..r; C likewise from the c
 *                              sums; n_v = sum n.  mean_v = S / (double)n_v, cov_v = C / (double)n_v.  An id listed twice counts twice,
 *                              as it does in the concatenation.
 * The map keeps its format, its voxel numbering and its key table; the passes are the same kernels.  Consequences: ijk, counts and voxel
 * numbers are exactly those of the map defined above for the same submap, so correspondences at a given pose are identical; means and
 * covariances differ from it in rounding only; with a single id the two maps are bit-equal.
 * The merged route is taken only when the setting is on, the current target is the submap ngicp_submap_set assembled, and its
 * covariances are still the set ngicp_submap_set installed: after ngicp_set_target_covs or ngicp_compute_target_covs the map is built
 * from the points, as for any other target.  A part is built lazily (only a merged build or ngicp_keyframe_voxelmap_get asks for one),
 * replaced when the resolution differs, and freed by ngicp_keyframe_clear.
 * ngicp_set_voxel_submap_merge: on != 0 switches the setting on.  It may be called whether or not the voxel mode is on, and is
 * remembered.  Setting the value already set does nothing.  A change drops the voxel map, the hooks' state and the correspondences, as a
 * change of resolution does.  ngicp_stats::voxelmap_ms and ngicp_voxelmap_builds keep their meaning: the last build and all builds, by
 * either route. */
int ngicp_set_voxel_submap_merge(ngicp_t* h, int on);
int ngicp_get_voxel_submap_merge(const ngicp_t* h, int* on);
/* maps built by the merged route and keyframe parts built, both since the handle was created; the device (event) times of the last
 * merged build, split into its part builds (0 when every part was there) and the merge itself.  Every pointer may be NULL. */
int ngicp_voxelmap_merge_stats(const ngicp_t* h, long long* merged_builds, long long* parts_built, double* last_parts_ms, double* last_merge_ms);
/* the voxel part of keyframe `id` at the current resolution, built if absent: *n_vox voxels; ijk (n x 3 ints), sum (n x 3),
 * covsum (n x 6: xx, xy, xz, yy, yz, zz), count (n).  The array pointers may be NULL to ask for the size only.  NGICP_ERR_STATE while
 * the voxel mode is off, NGICP_ERR_ARG for an unknown id. */
int ngicp_keyframe_voxelmap_get(ngicp_t* h, int id, size_t* n_vox, int* ijk_n3, double* sum_n3, double* covsum_n6, int* count_n);
/* --- rolling voxel map: insert scans, evict voxels, align (csrc/ngicp_voxel_roll.h) ---------------------------------
 * A SETTING of the voxelized mode, OFF by default.  With it off nothing changes anywhere.  With it on (and res > 0) the voxelized
 * entries align against a device-resident map that the caller maintains across frames, instead of a map built from the target.  It is
 * this project's own definition; no fidelity to any outside library is claimed.
 *   state                      per voxel v, in double: S_v (3 entries), C_v (6 entries: xx, xy, xz, yy, yz, zz), a count n_v and a stamp
 *                              t_v, the number of the last insert that added a point to v; the handle counts its accepted inserts
 *                              from 1.  Beside them the record the passes read, in the voxel map's format: mean_v = S_v / (double)n_v,
 *                              cov_v = C_v / (double)n_v, n_v.
 *   insert of cloud A at the   A is `from`'s current source cloud, as for ngicp_keyframe_add_transformed; its source covariances C_j are
 *   float pose T               computed with `from`'s k and regularisation if missing, exactly as ngicp_keyframe_add does.
 *                              q_j = T a_j in the order of ngicp_transform_source (pcl::transformPointCloud); the voxel of q_j by the
 *                              mode's rule, floorf(q * inv_res), |i| < 2^20.  Per voxel of the scan, in ascending original index of A,
 *                              every sum started at 0.0: s = sum (double)q_j, c = R (sum C_j) R^T with R the row-major double image of
 *                              T's float 3x3 block - ONE rotation per voxel, applied to the sum, evaluated as the passes evaluate
 *                              R C_a R^T - and n.  For a voxel the map has: S = S + s, C = C + c (one addition per entry), n += n,
 *                              t = this insert.  A new voxel starts from the scan's sums themselves.  The records of the touched voxels
 *                              are rewritten by one division per entry.
 *   numbering                  voxels are numbered in order of first insertion; the new voxels of one insert in ascending (iz, iy, ix).
 *                              An insert never changes the number of an existing voxel.
 *   refusal                    an insert with a transformed point that has no voxel (2^20 or more voxels from the origin on an axis, or
 *                              not finite) returns NGICP_ERR_ARG and changes nothing: map, counter and stamps stay as they were.
 *   evict(c, max_dist,         voxel v is removed if max_dist > 0 and ((dx*dx + dy*dy) + dz*dz) > max_dist*max_dist with
 *         min_stamp)           d = ((double)i + 0.5) * res - (double)c per axis (all in double, nothing fused), or if min_stamp > 0 and
 *                              t_v < min_stamp.  Survivors keep their relative order and are renumbered densely.  The map may end empty.
 *   clear                      empties the map and resets the insert counter.  ANY change of the resolution does the same (the sums belong
 *                              to one resolution), whether or not the setting is on; a change of neighbourhood keeps the map.
 * Insert, evict and clear drop the correspondences and the hooks' state, as a change of resolution does: ngicp_compute_error,
 * ngicp_get_correspondences and ngicp_voxel_correspondences return NGICP_ERR_STATE until the next linearisation.
 * While the setting is on and res > 0: ngicp_align, ngicp_linearize, ngicp_compute_error, ngicp_voxel_align_batch, ngicp_voxelmap_size
 * and ngicp_voxelmap_get use the rolling map (ngicp_voxelmap_get then lists the voxels in the numbering above).  THE TARGET SLOT IS NOT
 * READ AT ALL: it may be empty or hold anything; an empty rolling map is NGICP_ERR_STATE where a missing target would be.  The merged
 * setting (ngicp_set_voxel_submap_merge) is ignored.  ngicp_voxelmap_builds and ngicp_stats::voxelmap_ms keep their meaning - inserts
 * are not builds - and ngicp_stats::n_tgt reports the voxel count.  The exact path, the queries, keyframes, the submap, the filters and
 * the range median are unaffected.
 * Device memory: 208 bytes per voxel of capacity (80 sums, 80 record, 8 key, 8 stamp, 32 of the key table, which stays at most half
 * full); the per-voxel arrays start at 1024 voxels and double, the table starts at 64 slots and doubles.  An eviction uses a grow-only
 * workspace of 176 bytes per voxel; an insert 100 bytes per scan point on top of the voxel builds' sort buffers.
 * ngicp_set_voxel_rolling: on != 0 switches the setting on.  Callable in any mode and remembered.  Setting the value already set does
 * nothing.  Switching off keeps the rolling map and returns every entry to the target-based map; switching on again finds the map as it
 * was left.  A change drops the correspondences and the hooks' state.
 * ngicp_voxel_rolling_insert / _evict: NGICP_ERR_STATE unless the setting is on and res > 0.  `from` may be h itself (the usual loop:
 * align, then insert at the result).  *n_new: voxels the insert created; *n_touched: voxels of the scan (created or added to).
 * ngicp_voxel_rolling_get: the state in the numbering above - ijk (n x 3 ints), S (n x 3), C (n x 6), n (n), stamps (n); every array
 * pointer may be NULL.  ngicp_voxel_rolling_stats: accepted inserts since the last clear, voxels, capacity of the per-voxel arrays,
 * table slots, and the device event times of the last insert and the last eviction. */
int ngicp_set_voxel_rolling(ngicp_t* h, int on);
int ngicp_get_voxel_rolling(const ngicp_t* h, int* on);
int ngicp_voxel_rolling_insert(ngicp_t* h, ngicp_t* from, const float T_colmajor[16], size_t* n_new_or_null, size_t* n_touched_or_null);
int ngicp_voxel_rolling_evict(ngicp_t* h, const float centre[3], double max_dist, long long min_stamp, size_t* n_removed_or_null);
int ngicp_voxel_rolling_clear(ngicp_t* h);
int ngicp_voxel_rolling_get(ngicp_t* h, size_t* n_vox, int* ijk_n3, double* sum_n3, double* covsum_n6, int* count_n, long long* stamp_n);
int ngicp_voxel_rolling_stats(const ngicp_t* h, long long* inserts, size_t* n_vox, size_t* capacity_vox, size_t* table_slots, double* last_insert_ms, double* last_evict_ms);
/* --- rolling voxel map: records - restore, merge and move a map from its voxel sums (csrc/ngicp_voxel_roll.h) -------
 * A RECORD is what ngicp_voxel_rolling_get returns per voxel: S (3 doubles), C (6 doubles: xx, xy, xz, yy, yz, zz), n (int, at least 1)
 * and a stamp.  The state of the map is per-voxel sums, so it can be taken back, added to another map and moved without the points.
 * All four entries return NGICP_ERR_STATE unless the rolling setting is on and res > 0, and - when they succeed - drop the
 * correspondences and the hooks' state as the scan insert does.  None of them reads or changes the target slot, the last alignment's
 * results or ngicp_voxelmap_builds.
 *   restore: _set              the map becomes exactly the given state: voxel v has key ijk[v], sums S[v], C[v], n[v] and stamp stamp[v];
 *                              the numbering is the array order; the insert counter becomes `inserts`.  S and C are taken as they are.
 *                              The records the passes read are written by one division per entry, the key table is filled as after an
 *                              eviction.  n_vox == 0 empties the map and sets the counter.  NGICP_ERR_ARG, and then nothing changes (map,
 *                              numbering, counter, stamps, table): a null array with n_vox > 0, |i| >= 2^20 on any axis, a count below 1,
 *                              a stamp outside 1..inserts, inserts < 0, two equal ijk rows (the message names both rows), more voxels
 *                              than int indices allow.  Round trip: _get plus the `inserts` of _stats, _set on any handle with the same
 *                              resolution, _get: the same bytes in every array.
 *   insert of records at the   per record r, in ascending input index: m = S_r / (double)n_r (three divisions), p = (float)m per axis,
 *   float pose T               q = T p in the order of the scan insert's transform; the destination voxel is the voxel of q by the mode's
 *                              rule at h's resolution.  Per destination voxel, over its records in ascending input index, every sum
 *                              started at 0.0: A = sum S_r, Cc = sum C_r (one addition per entry and record), N = sum n_r in integers;
 *                              s_k = ((R[k][0]*A_0 + R[k][1]*A_1) + R[k][2]*A_2) + (double)N * (double)t_k, nothing fused;
 *                              c = R Cc R^T, ONE rotation per destination voxel, evaluated as the scan insert's; R the row-major double
 *                              image of T's float 3x3 block, t its float translation.  The commit is the scan insert's: an existing
 *                              voxel gets one addition per entry, a new one starts from (s, c, N); new voxels are numbered in ascending
 *                              (iz, iy, ix) behind the existing ones; the stamp is this insert's number and the counter advances by one;
 *                              the records of the touched voxels are rewritten by one division per entry.
 *                              NGICP_ERR_ARG, nothing written (all of it is found before the first write to the map; capacity and table
 *                              stay as they were too): a record whose moved mean has no voxel (2^20 voxels or more from the origin, or
 *                              not finite), a count below 1, a destination voxel whose count would pass 2^31 - 1, no records, null arrays.
 *   A WHOLE SOURCE VOXEL       lands in the voxel of its moved mean.  That is the definition, with its consequences: several records
 *                              may merge into one voxel; a map moved by T and then by T^-1 is not the original in general; a map taken
 *                              to a coarser (or finer) resolution this way is not the map the points would have built.  With T the
 *                              identity, q == p and both the rotation and the added N * 0 are exact: where every record's float mean
 *                              lies in that record's own voxel, inserting a map into an empty map of the same resolution reproduces
 *                              S, C and n bit for bit.
 *   _insert_voxels             takes the records from host arrays (n_rec of them).
 *   _insert_map                takes them from `from`'s rolling map on the device, in its numbering, without a pass through the host;
 *                              h's stream waits for `from`'s on the device.  `from` need neither have the rolling setting on nor h's
 *                              resolution: only its sums are read, and it is left unchanged.  NGICP_ERR_ARG: from == h, handles on
 *                              different devices, an empty `from`.
 *   move in place: _transform  the map becomes what the insert above gives for its own former records, in their former numbering,
 *                              inserted into an empty map.  The insert counter stays.  A destination voxel's stamp is the largest stamp
 *                              of the records that landed in it: ages survive a move, and evict(min_stamp) keeps working.  A refusal
 *                              leaves the map as it was.  An empty map is a no-op that returns 0.  *n_vox_after: the voxels left.
 * *n_new / *n_touched as for the scan insert: voxels created, destination voxels (created or added to).
 * Host synchronisations: two per insert or move (the destination voxel count with the refusal flags; the number of new voxels with the
 * overflow flag), both before the map is written; the commit is left in the handle's stream.  ngicp_voxel_rolling_stats'
 * last_insert_ms also reports the last record insert or move; asking for it waits for that commit.  _set: one.
 * Device memory on top of the map's: an insert of n records uses the voxel builds' sort buffers for n keys, 84 bytes per record of
 * workspace (80 destination sums, 4 lookup result), 8 more per record for a move, and 76 per uploaded record (_insert_voxels; 88 for _set). */
int ngicp_voxel_rolling_set(ngicp_t* h, size_t n_vox, const int* ijk_n3, const double* sum_n3, const double* covsum_n6, const int* count_n, const long long* stamp_n, long long inserts);
int ngicp_voxel_rolling_insert_voxels(ngicp_t* h, size_t n_rec, const double* sum_n3, const double* covsum_n6, const int* count_n, const float T_colmajor[16], size_t* n_new_or_null,
                                      size_t* n_touched_or_null);
int ngicp_voxel_rolling_insert_map(ngicp_t* h, ngicp_t* from, const float T_colmajor[16], size_t* n_new_or_null, size_t* n_touched_or_null);
int ngicp_voxel_rolling_transform(ngicp_t* h, const float T_colmajor[16], size_t* n_vox_after_or_null);
/* --- rolling voxel map: clearing along rays - drop what the sensor now sees through (csrc/ngicp_voxel_ray.h) ---------
 * Eviction removes voxels by distance and by age; nothing else removes a voxel whose content has moved away.  This entry counts, per
 * map voxel, the rays of a scan that pass through it (miss) and that end in it (hit), and removes the voxels seen through often enough.
 * It changes nothing else; while it is not called every other result is bit for bit what it was.  The project's own definition.
 *   rays                       A is `from`'s current source cloud (`from` may be h); q_j = T a_j exactly as ngicp_voxel_rolling_insert
 *                              computes it (float, in the order of ngicp_transform_source).  The origin o is three floats in the map
 *                              frame; NULL means T's float translation.  c0 is the cell of o and c1 the cell of q_j by the mode's rule,
 *                              floorf(x * inv_res), |i| < 2^20.  A q_j or an o without a cell (2^20 cells or more from the map's origin
 *                              on an axis, or not finite): NGICP_ERR_ARG and nothing changes - map, numbering, stamps, insert counter,
 *                              table, the hooks' state and the counts of the last accepted call all stay.
 *   the walk                   in double, nothing fused.  od = (double)o, qd = (double)q_j, d = qd - od.  Per axis a:
 *                              n_a = |c1_a - c0_a|, s_a = sign(c1_a - c0_a), inv_a = 1.0 / d_a (used only where n_a > 0; there d_a != 0
 *                              and has the sign of s_a).  The ray takes exactly N = n_x + n_y + n_z steps.  Before a step it is in cell
 *                              cur and has taken k_a steps along axis a; the candidates are the axes with k_a < n_a, with the
 *                              parameters t_a = ((double)(cur_a + (s_a > 0 ? 1 : 0)) * res - od_a) * inv_a.  The step goes along the
 *                              candidate with the smallest t_a - a tie goes to the lowest axis, x before y before z - and sets
 *                              cur_a += s_a.  The cell behind step N is c1 by construction: the walk is 6-connected, and its length is
 *                              set by the cells, not by floating point.  A diagonal through exact corners steps x, y, z, x, y, z, ...
 *   counted steps              step j (1 .. N; "its cell" is the cell behind it) is counted when
 *                              near_cells <= j <= min(N - 1 - back_cells, max_steps).  The origin's cell and the end cell are never
 *                              among them.  The walk stops behind its last counted step: a ray's cost is bounded by max_steps, not by
 *                              how far away its point lies.
 *   a miss                     at a counted step the cell's key is looked up in the map's table; without a voxel there nothing
 *                              happens.  With voxel v and radius_cells > 0: m = the mean in v's record (S_v / n_v), w = m - od,
 *                              dd = (d_x*d_x + d_y*d_y) + d_z*d_z, ts = ((w_x*d_x + w_y*d_y) + w_z*d_z) / dd, e = w - ts * d per axis;
 *                              the step is a miss when ((e_x*e_x + e_y*e_y) + e_z*e_z) <= r*r, r = radius_cells * res: the distance
 *                              of the mean from the infinite line, ts not clamped.  With radius_cells == 0 every counted step in an
 *                              occupied cell is a miss.  miss[v] counts the misses; hit[v] counts the rays whose c1 is v's cell
 *                              (whether or not the walk was cut short).  Why a radius: a ray that descends to a floor far away runs
 *                              through the CELLS of the floor layer for metres, above the floor itself; the mean of such a voxel lies
 *                              on the surface, and the ray does not come near it.
 *   removal                    voxel v goes when miss[v] >= min_miss and hit[v] == 0 and (keep_stamp <= 0 or t_v < keep_stamp).
 *                              Survivors keep their relative order and are renumbered densely; stamps and the insert counter stay; the
 *                              table is rebuilt.  The correspondences and the hooks' state are dropped as an eviction drops them
 *                              (whether or not a voxel went).  dry_run != 0 counts and removes nothing: map, table, correspondences and
 *                              hooks are left byte for byte alone.
 *   results                    n_removed; the numbers of counted steps, of counted steps in occupied cells and of misses over all rays
 *                              (integer sums: exact, whatever the order); the device event time of the counting kernel.  miss and hit
 *                              of the last accepted call stay on the device in the numbering from BEFORE that call's removal:
 *                              ngicp_voxel_rolling_ray_counts reads them back (*n_out voxels; NULL arrays ask for the size only;
 *                              NGICP_ERR_ARG when capacity < *n_out).  It returns NGICP_ERR_STATE when no call has been accepted, or
 *                              when anything else has written the map since (insert, evict, clear, restore, move, a change of
 *                              resolution).  An empty map: 0 removed, the steps counted, no counts to read (*n_out == 0).
 * Errors of _ray_clear: NGICP_ERR_STATE unless the rolling setting is on and res > 0.  NGICP_ERR_ARG: near_cells < 1, back_cells < 0,
 * max_steps outside 1 .. 65536, min_miss < 1, radius_cells negative or not a number, a null T, a producer without a source cloud,
 * handles on different devices.
 * One host synchronisation per call - the refusal flag, the survivors' count and the totals in one read-back, behind the compaction into
 * a workspace and before anything is copied back; the copies and the table rebuild are left in the handle's stream.  Device memory: 16
 * bytes per voxel (two pairs of 32-bit counters: a refused call counts into the pair the last accepted call does not occupy) and the
 * eviction's workspace.
 * Not here: miss counters that persist across scans (the dry run's counts let a caller keep its own), a Mahalanobis test against the
 * voxel's covariance, clearing of the target-based or merged maps, sharded and batch entries. */
typedef struct ngicp_ray_clear_options {
  int near_cells;        /* the first counted step (1) */
  int back_cells;        /* steps before the end cell that are not counted (2) */
  int max_steps;         /* the last step a ray may count, 1 .. 65536 (4096) */
  int min_miss;          /* misses that remove a voxel without a hit (2) */
  double radius_cells;   /* r / res of the miss test; 0: the cell test alone (0.25) */
  long long keep_stamp;  /* > 0: voxels with a stamp of at least this stay (0) */
  int dry_run;           /* != 0: count only (0) */
} ngicp_ray_clear_options;   /* NULL: the defaults in brackets */
typedef struct ngicp_ray_clear_result {
  size_t n_removed;
  long long steps, occupied, misses;  /* counted steps; of them in occupied cells; of those, misses */
  double kernel_ms;                   /* device event time of the counting kernel */
} ngicp_ray_clear_result;
int ngicp_voxel_rolling_ray_clear(ngicp_t* h, ngicp_t* from, const float T_colmajor[16], const float* origin_or_null, const ngicp_ray_clear_options* options_or_null,
                                  ngicp_ray_clear_result* result_out_or_null);
int ngicp_voxel_rolling_ray_counts(ngicp_t* h, uint32_t* miss_n_or_null, uint32_t* hit_n_or_null, size_t capacity, size_t* n_out_or_null);
/* --- rolling voxel map: gated insert - keep what the map contradicts out (csrc/ngicp_voxel_gate.h) ------------------
 * ngicp_voxel_rolling_insert adds every point of a scan, the points of a passer-by among them.  This entry classifies the scan's points
 * against the rolling map at the pose and inserts only the points the map explains, or that fall where it holds nothing - in one call,
 * on the device.  It changes nothing else; while it is not called every other result is bit for bit what it was.  The project's own
 * definition.
 *   inputs                     ngicp_voxel_rolling_insert's: `from`'s current source cloud A (`from` may be h) with its covariances C_j
 *                              (computed if missing, as the insert does) and the float pose T.
 *   per point j, in its ORIGINAL index:
 *   slots                      exactly voxel fitness's ("voxel fitness" below), under the neighbourhood in force on h (DIRECT1 / 7 / 27):
 *                              q = the float pose times the point in the passes' order, ((c0 x + c1 y) + c2 z) + c3; its cell by the
 *                              mode's rule; slot s is cell + offset s, in range on the integers; a slot is OCCUPIED when the rolling map
 *                              has that voxel.  A point whose q has no cell has no slots.
 *   judging slots              the occupied slots whose voxel count n_v is >= min_voxel_count.  The term m_s is voxel fitness's,
 *                              e^T (cov_v + R C_a R^T)^-1 e in FP64 in the same order of operations (no factor n_v).  best = +inf; in
 *                              ascending slot a judging slot wins when m_s < best: ties go to the lower slot, NaN and +inf never win.
 *   class                      NGICP_GATE_NEW (0): no occupied slot.  NGICP_GATE_EXPLAINED (1): a winner exists and
 *                              best <= max_mahalanobis.  NGICP_GATE_CONFLICT (2): a winner exists and best > max_mahalanobis.
 *                              NGICP_GATE_UNJUDGED (3): occupied slots exist but none won.
 *   kept                       EXPLAINED always; NEW iff insert_new; UNJUDGED iff insert_unjudged; CONFLICT never.
 *   the map afterwards         what ngicp_voxel_rolling_insert's definition gives for the kept points alone, in ascending original index,
 *                              with their covariances: the insert's own transform (x*c0 + (y*c1 + (z*c2 + c3)), which is NOT the gate's
 *                              q), the same keys, the same ascending-index sums per voxel, one rotation of the covariance sum, the same
 *                              numbering of new voxels, the same stamp; the counter advances by one.
 *   refusal                    the plain insert's, judged on EVERY point of the scan, kept or not, before anything is written: a
 *                              transformed point (the insert's) that is not finite or lies 2^20 voxels out returns NGICP_ERR_ARG and
 *                              changes nothing - map, counter, stamps, table, the hooks' state and the classes of the last accepted
 *                              call all stay.
 *   nothing kept               the call succeeds, changes nothing of the map and does NOT advance the insert counter (the classes and
 *                              the result are those of this call).
 *   dry_run != 0               classifies only: map, counter, stamps, hooks, stats and traces are untouched.  n_new = n_touched = 0.
 * Consequences: with min_voxel_count == 1 the classes follow from ngicp_voxel_fitness_points(T): v = -1 and m = -1 is NEW, m = +inf is
 * UNJUDGED, otherwise m is compared with the gate.  With max_mahalanobis == DBL_MAX and the default flags the call is
 * ngicp_voxel_rolling_insert bit for bit.  On an empty map every point is NEW.
 * In numpy (map: the model of the rolling map; slot_terms: voxel fitness's per-slot terms, NaN where a slot is empty):
 *     slots, m, _ = slot_terms(A, C, map, T, K);   occ = slots >= 0;   judge = occ & (map.count[slots] >= min_voxel_count)
 *     best = +inf;  won = False;  for s in range(K): w = judge[:, s] & (m[:, s] < best); best = where(w, m[:, s], best); won |= w
 *     cls = where(~occ.any(1), 0, where(~won, 3, where(best <= max_mahalanobis, 1, 2)))
 *     keep = (cls == 1) | ((cls == 0) & insert_new) | ((cls == 3) & insert_unjudged)
 *     if keep.any() and not dry_run: map.insert(A[keep], C[keep], T)
 * ngicp_voxel_rolling_insert_gated: options NULL means no gate (max_mahalanobis = DBL_MAX, which has no default of its own) and the
 * defaults in brackets.  The result: the scan's points, the points per class, the kept points, the voxels created and the voxels of the
 * kept points (created or added to), and the device event time of all launches of the call.
 * ngicp_voxel_rolling_insert_classes: the classes (one byte per point, the values above) of the last accepted gated call, dry or not, in
 * the scan's original order; *n_out points; a NULL array asks for the size only; NGICP_ERR_ARG when capacity < *n_out.  They stay
 * readable until the next accepted gated call or ngicp_voxel_rolling_clear (NGICP_ERR_STATE before the first call and after a clear); a
 * refused gated call leaves them as they were.
 * Errors of _insert_gated: NGICP_ERR_STATE unless the rolling setting is on and res > 0.  NGICP_ERR_ARG: max_mahalanobis negative, NaN
 * or infinite, min_voxel_count < 1, a null T, handles on different devices, an empty source cloud.
 * Host synchronisations: three, one more than ngicp_voxel_rolling_insert - first the refusal flag, the class counts and the kept points'
 * count in one read-back (a dry run, or a call that keeps nothing, ends here), then the plain insert's two.  Every refusal comes before
 * the first write to the map.  Device memory on top of the insert's: two bytes per scan point (two class arrays).
 * Not here: a gate on the robust weights, gating of the record inserts (_insert_voxels, _insert_map). */
#define NGICP_GATE_NEW 0
#define NGICP_GATE_EXPLAINED 1
#define NGICP_GATE_CONFLICT 2
#define NGICP_GATE_UNJUDGED 3
typedef struct ngicp_gate_options {
  double max_mahalanobis;  /* the gate on m: >= 0, finite; DBL_MAX keeps every judged point (no default) */
  int min_voxel_count;     /* a voxel judges only with at least this many points, >= 1 (1) */
  int insert_new;          /* != 0: NEW points are kept (1) */
  int insert_unjudged;     /* != 0: UNJUDGED points are kept (1) */
  int dry_run;             /* != 0: classify only (0) */
} ngicp_gate_options;
typedef struct ngicp_gate_result {
  size_t n_points;         /* the scan's points */
  size_t n_class[4];       /* of them NEW, EXPLAINED, CONFLICT, UNJUDGED */
  size_t n_kept;
  size_t n_new, n_touched; /* voxels created; voxels of the kept points (created or added to) */
  double kernel_ms;        /* device event time, all launches of the call */
} ngicp_gate_result;
int ngicp_voxel_rolling_insert_gated(ngicp_t* h, ngicp_t* from, const float T_colmajor[16], const ngicp_gate_options* options_or_null, ngicp_gate_result* result_out_or_null);
int ngicp_voxel_rolling_insert_classes(ngicp_t* h, uint8_t* cls_n_or_null, size_t capacity, size_t* n_out_or_null);
/* LM trace of the last align(): rows of 8 doubles {outer, trial, y0, yi, rho, lambda, |d|, accepted}
 * (the columns setDebugPrint prints, impl/lsq_registration_impl.hpp:183-189). */
int ngicp_get_lm_trace(ngicp_t* h, double* rows8_or_null, size_t max_rows, size_t* n_rows);

/* --- robust kernel: Huber, Cauchy or Geman-McClure on every term (no counterpart in the reference; csrc/ngicp_terms.h robust_term,
 *     DESIGN.md 4.13) -----------------------------------------------------------------------------------------------------------------
 * The kernels and their names are this project's own definition; no fidelity to another library is claimed.
 * A TERM is one (source point, correspondence) pair: the exact route and DIRECT1 have one per source point, DIRECT7 / DIRECT27 up to K.
 * For a term, s = e^T M e, where M is the matrix the pass computes and stores - (C_B + R C_A R^T)^-1, times n_v in the voxelized mode -
 * in the order of operations of the passes' error leg.  With the width c > 0 (finite) and c2 = c * c:
 *
 *   kind                             rho(s)                                        w(s) = d rho / d s
 *   NGICP_ROBUST_NONE           0    s                                             1
 *   NGICP_ROBUST_HUBER          1    s if s <= c2, else 2 c sqrt(s) - c2           1 if s <= c2, else c / sqrt(s)
 *   NGICP_ROBUST_CAUCHY         2    c2 log1p(s / c2)                              1 / (1 + s / c2)
 *   NGICP_ROBUST_GEMAN_MCCLURE  3    s q, with q = c2 / (c2 + s)                   q q
 *
 * A term with !(s > 0) (M need not be positive definite: covariances are the caller's) is taken as under NONE: rho = s, w = 1.
 * A linearisation adds w J^T M J to H, w J^T M e to b and rho to the error; a trial (ngicp_compute_error, the error leg of a pass) adds
 * rho(s), with s from the trial pose and the STORED matrices of the last linearisation.  The stored matrices stay the unweighted M;
 * the correspondence search, the distance gate, the covariances, the LM / Gauss-Newton schedule and the convergence test are what they
 * were.  The final Hessian is the weighted H.  A term whose weight is exactly 1 contributes the same bits as under NONE.
 *
 * What the width means: s is a squared Mahalanobis distance.  With PLANE covariances M has eigenvalues of about 500 across the plane
 * and 0.5 within it, so on the exact route c = 1 is roughly 4.5 cm off the plane (1 / sqrt(500)) or 1.4 m along it.  In the voxelized
 * mode s carries the voxel's point count n_v: the same residual against a voxel of 25 points is 25 times the s, i.e. a width reaches a
 * fifth as far; widths there are chosen larger, or in view of the typical n_v at the resolution in use.
 *
 * ngicp_set_robust_kernel: an unknown kind, or with kind != NONE a width that is not finite and positive, is NGICP_ERR_ARG and changes
 * nothing.  (With NONE the width is ignored and the remembered one stays.)  The setting is remembered across mode switches (exact /
 * voxelized, neighbourhood, rolling map) and takes effect at the next ngicp_align / ngicp_linearize / ngicp_compute_error; the state of
 * the hooks stays valid, since the stored correspondences and matrices do not depend on it.
 * While kind != NONE these return NGICP_ERR_ARG (the message names the robust kernel): ngicp_align_batch, ngicp_voxel_align_batch,
 * ngicp_sharded_begin / _pass / _step / _finish, and an exact-route ngicp_align under the kernel-variant switches NGICP_PASS_IMPL=1,
 * NGICP_FUSED, NGICP_QUEUE, NGICP_PERSIST or NGICP_HEAD (the hooks under NGICP_PASS_IMPL=1): those pass variants have no robust
 * instantiation.  The voxelized align obeys none of the switches and is not refused.
 *
 * ngicp_robust_terms: for the pose T (column-major 4x4 doubles), per term, s and w under the correspondences and matrices of the last
 * linearisation - ngicp_compute_error's contract term by term - as n_src x K doubles each, row i for source point i in ORIGINAL order
 * (K = 1 on the exact route; slot order as ngicp_voxel_correspondences).  Where the slot has no correspondence, s = -1 and w = 0.  With
 * NONE every w is 1.  *K_out (may be NULL) is K; capacity_doubles < n_src * K is NGICP_ERR_ARG (K_out is set first).  Valid when
 * ngicp_get_correspondences is.  The sum of rho(s) over the terms is ngicp_compute_error(T) up to the order of the additions. */
#define NGICP_ROBUST_NONE 0
#define NGICP_ROBUST_HUBER 1
#define NGICP_ROBUST_CAUCHY 2
#define NGICP_ROBUST_GEMAN_MCCLURE 3
int ngicp_set_robust_kernel(ngicp_t* h, int kind, double width);
int ngicp_get_robust_kernel(const ngicp_t* h, int* kind, double* width);
int ngicp_robust_terms(ngicp_t* h, const double T_colmajor[16], double* s_out, double* w_out, size_t capacity_doubles, int* K_out);

/* --- pose prior: a Gaussian prior on the pose, applied in the solver (no counterpart in the reference; csrc/ngicp_math.h prior_row,
 * csrc/ngicp_solve.h lm_solve_body; restated in numpy by tests/_prior_model.py) -----------------------------------------
 * With a prior set, every route minimises  y(T) = y_data(T) + r(T)^T L r(T)  - the scaling of sum e^T M e, no factor 1/2.
 *   prior      a pose T_p = (R_p, t_p) in double and a symmetric 6x6 information matrix L, rotation first, then translation (H's
 *              order); units rad^-2, m^-2 and their mixtures.
 *   residual   at T = (R, t):  phi = log_SO3(R R_p^T),  tau = t - t_p,  r = (phi, tau).
 *   log_SO3    the inverse of the engine's so3_exp.  v = ((R - R^T)^vee) / 2, c = (tr R - 1) / 2, s2 = |v|^2.  If s2 < 1e-6 and c > 0
 *              (angles below 1e-3 rad): phi = v (1 + s2 (1/6 + s2 (3/40 + s2 15/336))); otherwise phi = v atan2(sqrt(s2), c) / sqrt(s2)
 *              (0 where s2 == 0).  Domain: rotation angles of at most 3 rad; beyond that the result is unspecified but finite.
 *   Jacobian   under the engine's update T <- (so3_exp(d[0:3]), d[3:6]) * T:  J_p = [[J_l^{-1}(phi), 0], [-[t]x, I]], with the exact
 *              inverse left Jacobian of SO(3)  J_l^{-1} = I - [phi]x / 2 + k [phi]x^2,  [phi]x^2 = phi phi^T - th2 I,  th2 = |phi|^2,
 *              k = (1 - (th/2) cos(th/2) / sin(th/2)) / th2 for th2 >= 1e-2 (0.1 rad), and below that the series
 *              k = 1/12 + th2 (1/720 + th2 (1/30240 + th2 (1/1209600 + th2 / 47900160))).
 *   a pass     evaluated at the trial pose xi gains  H += J_p^T L J_p,  b += J_p^T L r,  y0 += r^T L r,  yi += r^T L r,  all at xi:
 *              one addition per sum, made by the solver after its fixed-order reduction of the block rows.
 *   order      every one of the 28 sums is  u^T (L w) = sum_k u[k] * (sum_l L[k][l] * w[l]),  k and l ascending from 0, both sums
 *              starting from 0.0:  H(i, j), i <= j:  u = column i of J_p, w = column j of J_p;  b[i]: u = column i of J_p, w = r;
 *              the cost: u = w = r.  J_p is formed as a dense 6x6 first.  (R R_p^T)[i][j] = R[i][0] R_p[j][0] + R[i][1] R_p[j][1] + R[i][2] R_p[j][2].
 * The prior is not re-weighted by a robust kernel.  The search, the distance gate, the covariances, lambda's initialisation (which sees
 * the summed H), the convergence test and the trace format are unchanged; the final Hessian is the summed H.  ngicp_linearize and
 * ngicp_compute_error include the prior; ngicp_pose_prior_terms reports its share alone.
 *
 * ngicp_set_pose_prior: T_prior and info are column-major doubles.  A NULL T_prior clears the prior.  A non-finite entry, a last row of
 * T_prior other than (0, 0, 0, 1), an info that is not exactly symmetric or has a negative diagonal entry is NGICP_ERR_ARG and changes
 * nothing.  The setting is remembered across mode switches (exact / voxelized, neighbourhood, rolling map), leaves the state of the
 * hooks valid and takes effect at the next ngicp_align / ngicp_align_batch / ngicp_voxel_align_batch / ngicp_linearize /
 * ngicp_compute_error.  The batch entries share the one prior among their lanes; lane g equals ngicp_align(guess g) bit for bit.
 * Every kernel-variant switch whose optimiser steps in the solver's body applies the prior, bit-equal to the default route:
 * NGICP_PASS_IMPL=1, NGICP_FUSED, NGICP_QUEUE, NGICP_PERSIST, NGICP_SERIAL_STEP.  While a prior is set these return NGICP_ERR_ARG (the
 * message names the pose prior): ngicp_align under NGICP_HEAD (every block steps from its own sums there), and ngicp_sharded_begin /
 * _pass / _step / _finish.
 * ngicp_get_pose_prior: *set is 0 or 1; T and info are written only when a prior is set.  Every pointer may be NULL.
 * ngicp_pose_prior_terms: at the pose T, the residual r, the cost r^T L r, H_p = J_p^T L J_p (6x6, symmetric) and b_p = J_p^T L r,
 * evaluated on the device by the functions the solver calls.  Every output pointer may be NULL.  NGICP_ERR_STATE when no prior is set. */
int ngicp_set_pose_prior(ngicp_t* h, const double T_prior_colmajor[16], const double info_colmajor[36]);
int ngicp_get_pose_prior(const ngicp_t* h, int* set, double T_prior_colmajor[16], double info_colmajor[36]);
int ngicp_pose_prior_terms(ngicp_t* h, const double T_colmajor[16], double r[6], double* cost, double H[36], double b[6]);

/* --- more than one initial guess on the same source / target pair (no counterpart in the reference) ------------------------------
 * ngicp_align_batch: n_guesses alignments on this handle at once.  They share the source, the target, both indices, both covariance
 * sets and every parameter; each has its own initial guess.  One kernel launch per pass serves every guess still running, one solver
 * launch steps every optimiser (csrc/ngicp_batch.h).  guesses and T_out: n_guesses x 16 floats, column-major; converged and
 * nr_iterations: n_guesses ints; final_hessians_or_null: n_guesses x 36 doubles, column-major.  Guess g's outputs are bit-identical to
 * what ngicp_align(h, guesses + 16 g, ...) returns on the same handle state.  The call changes nothing an existing getter returns -
 * final transformation, convergence flag, correspondences, LM trace, Hessian and ngicp_get_stats stay those of the last ngicp_align -
 * except that it computes missing covariances, exactly as ngicp_align would.  max_iter <= 0: every guess comes back as it is.
 * Errors: as ngicp_align for a missing source or target; NGICP_ERR_ARG for n_guesses == 0, n_guesses > NGICP_BATCH_MAX_LANES, null
 * guesses, T_out, converged or nr_iterations.  The working set is ~128 bytes x source points per guess, kept and reused by the handle;
 * an allocation that fails is NGICP_ERR_HIP and leaves the handle usable.
 * When it pays (MI355X): for two or more guesses at every size measured, 10k -> 10k to 250k -> 2M points - eight guesses
 * take 1.2x the time of one at 10k points, 3.4x at 100k -> 500k, 4.2x at 250k -> 2M.  No size was found from which a loop of
 * ngicp_align calls serves the caller better; a single guess is 4-5 % faster through ngicp_align. */
#define NGICP_BATCH_MAX_LANES 64
int ngicp_align_batch(ngicp_t* h, size_t n_guesses, const float* guesses_n16_colmajor, float* T_out_n16_colmajor, int* converged_n, int* nr_iterations_n,
                      double* final_hessians_n36_colmajor_or_null);
/* ngicp_voxel_align_batch: ngicp_align_batch for a voxelized target (ngicp_set_voxel_resolution; ngicp_align_batch itself stays refused
 * while that mode is on).  n_guesses alignments on this handle at once.  They share the source, its covariances, the voxel map, the
 * neighbourhood (ngicp_set_voxel_neighbors) and every parameter; each has its own initial guess.  One kernel launch per pass serves
 * every guess still running, one solver launch steps every optimiser (csrc/ngicp_voxel_batch.h).  The arrays are ngicp_align_batch's.
 * Guess g's transform, convergence flag, iteration count, Hessian and LM trace are bit-identical to what ngicp_align(h, guesses + 16 g,
 * ...) returns on the same handle state with the voxel mode on, for DIRECT1, DIRECT7 and DIRECT27, LM and Gauss-Newton.  The call
 * changes nothing an existing getter returns - final transformation, convergence flag, iteration count, Hessian,
 * ngicp_get_correspondences, ngicp_voxel_correspondences, the state ngicp_compute_error evaluates, ngicp_get_lm_trace and
 * ngicp_get_stats stay those of the last ngicp_align - except that it computes missing covariances and rebuilds a stale voxel map, once
 * per call and not per guess, exactly as ngicp_align would (ngicp_voxelmap_builds then grows by one, and ngicp_stats::voxelmap_ms is
 * that build's).  max_iter <= 0: every guess comes back as it is and no pass is launched.
 * Errors: NGICP_ERR_STATE while the voxel mode is off (as ngicp_voxelmap_size); as ngicp_align for a missing source or target;
 * NGICP_ERR_ARG for n_guesses == 0, n_guesses > NGICP_BATCH_MAX_LANES, null guesses, T_out, converged or nr_iterations.  The working set
 * is 2 * K * 52 bytes per source point PER GUESS (K = 1, 7, 27: the voxel numbers and n_v M of both ping-pong halves), grow-only, kept
 * and reused by the handle and separate from the single alignment's: DIRECT27 with 64 guesses on 100k source points is about 18 GB.  An
 * allocation that fails is NGICP_ERR_HIP and leaves the handle usable.
 * Measured (MI355X): at 20k -> 60k and 100k -> 500k points with 2 and 8 guesses, faster than a loop of ngicp_align calls in
 * every case - 4.8x for eight guesses under DIRECT1 on the small pair, 1.1x for two under DIRECT27 on the large one. */
int ngicp_voxel_align_batch(ngicp_t* h, size_t n_guesses, const float* guesses_n16_colmajor, float* T_out_n16_colmajor, int* converged_n, int* nr_iterations_n,
                            double* final_hessians_n36_colmajor_or_null);
/* LM trace of guess `lane` of the last batch call of either entry, ngicp_align_batch or ngicp_voxel_align_batch: rows as
 * ngicp_get_lm_trace.  Valid until the next call of either or a change of the source or target. */
int ngicp_batch_get_lm_trace(ngicp_t* h, size_t lane, double* rows8_or_null, size_t max_rows, size_t* n_rows);
/* ngicp_fitness_score for n transforms in one launch (n x 16 floats, column-major): scores[i] and n_inliers[i] are bit-identical to
 * ngicp_fitness_score(h, T + 16 i, max_range, ...).  The recipe for several candidate poses: align the batch, score the results, take
 * the lowest score. */
int ngicp_fitness_score_batch(ngicp_t* h, size_t n, const float* T_n16_colmajor, double max_range, double* scores_n, size_t* n_inliers_n_or_null);

/* --- voxel fitness: poses scored against the voxel map the handle aligns against (no counterpart in the reference;
 *     csrc/ngicp_voxel_fitness.h) -----------------------------------------------------------------------------------
 * ngicp_fitness_score needs a target cloud and its exact index; a handle on a rolling voxel map has neither.  These entries score a
 * pose against the voxel map itself - the target's, the merged one, or the rolling one - and say how much of the source it explains.
 * The definition is the project's own:
 *   inputs     a float 4x4 pose T (column-major; NULL where allowed: the final transformation of the last align); the source with its
 *              covariances, computed if missing exactly as ngicp_align does; the voxel map as ngicp_align would use it (built if stale,
 *              at most once per call; the rolling map while that setting is on, an empty one being NGICP_ERR_STATE); the resolution and
 *              the neighbourhood K (1, 7 or 27) in force.
 *   the point  q = the float pose times the source point a in the passes' order, ((c0 x + c1 y) + c2 z) + c3 per row, nothing fused;
 *              its cell is floorf(q * inv_res) as everywhere in the voxelized mode.
 *   the slots  slot s = 0..K-1 is voxel c + off[s] under the passes' rule (see "voxelized GICP"): the centre and the neighbour in range
 *              on the integers, the voxel occupied.  A point without an occupied slot is UNMATCHED.
 *   a term     of an occupied slot, in FP64 with nothing fused, R and t being the float entries of T widened to double:
 *              e = mean_v - (R a + t), M = (cov_v + R C_a R^T)^-1 (the passes' routines in the passes' order of operations),
 *              m_s = e^T M e - the pass's term WITHOUT the factor n_v - and d_s = (ex ex + ey ey) + ez ez.
 *   the value  of a point: best = +inf; in ascending slot, slot s wins when m_s < best (ties go to the lower slot, a NaN never wins);
 *              (m, d, v) are those of the winning slot, v its voxel number (ngicp_voxelmap_get / ngicp_voxel_rolling_get order).  A
 *              matched point without a winner (every term non-finite) has m = d = +inf, v = -1: matched, never an inlier.
 *   counting   a point is an INLIER iff m <= max_mahalanobis (pass DBL_MAX for no gate; NaN or negative: NGICP_ERR_ARG).  Per pose:
 *              n_matched, n_inliers, mahalanobis = (sum of m over the inliers) / n_inliers, sqdist = (sum of d) / n_inliers, both
 *              DBL_MAX when there is no inlier.  n_matched / n_src is the overlap.
 * The sums are fixed-order FP64 reductions (a lane's value, the wave's butterflies, the block's waves in order, the blocks strided per
 * thread of one block and reduced the same way): bitwise reproducible, pose i of a batch is bit for bit the single call, and nothing
 * depends on n or on how the poses are cut into launches.  The robust kernel, the pose prior and max_correspondence_distance are not
 * consulted, and nothing is refused because they are set.  The calls leave the hooks' state (ngicp_compute_error, the correspondences),
 * the results, trace and stats of the last ngicp_align and the lanes and traces of the last batch call untouched.
 * Errors: voxel mode off NGICP_ERR_STATE; no source as ngicp_align; empty rolling map NGICP_ERR_STATE; n == 0, a null pointer, a short
 * capacity or a bad gate NGICP_ERR_ARG.  Everything passed in is checked before anything is enqueued. */
typedef struct ngicp_voxel_fitness {
  double mahalanobis, sqdist;
  size_t n_inliers, n_matched;
} ngicp_voxel_fitness_t;
int ngicp_voxel_fitness(ngicp_t* h, const float T_colmajor_or_null[16], double max_mahalanobis, ngicp_voxel_fitness_t* out);
/* n poses (n x 16 floats, column-major; any n: a launch takes at most 4096) -> out[n] */
int ngicp_voxel_fitness_batch(ngicp_t* h, size_t n, const float* T_n16_colmajor, double max_mahalanobis, ngicp_voxel_fitness_t* out_n);
/* The per-point values of one pose in ORIGINAL source order, capacity >= n_src entries each: unmatched points come out as
 * m = -1, d = -1, v = -1 (the convention of ngicp_robust_terms).  No gate applies. */
int ngicp_voxel_fitness_points(ngicp_t* h, const float T_colmajor_or_null[16], double* m_out, double* sqd_out, int* voxel_out, size_t capacity);
/* device time (HIP events on the handle's stream) of the kernels of the last call of any of the three, all launches together;
 * kept here and not in ngicp_stats, which these calls leave alone */
int ngicp_voxel_fitness_kernel_ms(const ngicp_t* h, double* ms);

/* --- scan context: which earlier keyframe does this scan revisit, and at what yaw (no counterpart in the reference;
 *     csrc/ngicp_scan_context.h) ------------------------------------------------------------------------------------
 * A polar height descriptor of a scan in the manner of Scan Context (Kim & Kim, IROS 2018), a device-resident database of such
 * descriptors (one per keyframe) and an exhaustive match of a query against a range of the database over every column shift.  The
 * definition is this project's own, written so that a host restates it bit for bit (tests/_scan_context_model.py); no fidelity to any
 * outside implementation is claimed.  There is no pruning stage (no ring key, no tree): every candidate is matched at every shift.
 *   parameters  n_rings R in 1..64, n_sectors S even in 2..64, max_radius L > 0 finite, z_offset z0 finite; defaults 20, 60, 80.0f, 2.0f.
 *   tables      built on the host once per parameter change: ring edges e_k = (float)((double)L * k / R) and E2_k = e_k * e_k in float,
 *               k = 0..R; sector boundary directions b_k = ((float)cos(2 pi k / S), (float)sin(2 pi k / S)), k = 0..S/2-1, computed in
 *               double.  ngicp_scan_context_tables returns both (E2: R + 1 floats; b: S floats, x and y interleaved).
 *   a point     (x, y, z) float.  A non-finite coordinate: skipped.  r2 = x*x + y*y (two rounded products, one addition, nothing
 *               fused); skipped unless r2 < E2_R.  ring = the number of k in 1..R-1 with r2 >= E2_k.  low = y < 0 || (y == 0 && x < 0);
 *               (xs, ys) = low ? (-x, -y) : (x, y).  sector = the number of k in 1..S/2-1 with b_k.x * ys - b_k.y * xs >= 0 (two rounded
 *               products, one subtraction), plus S/2 if low - a COUNT, not a search: it stays defined where rounding breaks monotonicity
 *               near a boundary.  v = z + z0 in float.
 *   descriptor  D[R][S] floats, row-major by ring; every cell starts at 0.0f; D[ring][sector] = max(D[ring][sector], v).  A maximum does
 *               not depend on order: the descriptor is deterministic.  Cells are >= 0.
 *   norms       n_j = sqrt(sum_r (double)D[r][j] * (double)D[r][j]), r ascending from 0.0, the root correctly rounded.
 *   distance    of query Q to candidate C at shift k (0 <= k < S), all in double: with j' = (j + k) mod S, column j counts iff
 *               nq_j > 0 && nc_j' > 0; its term is (sum_r (double)Q[r][j] * (double)C[r][j']) / (nq_j * nc_j'), r ascending from 0.0;
 *               d_k = 1.0 - (sum of the counted terms, j ascending from 0.0) / (double)m for m counted columns, 1.0 when m = 0.
 *               dist(Q, C) = min_k d_k and shift = the smallest k that attains it (a scan with k ascending under strict <).
 *   the shift   column j of the query lies on column j + k of the candidate: if the query scan was taken at the candidate's place with
 *               the sensor yawed by psi, k is about psi / (2 pi / S), and the guess that carries the query scan into the candidate's
 *               frame is a rotation about z by k * 2 pi / S.
 *   ranking     candidates ascending by (distance, id).
 * which: as ngicp_range_select defines it (0 source, 1 target, 2 the preprocessed scan; non-finite rows left in it are skipped), with its
 * state errors.  A query is EITHER a slot (which 0..2 and desc_or_null NULL) OR a host descriptor (which -1 and R * S floats).  Host
 * descriptors must be finite and >= 0, else NGICP_ERR_ARG.  Ids are dense in insertion order, like keyframe ids.
 * Everything passed in is checked before anything is enqueued; a refused call changes nothing.  None of these entries changes what any
 * existing getter returns: scratch of their own; hooks, results, stats and batch traces are left alone. */
/* A refused value is NGICP_ERR_ARG and changes nothing; an accepted CHANGE clears the database (as a change of resolution clears the
 * rolling map); setting the values in force is a no-op. */
int ngicp_scan_context_set_params(ngicp_t* h, int n_rings, int n_sectors, float max_radius, float z_offset);
int ngicp_scan_context_get_params(const ngicp_t* h, int* n_rings, int* n_sectors, float* max_radius, float* z_offset);
int ngicp_scan_context_tables(ngicp_t* h, float* E2_out_R_plus_1, float* b_out_S);
/* the descriptor of a slot's cloud, R * S floats to the host; a cloud whose points are all skipped gives the all-zero descriptor */
int ngicp_scan_context_compute(ngicp_t* h, int which, float* desc_out);
/* compute the descriptor and append it, with its column norms, without leaving the device / append a host descriptor */
int ngicp_scan_context_add(ngicp_t* h, int which, int* id);
int ngicp_scan_context_add_descriptor(ngicp_t* h, const float* desc, int* id);
int ngicp_scan_context_count(const ngicp_t* h, size_t* n);
int ngicp_scan_context_get(ngicp_t* h, int id, float* desc_out);
int ngicp_scan_context_clear(ngicp_t* h);
/* distance and shift of the query to every entry of [id_begin, id_end): id_end - id_begin values each, one launch, one read-back.
 * id_end > count or id_begin > id_end is NGICP_ERR_ARG; an empty range writes nothing and succeeds. */
int ngicp_scan_context_distances(ngicp_t* h, int which_or_minus1, const float* desc_or_null, size_t id_begin, size_t id_end, double* dist_out, int* shift_out);
/* the first min(top_k, id_end - id_begin) entries of the ranking, selected on the device (top_k in 1..64; the outputs hold top_k
 * entries); *n_out = their number, 0 for an empty range */
int ngicp_scan_context_match(ngicp_t* h, int which_or_minus1, const float* desc_or_null, size_t id_begin, size_t id_end, int top_k, int* ids_out, double* dist_out,
                             int* shift_out, size_t* n_out);
/* device time of the kernels of the last compute / add / distances / match call (as ngicp_voxel_fitness_kernel_ms) */
int ngicp_scan_context_kernel_ms(const ngicp_t* h, double* ms);

/* --- voxel pose search: which translation (and which of several orientations) puts the source on the voxel map (no counterpart in
 *     the reference; csrc/ngicp_pose_search.h) ---------------------------------------------------------------------
 * Correlative scan matching in the manner of Olson (ICRA 2009): an exhaustive search over a lattice of poses - B base poses times a
 * window of whole-voxel shifts - each scored by the number of source points that land in occupied voxels; the best few come back and
 * are meant for ngicp_voxel_align_batch.  The score is an integer: sums are order-free, the result is deterministic and a host
 * restates it exactly (tests/_pose_search_model.py).  The definition is the project's own:
 *   inputs     B >= 1 base poses T_b (float 4x4, column-major); integer extents ex, ey, ez >= 0; top_k in 1..64; the source cloud (its
 *              covariances are neither needed nor computed); the voxel map exactly as ngicp_voxel_fitness takes it (the target's, the
 *              merged one or the rolling one; built if stale, at most once per call; an empty rolling map is NGICP_ERR_STATE).
 *   the cell   c_b(p) = floorf(q * inv_res) of q = the float pose T_b times the source point p in the passes' order,
 *              ((c0 x + c1 y) + c2 z) + c3 per row, nothing fused - as everywhere in the voxelized mode.  A point with a component at or
 *              beyond 2^20 cells, or a NaN coordinate, has no cell.  A source cloud cannot hold a non-finite point (it is refused when
 *              it is set), so q is NaN or infinite only through the pose: unlike most entries this one does NOT refuse a non-finite
 *              T_b - the poses are not inspected on the host - and such a pose simply scores 0 wherever its points lose their cells.
 *   shifts     s = (sx, sy, sz) with |sx| <= ex, |sy| <= ey, |sz| <= ez; the index of a shift is
 *              ((sz + ez)(2 ey + 1) + (sy + ey))(2 ex + 1) + (sx + ex); |S| = (2 ex + 1)(2 ey + 1)(2 ez + 1) is their number.
 *   score      score[b][s], int32 = the number of source points that have a cell, for which every component of c_b(p) + s lies strictly
 *              inside (-2^20, 2^20) (the passes' neighbour rule), and whose voxel c_b(p) + s is in the map's table.  Duplicate points
 *              count each time.  The neighbourhood setting (DIRECT1 / 7 / 27) is not consulted.
 *   on cells   The score is defined ON CELLS: it moves the point's cell by s.  The float pose T_b translated by s * res may put a point
 *              that lies near a cell border into another cell, so ngicp_voxel_fitness at a candidate pose need not report exactly
 *              score[b][s] matched points.  At s = 0 it does: score[b][0] equals n_matched of ngicp_voxel_fitness_batch under DIRECT1
 *              at T_b.
 *   ranking    descending score, then ascending b, then ascending shift index; the result is the first min(top_k, B |S|) entries,
 *              selected on the device, with one read-back.
 *   candidate  the pose of entry (b, s), computed on the host by the caller (the C++ shim and the Python wrapper do): T_b with its
 *              translation replaced, per axis, by (float)((double)t + (double)s * res), res the voxel resolution as a double.
 *   caps       ex, ey <= 31 (a row of shifts is at most 63 bits wide), ez <= 7, |S| <= 12288 (48 KB of int32 in LDS), B |S| <= 2^24.
 *              Anything beyond a cap is NGICP_ERR_ARG before anything is enqueued; tile a larger window with more base poses (sub-voxel
 *              steps likewise: base poses offset by a fraction of a voxel).
 * How: the map's cell bounding box and the source's over all base poses are computed on the device and read back together; the host
 * plans a dense occupancy bit grid over map box INTERSECTED WITH (source box dilated by the extents), x along the bits of 64-bit words,
 * rows padded with guard words; a grid beyond 256 MiB is NGICP_ERR_ARG (the one refusal that comes after kernels have run; it still
 * changes nothing).  An empty intersection gives all-zero scores, ranked by index.
 * A query: the robust kernel, the pose prior and max_correspondence_distance are not consulted and nothing is refused because they
 * are set; the hooks' state, the results, trace and stats of the last ngicp_align and the lanes and traces of the last batch call are
 * left untouched.  Errors: voxel mode off NGICP_ERR_STATE; no source as ngicp_align; empty rolling map NGICP_ERR_STATE; n_poses == 0, a
 * null pointer, a cap or a bad top_k NGICP_ERR_ARG.  A refused call changes nothing.
 * Outputs hold top_k entries each (shift_out_xyz: 3 ints per entry); *n_out = the number written. */
int ngicp_voxel_pose_search(ngicp_t* h, size_t n_poses, const float* T_n16_colmajor, int ex, int ey, int ez, int top_k, int* pose_out, int* shift_out_xyz, int* score_out,
                            size_t* n_out);
/* The full volume of the last successful search, [B][2 ez + 1][2 ey + 1][2 ex + 1] int32 (the shift index order), capacity >= B |S|
 * entries.  NGICP_ERR_STATE when there has been no search, or when the map has changed since (an insert, evict, clear, restore or move of
 * the rolling map; another target, resolution or map setting). */
int ngicp_voxel_pose_search_scores(ngicp_t* h, int* out, size_t capacity);
/* device time of the kernels of the last search: the two box kernels, and - behind their read-back - the grid fill, the score kernel
 * and the top-k levels (as ngicp_voxel_fitness_kernel_ms) */
int ngicp_voxel_pose_search_kernel_ms(const ngicp_t* h, double* ms);

/* The small FP64 routines of the engine evaluated on the device, one problem per thread (unit-test hook): which = 0 so3_exp
 * (gicp/so3.hpp:99-118 followed by Quaternion::toRotationMatrix; in: 3 doubles, out: R row-major 9), 1 the 6x6 LDLT solve that
 * stands in for Eigen::LDLT (impl/lsq_registration_impl.hpp:147-148,172-173; in: A row-major 36 + rhs 6, out: 6), 2 the
 * symmetric 3x3 eigen-decomposition that stands in for JacobiSVD (impl/nano_gicp_impl.hpp:332; in: {xx,xy,xz,yy,yz,zz}, out:
 * w 3 + V row-major 9), 3 the symmetric 3x3 inverse (impl/nano_gicp_impl.hpp:205-209; in 6, out 6), 4 so3_log ("pose prior"; in: R
 * row-major 9, out: 3), 5 the pose prior's row (in: pose R row-major 9 + t 3, prior R_p row-major 9 + t_p 3 + L row-major 36; out: H's
 * upper triangle row by row 21 + b 6 + the cost 1). */
int ngicp_math_selftest(ngicp_t* h, int which, const double* in, size_t n_problems, double* out);
/* One step of the optimiser on the device in both of its forms (unit-test hook): the serial step on one lane and the wave-level step the
 * solver runs by default (NGICP_SERIAL_STEP=1 selects the serial one), from the same state, sums and configuration.  in: 132 doubles
 * per problem - x0 12, xi 12, delta 12 (each R row-major 9, t 3), H 36, b 6, y0, d 6, lambda, nu, then iter, trial, have_lin, cur,
 * n_trace, lin_unneeded, then max_iterations, lm_max_iterations, optimizer, rot_eps, trans_eps, lm_init_lambda_factor, then the 32
 * reduced sums of the pass (H upper triangle 21, b 6, y0, yi, three counters), then `searched`.  out: per problem two records of
 * *record_bytes bytes, serial then wave: the state image after the step (it begins with the 87 doubles x0 .. nu in the input's order;
 * record_bytes - 144 bytes in all), the LM trace row (8 doubles, written when n_trace == 0),
 * d (6 doubles) and {done, converged, lm_failed, trial} as doubles.  out_or_null == NULL: only *record_bytes is set. */
int ngicp_step_selftest(ngicp_t* h, const double* in, size_t n_problems, unsigned char* out_or_null, size_t* record_bytes);

/* --- measurement ----------------------------------------------------------- */
typedef struct ngicp_stats {
  double align_ms;          /* host wall time of the last ngicp_align() */
  double loop_ms;           /* device time (HIP events on the handle's stream) of the iteration loop */
  double pass_ms_total;     /* device time (HIP events on the handle's stream) summed over the k_gicp_pass launches of the
                               last align that did work; only collected while ngicp_set_profiling(h, 1) */
  int passes;               /* per-iteration kernels launched that did work (= lm_trials + 1 under LM; see search_passes) */
  int outer_iterations;     /* nr_iterations_ + 1 */
  int lm_trials;            /* LM trials evaluated */
  double mean_candidates;   /* C-bar: target points distance-tested per source point per pass that searched */
  double valid_fraction;    /* fraction of source points with a correspondence, mean over the passes that searched */
  double index_build_ms;    /* device time of the last index build on this handle */
  double covariance_ms;     /* device time of the last covariance computation */
  double upload_ms;         /* host wall time of the last cloud upload */
  double voxel_size;        /* target grid voxel edge in use */
  int grid_dims[3];
  int lanes_per_query;
  int passes_timed;         /* launches covered by pass_ms_total */
  long long n_src, n_tgt;   /* cloud sizes of the last align */
  double staged_fraction;   /* fraction of queries served through the LDS row index of their batch region (mean over the passes that searched) */
  double submap_ms;         /* host wall time of the last ngicp_submap_set() that rebuilt the target (enqueue + index build) */
  long long device_allocs;  /* hipMalloc calls made by this process's engine buffers so far (a call that grows a buffer in the middle of
                               a frame shows up as a latency outlier: two readings around a call attribute it) */
  long long host_wait_spins; /* polls of the solver's progress word during the last ngicp_align() (busy or yielding, see below) */
  double query_ms;          /* device time (HIP events on the handle's stream) of the kernels of the last knn / radius / fitness / range query */
  double voxelmap_ms;       /* device time of the last voxel-map build (voxelized GICP) */
  int search_passes;        /* passes that searched and linearised.  < passes where the route's pass kernel evaluates only the trial's
                               error in a pass whose linearisation could never be adopted (the trial can only end the alignment:
                               its step already meets the convergence test, or it belongs to the last outer iteration); the
                               denominator of mean_candidates, valid_fraction and staged_fraction */
} ngicp_stats;
int ngicp_get_stats(ngicp_t* h, ngicp_stats* out);
/* HIP-event timing of the k_gicp_pass launches inside align (two event records per timed launch; off by default).
   on = 1: every launch; on = N > 1: every N-th launch (an event between two kernels costs a few microseconds of stream time) */
int ngicp_set_profiling(ngicp_t* h, int on);

/* --- point-sharded multi-GPU stepping ------------------------ */
/* One alignment whose SOURCE points are split over ranks (each rank's handle holds its block of the source, the whole target
 * and both covariance sets).  Per pass: ngicp_sharded_pass runs the fused pass over this rank's block at the engine's current
 * trial pose and leaves 32 doubles {H upper-tri 21, b 6, y0, yi, candidates tested, valid correspondences, listed queries} in
 * device memory `sums32_dev`; the caller all-reduces them (RCCL through torch.distributed: 256 B, latency-bound);
 * ngicp_sharded_step feeds the reduced sums to the LM state machine, which advances identically on every rank (what is
 * reduced is the reference's own per-thread partial sum, impl/nano_gicp_impl.hpp:260-267).  Nothing synchronises the host per
 * pass: *done reports the state as of TWO steps earlier (a constant lag, so that every rank leaves the loop in the same step -
 * a rank that stopped calling the collective before its peers would hang them); the two passes after the end do nothing.
 * All calls of one alignment must use the same stream (NULL: the handle's own). */
int ngicp_sharded_begin(ngicp_t* h, const float guess_colmajor[16]);
int ngicp_sharded_pass(ngicp_t* h, double* sums32_dev, void* hip_stream_or_null);
int ngicp_sharded_step(ngicp_t* h, const double* sums32_dev, void* hip_stream_or_null, int* done);
int ngicp_sharded_finish(ngicp_t* h, float T_out_colmajor[16], int* converged, int* nr_iterations, double final_hessian_colmajor[36]);
/* K1 sharded the same way ("K1 shards the same way with an all-gather of the packed covariances"; the loop being split is
 * impl/nano_gicp_impl.hpp:309-354).  Every rank holds the whole cloud (the k-NN of a point looks at all of it) and the same index
 * (the build is deterministic), so the packed covariance array [n][6] FP64 has the same layout on every rank: rank r computes the
 * rows of the points at sorted positions [lo, hi) of the source (which = 0) or target (which = 1) cloud in place, the caller
 * all-gathers the blocks (RCCL through torch.distributed on the device pointer *covs6_dev, n * 6 doubles) and commits the set.
 *   ngicp_covs_shard_begin    allocates the set (uncommitted: align() will not use it) and returns its device pointer and n
 *   ngicp_covs_shard_compute  computes the block [lo, hi) (sorted positions) on the handle's stream, or on `stream` if given
 *   ngicp_covs_shard_commit   the set becomes the cloud's covariances (as after ngicp_compute_*_covs) */
int ngicp_covs_shard_begin(ngicp_t* h, int which, double** covs6_dev, size_t* n_points);
int ngicp_covs_shard_compute(ngicp_t* h, int which, size_t lo, size_t hi, void* hip_stream_or_null);
int ngicp_covs_shard_commit(ngicp_t* h, int which);

/* --- device-resident keyframe store + submap assembly ------------ */
/* DLO keeps every keyframe twice on the host: its cloud (`keyframes`, src/dlo/odom.cc:1166) and its covariances
 * (`keyframe_normals`, odom.cc:1172-1174, computed by gicp_s2s used as a covariance service), and on every change of the
 * selected keyframe set concatenates both (odom.cc:1318-1325) and hands them to gicp (odom.cc:830-833): a re-upload, a
 * re-index and a 128 B/point covariance image per change.  Here the keyframes stay on the device:
 *   ngicp_keyframe_add(h, from, &id)   replaces odom.cc:1174: h's store adopts `from`'s current SOURCE cloud (already uploaded
 *                                      and indexed by setInputSource, odom.cc:1172) and its source covariances (computed with
 *                                      `from`'s k / regularisation if not yet present, odom.cc:1173).  No copy.  `from` may be h.
 *   ngicp_keyframe_add_transformed     replaces odom.cc:971-974 + 1166-1174 when the submap voxel filter is off: the keyframe is
 *                                      `from`'s current source cloud (the scan, already on the device) transformed by the float
 *                                      matrix T (pcl::transformPointCloud), indexed and given covariances with `from`'s k, all
 *                                      on the device.  `from`'s own source slot is left untouched.
 *   ngicp_submap_set(h, ids, n, &chg)  replaces odom.cc:1318-1325 + 830-833: target := the keyframes ids[0..n) concatenated in
 *                                      that order (point g = offset_k + original index inside keyframe k, exactly the host
 *                                      concatenation), target covariances := their covariances likewise; one index build, no
 *                                      host traffic.  A call with the id list the current target was built from is a no-op
 *                                      (*chg = 0), like the submap_hasChanged test (odom.cc:827,1308).
 * Keyframe ids are dense, in insertion order (the index DLO uses for `keyframes[k]`). */
int ngicp_keyframe_add(ngicp_t* h, ngicp_t* from, int* id_out);
int ngicp_keyframe_add_transformed(ngicp_t* h, ngicp_t* from, const float T_colmajor[16], int* id_out);
/* The same for DLO's SHIPPED configuration (cfg/params.yaml:33-35: voxelFilter.submap.use = true, res = 0.5), where the transformed
 * scan is voxel-filtered BEFORE it becomes a keyframe (src/dlo/odom.cc:1160-1163): replaces odom.cc:971-974 + 1160-1174.  The
 * keyframe is pcl::VoxelGrid(leaf) of `from`'s current source cloud transformed by T - transform (in the scan's original point
 * order), centroids, index build and covariances all on the device.  leaf <= 0 is ngicp_keyframe_add_transformed. */
int ngicp_keyframe_add_transformed_filtered(ngicp_t* h, ngicp_t* from, const float T_colmajor[16], float leaf, int* id_out);
int ngicp_keyframe_count(const ngicp_t* h, size_t* n);
int ngicp_keyframe_size(const ngicp_t* h, int id, size_t* n_points);
int ngicp_keyframe_clear(ngicp_t* h);
int ngicp_submap_set(ngicp_t* h, const int* ids, size_t n_ids, int* changed_out_or_null);
/* the target cloud as the engine holds it, in ORIGINAL point order (for a device-assembled submap: the concatenation).
 * xyz_out may be NULL to query the size only. */
int ngicp_get_target_points(ngicp_t* h, float* xyz_out_or_null, size_t out_stride_bytes, size_t* n_out_or_null);

/* --- moving keyframes: re-pose keyframes of the store after a loop closure, and read one back (no counterpart in the reference, which
 *     keeps its keyframes on the host; csrc/ngicp_keyframe_move.h) ------------------------------------------------------
 * A keyframe is held in the world frame at the pose it was added with.  After a pose-graph correction ngicp_keyframe_transform applies a
 * rigid correction to any subset of the store, on the device, in one kernel launch; ngicp_keyframe_get hands a keyframe to the host.  The
 * project's own definition, every operation spelled out (tests/_keyframe_move_model.py restates it; the engine is held to it bit for bit):
 *   the points        of keyframe ids[j] under the float matrix T_j (column-major):  p' = T_j p  as pcl::transformPointCloud,
 *                     x*c0 + (y*c1 + (z*c2 + c3)) per row in float32, nothing fused.  A point keeps its original index.
 *   the covariances   C' = R_j C R_j^T with R_j the float 3x3 block of T_j widened to double, evaluated as the rolling insert evaluates it:
 *                     RA = R C row by row, each entry (r0 a0 + r1 a1) + r2 a2, then the upper triangle of RA R^T the same way, in FP64.
 *                     One rotation per point.  The covariances are NOT recomputed from the moved points: under a rigid motion a
 *                     regularised covariance keeps its eigenvalues, and no neighbour search runs.
 *   the box           the exact float min / max of the moved points.
 *   the voxel part    (merged voxel map) is dropped and rebuilt lazily from the moved points and covariances.
 *   copy on move      a keyframe may share its buffers with a producer's source slot (ngicp_keyframe_add adopts them without a copy): a
 *                     move always writes fresh buffers and swaps them in at the end.  Nothing another handle or slot sees changes.  PEAK
 *                     DEVICE MEMORY IS TWICE THE MOVED KEYFRAMES (64 bytes per point more until the call returns).
 *   no index          nothing searches a keyframe, so a moved keyframe keeps its storage order and gets no index build: its points
 *                     (16 bytes each) and covariances (48) are all it holds from then on.  Later index builds on the handle behave as if the move had not happened.
 *   the target        is not touched: it owns its buffers; its points, covariances, voxel map, correspondences, the hooks' state and the
 *                     last alignment's results stay bit for bit.  If a moved id is in the list the current target was built from, the
 *                     no-op memo of ngicp_submap_set is forgotten and *submap_stale_out = 1: the next ngicp_submap_set, even with the
 *                     same list, rebuilds and reports changed = 1.  Otherwise the memo stays and *submap_stale_out = 0.
 *   all or nothing    NGICP_ERR_ARG, and nothing changes (keyframes, voxel parts, the memo, the target), for: null ids or T, n_ids == 0;
 *                     an unknown id; an id listed twice (the message names both positions); a matrix entry that is not finite; a last row
 *                     other than (0, 0, 0, 1); any moved coordinate that is not finite (found on the device, with a flag of its own).
 *                     Rigidity is not checked, as by no other entry that takes a float pose.
 * One host synchronisation per call (the boxes and the flag are read back before the swap).  Moving a keyframe twice is two roundings,
 * not the rounding of the composed matrix.
 * ngicp_keyframe_get: the keyframe's points in ORIGINAL point order (what ngicp_get_target_points gives for a one-keyframe submap) and its
 * covariances as ngicp_get_source_covs formats them (n x 16 doubles, column-major 4x4, last row and column zero, original order).
 * Either array may be NULL.  Unknown id, or (with xyz_out) a stride below 12 or not a multiple of 4: NGICP_ERR_ARG. */
int ngicp_keyframe_get(ngicp_t* h, int id, float* xyz_out_or_null, size_t out_stride_bytes, double* covs_n16_or_null, size_t* n_out_or_null);
int ngicp_keyframe_transform(ngicp_t* h, const int* ids, size_t n_ids, const float* T_colmajor_n16, int* submap_stale_out_or_null);
/* device time (HIP events on the handle's stream) of the kernel of the last ngicp_keyframe_transform that ran one, refused or not */
int ngicp_keyframe_transform_kernel_ms(const ngicp_t* h, double* ms);

/* --- pose graph: turn loop-closure edges into corrected keyframe poses, on the device (no counterpart in the reference;
 *     csrc/ngicp_pose_graph.h, csrc/ngicp_pose_graph_plan.h) -----------------------------------------------------------
 * The step between "scan j is keyframe i, at this relative pose, with this information" (ngicp_scan_context_match, ngicp_voxel_pose_search,
 * ngicp_voxel_align_batch, the final Hessian) and ngicp_keyframe_transform / ngicp_voxel_rolling_transform.  The graph lives on the
 * handle, survives alignments and is independent of the clouds.  The project's own definition, restated by tests/_pose_graph_model.py:
 *   nodes         world poses T_k = (R_k, t_k) in FP64, column-major 4x4 with last row (0, 0, 0, 1).  Ids are dense, in order of insertion
 *                 (as the scan-context database's).  Each node has a `fixed` flag.
 *   edges         (i, j, Z, Lambda, robust flag): Z the measured T_i^-1 T_j (column-major 4x4), Lambda a symmetric 6x6 information matrix
 *                 (row-major; rotation first, then translation - the project's twist order).  Ids dense, in order of insertion.
 *   residual      E = Z^-1 T_i^-1 T_j,  r = (so3_log(R_E), t_E).  so3_log (csrc/ngicp_math.h) is valid to 3 rad: a residual rotation
 *                 beyond that gives a finite but unspecified result - start an optimisation closer than that.
 *   perturbation  the project's own: T_k <- (so3_exp(d[0:3]), d[3:6]) * T_k.  With A = Z^-1 T_i^-1 the exact Jacobians are
 *                 J_j = [[Jl^-1(phi) R_A, 0], [-R_A [t_j]x, R_A]] and J_i = -J_j (DESIGN.md 4.22 derives them).
 *   cost          chi2 = sum_e rho(s_e), s_e = r_e^T Lambda_e r_e.  rho is the identity unless the edge's robust flag is set AND a kernel is
 *                 chosen for the graph (ngicp_pose_graph_set_robust: NGICP_ROBUST_*, width c; the functions of "robust kernel" above).  The
 *                 weight w(s_e) then scales Lambda_e in the normal equations (iteratively re-weighted least squares, as the passes do).
 *                 Flag loop edges and leave odometry edges unflagged, and one false loop edge cannot fold the map.
 *   gauge         columns of fixed nodes are dropped.  ngicp_pose_graph_optimize refuses (NGICP_ERR_ARG, nothing changed) while any connected
 *                 component of the graph holds no fixed node (a node without edges is a component of its own).
 *   refused       at add time, all or nothing per call, NGICP_ERR_ARG: n == 0 or a null array; a self-edge; an unknown node id; an entry that
 *                 is not finite; a last row other than (0, 0, 0, 1); an asymmetric Lambda - mirrored entries must be EXACTLY equal; more
 *                 than 2^20 nodes or 2^22 edges in the graph.  Several edges between one pair, and an edge given as (j, i) with j > i, are legal.
 *   optimise      Levenberg-Marquardt on the whole graph with the aligner's schedule (csrc/ngicp_lm.h): H + lambda I; the first lambda is
 *                 1e-9 times the largest diagonal entry of H; a rejected try multiplies lambda by nu (2, doubling); an accepted one by
 *                 max(1/3, 1 - (2 rho - 1)^3); a try is accepted unless its gain ratio rho is negative; ten tries per outer iteration.
 *                 It stops after max_iterations outer iterations, or when a try's largest per-node |so3_exp(d_w) - I| entry is below rot_eps
 *                 and its largest |d_t| entry below trans_eps (is_converged's two thresholds), or when ten tries in a row were rejected.
 *                 An accepted step changes the poses; a call that runs out of tries leaves the last accepted poses.
 *   linear solve  (H + lambda I) delta = -b by conjugate gradients from delta = 0, preconditioned by the inverses of the damped 6x6
 *                 diagonal blocks (ldlt6_solve), stopped when |res| <= cg_tol |b| or after cg_max_iterations; decided on the device.
 *   determinism   every sum has a written order (per node: its incident edges in ascending edge id; dot products: a fixed tree); no
 *                 floating-point atomics.  Two runs on the same input are bit-equal.
 * ngicp_pose_graph_linearize (test hook; the poses stay): chi2; per edge r (m x 6) and (s, w) (m x 2); per node the gradient (n x 6) and the
 * diagonal block of H (n x 36, row-major) - both ZERO for fixed nodes.  ngicp_pose_graph_multiply (test hook): y = (H + lambda I) x at the
 * current poses' linearisation; rows of fixed nodes are zero and their x is not read.
 * ngicp_pose_graph_corrections: for the listed nodes C_k = T_k * T_k_old^-1 in FP64 - T_old^-1 = (R^T, -(R^T t)), every sum
 * (a0 b0 + a1 b1) + a2 b2, then the product the same way - rounded to the float column-major 4x4 ngicp_keyframe_transform and
 * ngicp_voxel_rolling_transform take.  T_old: the caller's array (one per listed id), or NULL for the poses the last
 * ngicp_pose_graph_optimize started from (NGICP_ERR_ARG for a node added since, or when none has run).
 * A refused call changes nothing.  No entry here touches the source, the target, the keyframes, the voxel maps, the hooks' state or the
 * last alignment's results. */
#define NGICP_PG_TRACE_CAP 256
typedef struct ngicp_pg_options {
  int max_iterations;      /* outer iterations (64) */
  double rot_eps;          /* 2e-3 */
  double trans_eps;        /* 5e-4 */
  double cg_tol;           /* 1e-8 */
  int cg_max_iterations;   /* 1000 */
} ngicp_pg_options;        /* NULL: the defaults in brackets */
typedef struct ngicp_pg_result {
  double initial_chi2, final_chi2;
  int iterations;          /* outer iterations begun */
  int accepted;            /* accepted steps */
  long long cg_iterations; /* over all tries */
  int converged;           /* the step-size test was met */
  int n_trace;             /* rows of trace, at most NGICP_PG_TRACE_CAP (later tries are not recorded) */
  double trace[NGICP_PG_TRACE_CAP * 5]; /* per try: chi2 of the trial poses, lambda, gain ratio rho, CG iterations, accepted (1 / 0) */
} ngicp_pg_result;
int ngicp_pose_graph_clear(ngicp_t* h);
int ngicp_pose_graph_size(const ngicp_t* h, size_t* nodes_or_null, size_t* edges_or_null);
int ngicp_pose_graph_add_nodes(ngicp_t* h, const double* T_colmajor_n16, const unsigned char* fixed_or_null, size_t n, int* first_id_out_or_null);
int ngicp_pose_graph_add_edges(ngicp_t* h, const int* ij_n2, const double* Z_colmajor_n16, const double* info_n36, const unsigned char* robust_flags_or_null, size_t n,
                               int* first_edge_out_or_null);
int ngicp_pose_graph_get_edges(ngicp_t* h, int first, size_t n, int* ij_n2_or_null, double* Z_colmajor_n16_or_null, double* info_n36_or_null,
                               unsigned char* robust_flags_or_null);
int ngicp_pose_graph_set_fixed(ngicp_t* h, const int* ids, const unsigned char* flags, size_t n);
int ngicp_pose_graph_get_fixed(ngicp_t* h, int first, size_t n, unsigned char* flags_out);
int ngicp_pose_graph_set_robust(ngicp_t* h, int kind, double width);
int ngicp_pose_graph_get_poses(ngicp_t* h, int first, size_t n, double* T_colmajor_n16);
int ngicp_pose_graph_set_poses(ngicp_t* h, int first, size_t n, const double* T_colmajor_n16);
int ngicp_pose_graph_linearize(ngicp_t* h, double* chi2_out_or_null, double* edge_r_m6_or_null, double* edge_s_w_m2_or_null, double* grad_n6_or_null, double* diag_n36_or_null);
int ngicp_pose_graph_multiply(ngicp_t* h, double lambda, const double* x_n6, double* y_n6);
int ngicp_pose_graph_optimize(ngicp_t* h, const ngicp_pg_options* options_or_null, ngicp_pg_result* result);
int ngicp_pose_graph_corrections(ngicp_t* h, const int* ids, size_t n, const double* T_old_colmajor_n16_or_null, float* C_colmajor_n16);
/* device time (HIP events on the handle's stream) of the last ngicp_pose_graph_optimize, its read-backs included */
int ngicp_pose_graph_kernel_ms(const ngicp_t* h, double* ms);

/* --- rigid transform of clouds ------------------------------------ */
/* pcl::transformPointCloud(in, out, Eigen::Matrix4f) — impl/lsq_registration_impl.hpp:114, src/dlo/odom.cc:484,971-974.
 * ngicp_transform_source: the handle's current source cloud (already on the device) -> host, original point order;
 * ngicp_transform_cloud: any host cloud -> host (upload, transform, download).  Float arithmetic in PCL's order, no FMA. */
int ngicp_transform_source(ngicp_t* h, const float T_colmajor[16], float* xyz_out, size_t out_stride_bytes);
int ngicp_transform_cloud(ngicp_t* h, const float* xyz, size_t n, size_t stride_bytes, const float T_colmajor[16], float* xyz_out, size_t out_stride_bytes);

/* --- scan preprocessing ---------------------------------------------- */
/* dlo::OdomNode::preprocessPoints (src/dlo/odom.cc:443-465, configured at :122-127): pcl::removeNaNFromPointCloud, then
 * pcl::CropBox with setNegative(true) and min/max = -/+crop_half_extent (drops the points inside the cube around the
 * sensor), then pcl::VoxelGrid with a cubic leaf (one centroid of x, y, z AND intensity per occupied voxel, in ascending
 * voxel index).  Each stage is optional (remove_nan = 0, crop_half_extent <= 0, voxel_leaf <= 0).  Input: strided points,
 * xyz at byte 0 and (optionally) a float intensity at intensity_offset_bytes (16 for pcl::PointXYZI; -1: none).  Output:
 * 16 bytes per point {x, y, z, intensity}, written to out_xyzi (capacity in points; may be NULL) and kept on the device.
 * PCL's sources are not under /root/reference: the rules are restated from memory (see csrc/ngicp_filters.hip).
 * Overflow rule (restated from memory of PCL as well): when the voxel indices would not fit an int, VoxelGrid warns on stderr
 * and returns ITS input - what removeNaN / CropBox left, so with remove_nan = 0 the non-finite rows are still in it.  That is
 * the case when (1) 1 / leaf is not finite, or on an axis (max - min) / leaf is not finite or >= 2^31, or the product over the
 * axes of int64((max - min) / leaf) + 1 exceeds INT_MAX (PCL's extent test, made in float and int64 before anything is
 * converted to int); (2) floor(min / leaf) or floor(max / leaf) does not fit an int32 on an axis (a small cloud far from the
 * origin: undefined in PCL, the input is returned here); (3) the product of the lattice's extents div_b exceeds INT_MAX.
 * ngicp_set_source_preprocessed makes the filtered cloud (still on the device) the handle's source: setInputSource
 * (odom.cc:519) without the download / upload pair. */
int ngicp_preprocess_scan(ngicp_t* h, const float* pts, size_t n, size_t stride_bytes, long intensity_offset_bytes, int remove_nan, float crop_half_extent,
                          float voxel_leaf, float* out_xyzi_or_null, size_t out_capacity, size_t* n_out);
int ngicp_set_source_preprocessed(ngicp_t* h, uint64_t host_identity);

/* --- motion deskew (no counterpart in the reference) ------------------- */
/* A spinning LiDAR collects a sweep over ~100 ms while the platform moves.  Given a time per point and a pose trajectory over the
 * sweep (from an IMU or a velocity model: estimating it stays with the caller), every point is moved into the frame of ONE
 * reference pose, on the device, where the scan is unpacked.  Restated in numpy float64 by tests/_deskew_model.py.
 *   points      p_i, float32 xyz at byte 0 of a strided record.
 *   times       s_i = double(raw_i) * unit + time_offset: two roundings in that order, no FMA.  unit = 1 for NGICP_TIME_F32_S and
 *               NGICP_TIME_F64_S (seconds), 1e-9 for NGICP_TIME_U32_NS (nanoseconds).  raw_i lies inside the point record at
 *               time_offset_bytes (times == NULL), or in the strided array `times`.  It is read with one load of its own size: the
 *               offset, the stride it advances by and (inside the record) the point stride are multiples of 4 (8 for F64).
 *   trajectory  n_poses poses T_k = (R_k, t_k), double, column-major 4x4 with last row (0, 0, 0, 1), at times tau_0 < ... <
 *               tau_{M-1} in the clock of s_i; 2 <= n_poses <= NGICP_DESKEW_MAX_POSES.  T_ref: the pose whose frame the output is
 *               expressed in (NULL: identity).
 *   1. once per call  R'_k = R_ref^T R_k,  t'_k = R_ref^T (t_k - t_ref).
 *   2. per segment k < M - 1:  phi_k = so3_log(R'_k^T R'_{k+1}) (csrc/ngicp_math.h).  Consecutive poses must be less than 3 rad
 *      apart; beyond that the result is finite but unspecified.
 *   3. bracket: k_i = the largest k with tau_k <= s_i, clamped to [0, M - 2]; alpha = (s_i - tau_k) / (tau_{k+1} - tau_k), clamped to
 *      [0, 1].  No extrapolation: a time before tau_0 takes pose 0, a time at or after tau_{M-1} the last pose.
 *   4. R(s) = R'_k * so3_exp_matrix(alpha * phi_k),  t(s) = t'_k + alpha * (t'_{k+1} - t'_k).
 *   5. p'_i = R(s) p_i + t(s) in double, row by row as ((r0 * x + r1 * y) + r2 * z) + t, rounded once to float32.  Intensity is
 *      carried through unchanged.  (An identity trajectory returns the input, except that -0.0 becomes +0.0.)
 *   6. a point with a non-finite coordinate is copied unchanged; a finite point with a non-finite time gets x = y = z = NaN, so that
 *      removeNaN drops it instead of leaving it skewed unnoticed.
 * No result depends on n or on another point.
 * ngicp_deskew_cloud: host cloud -> host, like ngicp_transform_cloud (xyz only); it changes nothing a getter returns and leaves a
 * pending preprocessed cloud in place.
 * ngicp_preprocess_scan_deskewed: ngicp_preprocess_scan with the deskew in the unpack step; the filters that follow and the result
 * left on the device for ngicp_set_source_preprocessed are the same (every stage off: the deskewed scan becomes the source with no
 * download).  On an error no preprocessed cloud is pending.
 * NGICP_ERR_ARG, with ngicp_last_error naming the field: d == NULL; n_poses outside 2..256; pose_times not finite or not strictly
 * ascending; a non-finite pose entry or a last row other than (0, 0, 0, 1) (T_ref included); an unknown time_format; a time offset
 * or stride that does not fit the point stride or the format's size and alignment.  n == 0: nothing is done, 0 is returned. */
#define NGICP_TIME_F32_S 0
#define NGICP_TIME_F64_S 1
#define NGICP_TIME_U32_NS 2
#define NGICP_DESKEW_MAX_POSES 256
typedef struct ngicp_deskew {
  const void* times;            /* NULL: the time lies inside each point record at time_offset_bytes */
  size_t time_stride_bytes;     /* of `times`; ignored when times is NULL */
  long time_offset_bytes;       /* inside the point record, when times is NULL */
  int time_format;              /* NGICP_TIME_* */
  double time_offset;           /* added to every time after the unit conversion */
  size_t n_poses;
  const double* pose_times;     /* n_poses */
  const double* poses_colmajor; /* n_poses x 16 */
  const double* T_ref_colmajor; /* 16, or NULL = identity */
} ngicp_deskew_t;
int ngicp_deskew_cloud(ngicp_t* h, const float* pts, size_t n, size_t stride_bytes, const ngicp_deskew_t* d, float* xyz_out, size_t out_stride_bytes);
int ngicp_preprocess_scan_deskewed(ngicp_t* h, const float* pts, size_t n, size_t stride_bytes, long intensity_offset_bytes, const ngicp_deskew_t* d, int remove_nan,
                                   float crop_half_extent, float voxel_leaf, float* out_xyzi_or_null, size_t out_capacity, size_t* n_out);

/* --- map accumulation + voxel filter ---------------------------------- */
/* dlo::MapNode (src/dlo/map.cc:100-131): `*dlo_map += *keyframe` per keyframe (ngicp_map_add: the keyframe is appended to
 * a device-resident map), and on the publish timer `voxelgrid.filter(*dlo_map)` with a cubic leaf (ngicp_map_voxel_filter:
 * the map is replaced by its voxel centroids, same rules as above - on overflow the map, NaN rows included, stays entirely
 * unchanged; leaf <= 0 is a no-op); ngicp_map_get downloads it for publishing
 * ({x, y, z, intensity}, 16 bytes per point). */
int ngicp_map_add(ngicp_t* h, const float* pts, size_t n, size_t stride_bytes, long intensity_offset_bytes);
int ngicp_map_voxel_filter(ngicp_t* h, float leaf, size_t* n_out_or_null);
int ngicp_map_size(const ngicp_t* h, size_t* n);
int ngicp_map_get(ngicp_t* h, float* out_xyzi, size_t out_capacity);
int ngicp_map_clear(ngicp_t* h);

/* --- measurement: device stream copy -------------------------------- */
/* float4 grid-stride copy of `bytes` bytes, `reps` times on the handle's stream, HIP-event timed: (read + write) GB/s. */
int ngicp_measure_copy_bandwidth(ngicp_t* h, size_t bytes, int reps, double* gbps_out);

#ifdef __cplusplus
}
#endif
#endif /* NGICP_H */
