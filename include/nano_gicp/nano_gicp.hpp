// nano_gicp::NanoGICP<PointSource, PointTarget> — header-only drop-in for DLO's scan-matching class, running
// on an MI355X through the C ABI of include/ngicp.h (hand-written HIP kernels; no CPU fallback).
//
// It reproduces the public surface the reference exposes and DLO uses
// (/root/reference/include/nano_gicp/nano_gicp.hpp:79-125, lsq_registration.hpp:75-89 and the
// pcl::Registration entry points called at /root/reference/src/dlo/odom.cc:100-120,479-480,498-500,519-526,
// 803-837): same method names, argument meaning and failure behaviour (nothing throws on the normal path;
// failure = hasConverged() == false plus a line on stderr), including the two PUBLIC DATA MEMBERS the odometry
// node touches directly:
//     gicp.source_kdtree_ = gicp_s2s.source_kdtree_;    (odom.cc:525)  -> shares the device-resident index
//     gicp.source_covs_.clear();                        (odom.cc:526)
//     gicp.source_covs_   = gicp_s2s.source_covs_;      (odom.cc:815)  -> device-to-device, no host round trip
//
// With PCL and Eigen installed the class uses pcl::PointCloud / Eigen::Matrix4f; without them (this repo's
// build container) it uses the layout-compatible stand-ins of pcl_compat.hpp.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../ngicp.h"

#if defined(__has_include)
#if __has_include(<pcl/point_cloud.h>) && __has_include(<Eigen/Core>)
#define NGICP_HAVE_PCL 1
#endif
#endif

#ifdef NGICP_HAVE_PCL
#include <Eigen/Core>
#include <Eigen/StdVector>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <pcl/search/kdtree.h>
namespace nano_gicp {
namespace types {
template <class P> using Cloud = pcl::PointCloud<P>;
using Matrix4f = Eigen::Matrix4f;
using Matrix4d = Eigen::Matrix4d;
using Matrix6d = Eigen::Matrix<double, 6, 6>;
using CovVector = std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>>;
}  // namespace types
}  // namespace nano_gicp
#else
#include "pcl_compat.hpp"
namespace pcl {
using PointXYZI = ngicp_compat::PointXYZI;
template <class P> using PointCloud = ngicp_compat::PointCloud<P>;
template <class S, class T, class Scalar = float> using Registration = ngicp_compat::Registration<S, T, Scalar>;
namespace search {
template <class P> using KdTree = ngicp_compat::SearchKdTree<P>;
}
}  // namespace pcl
namespace Eigen {  // the two spellings DLO's members use (include/dlo/odom.h:104,133; src/dlo/odom.cc:809)
using Matrix4f = ngicp_compat::Matrix4f;
using Matrix4d = ngicp_compat::Matrix4d;
template <class T> using aligned_allocator = std::allocator<T>;
}  // namespace Eigen
namespace nano_gicp {
namespace types {
template <class P> using Cloud = ngicp_compat::PointCloud<P>;
using Matrix4f = ngicp_compat::Matrix4f;
using Matrix4d = ngicp_compat::Matrix4d;
using Matrix6d = ngicp_compat::Matrix6d;
using CovVector = std::vector<ngicp_compat::Matrix4d>;
}  // namespace types
}  // namespace nano_gicp
#endif

namespace nano_gicp {

// The low-pass state of computeSpaciousness (odom.cc:1003-1005): `static float median_prev = median_curr;
// float median_lpf = 0.95*median_prev + 0.05*median_curr; median_prev = median_lpf;` - the state is a float seeded with the first
// median, the update is evaluated in double (the literals are doubles) and narrowed to float.  Host only.  With it the call site is
//     float median_curr = this->gicp_s2s.medianRange();
//     this->metrics.spaciousness.push_back(this->spaciousness_lpf.update(median_curr));
struct SpaciousnessFilter {
  bool seeded = false;
  float median_prev = 0.f;
  float update(float median_curr) {
    if (!seeded) {
      median_prev = median_curr;
      seeded = true;
    }
    const float median_lpf = 0.95 * median_prev + 0.05 * median_curr;
    median_prev = median_lpf;
    return median_lpf;
  }
  void reset() { seeded = false; }
};

// Motion deskew (ngicp.h "motion deskew"; no counterpart in the reference, DLIO's headline addition): the pose trajectory over one
// sweep, from an IMU or a velocity model, and where each point's time is found.  A value type: it owns the poses, and only
// refers to a separate array of times.  In a DLIO-style callback:
//     nano_gicp::DeskewTrajectory traj;
//     for (auto& s : imu_states) traj.addPose(s.stamp - sweep_start, s.T_world_lidar);
//     traj.setReference(imu_states.back().T_world_lidar);                      // output in the frame at the sweep's end
//     traj.setTimesInRecord(offsetof(PointType, time), NGICP_TIME_F32_S);      // or setTimes(array.data(), n)
//     gicp_s2s.preprocessScanDeskewed(scan, traj, true, crop, leaf, /*set_as_source=*/true);
struct DeskewTrajectory {
  std::vector<double> pose_times;      // strictly ascending, in the clock of the point times (after time_offset)
  std::vector<double> poses_colmajor;  // 16 per pose
  bool has_reference = false;
  double T_ref_colmajor[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const void* times = nullptr;  // nullptr: inside each point record at time_offset_bytes
  size_t time_stride_bytes = 0;
  long time_offset_bytes = 0;
  int time_format = NGICP_TIME_F32_S;
  double time_offset = 0.0;  // added to every point time (seconds)

  void clear() { pose_times.clear(); poses_colmajor.clear(); }
  size_t size() const { return pose_times.size(); }
  void addPose(double t, const types::Matrix4d& T) {
    pose_times.push_back(t);
    poses_colmajor.insert(poses_colmajor.end(), T.data(), T.data() + 16);
  }
  void setReference(const types::Matrix4d& T) {
    has_reference = true;
    for (int e = 0; e < 16; ++e) T_ref_colmajor[e] = T.data()[e];
  }
  void setTimes(const float* t, size_t stride_bytes = sizeof(float)) { times = t; time_stride_bytes = stride_bytes; time_format = NGICP_TIME_F32_S; }
  void setTimes(const double* t, size_t stride_bytes = sizeof(double)) { times = t; time_stride_bytes = stride_bytes; time_format = NGICP_TIME_F64_S; }
  void setTimesNanoseconds(const std::uint32_t* t, size_t stride_bytes = sizeof(std::uint32_t)) { times = t; time_stride_bytes = stride_bytes; time_format = NGICP_TIME_U32_NS; }
  void setTimesInRecord(long offset_bytes, int format) { times = nullptr; time_stride_bytes = 0; time_offset_bytes = offset_bytes; time_format = format; }
  ngicp_deskew_t describe() const {
    ngicp_deskew_t d;
    d.times = times;
    d.time_stride_bytes = time_stride_bytes;
    d.time_offset_bytes = time_offset_bytes;
    d.time_format = time_format;
    d.time_offset = time_offset;
    d.n_poses = poses_colmajor.size() == pose_times.size() * 16 ? pose_times.size() : 0;
    d.pose_times = pose_times.data();
    d.poses_colmajor = poses_colmajor.data();
    d.T_ref_colmajor = has_reference ? T_ref_colmajor : nullptr;
    return d;
  }
};

enum class RegularizationMethod { NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS };  // gicp/gicp_settings.hpp:47
enum class LSQ_OPTIMIZER_TYPE { GaussNewton, LevenbergMarquardt };                         // lsq_registration.hpp:54
enum class NeighborSearchMethod { DIRECT1 = 1, DIRECT7 = 7, DIRECT27 = 27 };                // voxelized GICP (ngicp.h NGICP_VOX_*); no counterpart in the reference
enum class RobustKernel { NONE = 0, HUBER = 1, CAUCHY = 2, GEMAN_MCCLURE = 3 };                // robust kernel on every term (ngicp.h NGICP_ROBUST_*); no counterpart in the reference

template <typename PointSource, typename PointTarget>
class NanoGICP {
 public:
  using Scalar = float;
  using Matrix4 = types::Matrix4f;
  using PointCloudSource = types::Cloud<PointSource>;
  using PointCloudSourcePtr = typename PointCloudSource::Ptr;
  using PointCloudSourceConstPtr = typename PointCloudSource::ConstPtr;
  using PointCloudTarget = types::Cloud<PointTarget>;
  using PointCloudTargetPtr = typename PointCloudTarget::Ptr;
  using PointCloudTargetConstPtr = typename PointCloudTarget::ConstPtr;
  using CovVector = types::CovVector;
#ifdef NGICP_HAVE_PCL
  using KdTreeReciprocal = pcl::search::KdTree<PointSource>;  // as pcl::Registration<PointSource, PointTarget>
#else
  using KdTreeReciprocal = typename pcl::Registration<PointSource, PointTarget, Scalar>::KdTreeReciprocal;
#endif
  using KdTreeReciprocalPtr = typename KdTreeReciprocal::Ptr;

  // ---- proxies for the public data members DLO assigns to ----
  struct IndexRef {  // stands for std::shared_ptr<nanoflann::KdTreeFLANN<PointSource>> source_kdtree_ / target_kdtree_
    NanoGICP* owner = nullptr;
    bool source = true;  // which index: the source's or the target's
    IndexRef& operator=(const IndexRef& o) {
      if (owner && o.owner && owner != o.owner) owner->check(ngicp_share_source_index(owner->h_, o.owner->h_), "share_source_index");
      return *this;
    }
    // `gicp.target_kdtree_->radiusSearch(...)` as with the reference's shared_ptr
    IndexRef* operator->() { return this; }
    const IndexRef* operator->() const { return this; }
    // KdTreeFLANN::nearestKSearch / radiusSearch (include/nano_gicp/nanoflann.hpp:141-175): same signatures and return values (the
    // number found).  radius is a SQUARED distance and a hit is d2 < (float)radius, as in the reference; the hits come in ascending
    // (d2, index) order where the reference's unsorted trees give kd-tree visiting order.  The index is always the slot's current
    // cloud.  A single point is a GPU round trip (tens of microseconds): for many points use the batched forms below.
    template <class PointT>
    int nearestKSearch(const PointT& point, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) const {
      k_indices.resize(k > 0 ? k : 0);
      k_sqr_distances.resize(k_indices.size());
      if (!owner->check(ngicp_knn_search(owner->h_, source ? 0 : 1, point.data, 1, 12, k, k_indices.data(), k_sqr_distances.data()), "nearestKSearch")) {
        k_indices.clear();
        k_sqr_distances.clear();
        return 0;
      }
      return k;
    }
    template <class PointT>
    int radiusSearch(const PointT& point, double radius, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) const {
      std::vector<size_t> offsets;
      return (int)search_radius(point.data, 1, 12, radius, offsets, k_indices, k_sqr_distances);
    }
    // batched: every point of `queries`; k_indices / k_sqr_distances are row-major [queries.size()][k].  Returns queries.size() * k.
    template <class P>
    size_t nearestKSearch(const types::Cloud<P>& queries, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) const {
      const size_t nq = queries.size(), m = k > 0 ? nq * (size_t)k : 0;
      k_indices.resize(m);
      k_sqr_distances.resize(m);
      if (nq && !owner->check(ngicp_knn_search(owner->h_, source ? 0 : 1, queries.points[0].data, nq, sizeof(P), k, k_indices.data(), k_sqr_distances.data()),
                              "nearestKSearch")) {
        k_indices.clear();
        k_sqr_distances.clear();
        return 0;
      }
      return m;
    }
    // batched: query i's hits are [offsets[i], offsets[i + 1]) of the flat vectors (offsets has queries.size() + 1 entries).  Returns
    // the total number of hits.
    template <class P>
    size_t radiusSearch(const types::Cloud<P>& queries, double radius, std::vector<size_t>& offsets, std::vector<int>& k_indices,
                        std::vector<float>& k_sqr_distances) const {
      return search_radius(queries.size() ? queries.points[0].data : nullptr, queries.size(), sizeof(P), radius, offsets, k_indices, k_sqr_distances);
    }

   private:
    size_t search_radius(const float* xyz, size_t nq, size_t stride, double radius, std::vector<size_t>& offsets, std::vector<int>& idx,
                         std::vector<float>& d2) const {
      offsets.assign(nq + 1, 0);
      size_t total = 0;
      bool ok = owner->check(ngicp_radius_search(owner->h_, source ? 0 : 1, xyz, nq, stride, radius, offsets.data(), &total), "radiusSearch");
      idx.resize(ok ? total : 0);
      d2.resize(idx.size());
      if (ok && total && !owner->check(ngicp_radius_fetch(owner->h_, idx.data(), d2.data(), total), "radiusSearch")) ok = false;
      if (!ok) {
        offsets.assign(nq + 1, 0);
        idx.clear();
        d2.clear();
        return 0;
      }
      return total;
    }
  };
  struct CovRef {  // stands for std::vector<Eigen::Matrix4d> source_covs_ / target_covs_
    NanoGICP* owner = nullptr;
    bool source = true;
    void clear() { owner->check(source ? ngicp_clear_source_covs(owner->h_) : ngicp_clear_target_covs(owner->h_), "clear_covs"); }
    size_t size() const {
      size_t n = 0;
      if (source) ngicp_source_covs_size(owner->h_, &n); else ngicp_target_covs_size(owner->h_, &n);
      return n;
    }
    CovRef& operator=(const CovRef& o) {
      if (this == &o) return *this;
      if (source && o.source) {
        owner->check(ngicp_copy_source_covs(owner->h_, o.owner->h_), "copy_source_covs");  // stays on the device
      } else {
        CovVector tmp = o.owner->fetch(o.source);
        *this = tmp;
      }
      return *this;
    }
    CovRef& operator=(const CovVector& v) {
      owner->check(source ? ngicp_set_source_covs(owner->h_, reinterpret_cast<const double*>(v.data()), v.size())
                          : ngicp_set_target_covs(owner->h_, reinterpret_cast<const double*>(v.data()), v.size()), "set_covs");
      return *this;
    }
    operator CovVector() const { return owner->fetch(source); }
  };

  explicit NanoGICP(int device = 0) {
    int rc = ngicp_create(device, &h_);
    if (rc != NGICP_OK) {
      std::fprintf(stderr, "[NanoGICP] cannot create the GPU engine: %s\n", ngicp_last_error(nullptr));
      h_ = nullptr;
    }
    source_kdtree_.owner = target_kdtree_.owner = this;
    source_kdtree_.source = true;
    target_kdtree_.source = false;
    source_covs_.owner = target_covs_.owner = this;
    source_covs_.source = true;
    target_covs_.source = false;
    set_identity(final_transformation_);
    final_hessian_ = types::Matrix6d::Identity();
  }
  virtual ~NanoGICP() { ngicp_destroy(h_); }
  NanoGICP(const NanoGICP&) = delete;
  NanoGICP& operator=(const NanoGICP&) = delete;

  bool valid() const { return h_ != nullptr; }

  // ---- NanoGICP / LsqRegistration setters (impl/nano_gicp_impl.hpp:70-88, impl/lsq_registration_impl.hpp:69-81) ----
  void setNumThreads(int n) { num_threads_ = n; push(); }
  void setCorrespondenceRandomness(int k) { k_correspondences_ = k; push(); }
  void setRegularizationMethod(RegularizationMethod m) { regularization_method_ = m; push(); }
  void setRotationEpsilon(double e) { rotation_epsilon_ = e; push(); }
  void setInitialLambdaFactor(double f) { lm_init_lambda_factor_ = f; push(); }
  void setDebugPrint(bool on) { lm_debug_print_ = on; }
  // ---- pcl::Registration setters DLO calls (odom.cc:101-120) ----
  void setMaxCorrespondenceDistance(double d) { corr_dist_threshold_ = d; push(); }
  void setMaximumIterations(int n) { max_iterations_ = n; push(); }
  void setTransformationEpsilon(double e) { transformation_epsilon_ = e; push(); }
  void setEuclideanFitnessEpsilon(double) {}               // accepted, never read by nano_gicp
  void setRANSACIterations(int) {}                         // "
  void setRANSACOutlierRejectionThreshold(double) {}       // "
  // PCL's own FLANN trees are never used by nano_gicp (DLO hands over null pointers with force_no_recompute = true so that
  // initCompute() does not build them, odom.cc:116-120): any pointer type is accepted - pcl::search::KdTree<P>::Ptr with
  // real PCL, the stand-in of pcl_compat.hpp without - and dropped.
  template <class TreePtr> void setSearchMethodSource(const TreePtr&, bool /*force_no_recompute*/ = false) {}
  template <class TreePtr> void setSearchMethodTarget(const TreePtr&, bool /*force_no_recompute*/ = false) {}
  void setLSQType(LSQ_OPTIMIZER_TYPE t) { lsq_optimizer_type_ = t; push(); }

  // ---- clouds (impl/nano_gicp_impl.hpp:101-139) ----
  virtual void setInputSource(const PointCloudSourceConstPtr& cloud) {
    if (input_ == cloud) return;
    input_ = cloud;
    check(ngicp_set_source(h_, xyz(cloud), cloud->size(), sizeof(PointSource), id(cloud)), "setInputSource");
  }
  virtual void registerInputSource(const PointCloudSourceConstPtr& cloud) {
    if (input_ == cloud) return;
    input_ = cloud;
    check(ngicp_register_source(h_, xyz(cloud), cloud->size(), sizeof(PointSource), id(cloud)), "registerInputSource");
  }
  virtual void setInputTarget(const PointCloudTargetConstPtr& cloud) {
    if (target_ == cloud && !device_target_) return;
    target_ = cloud;
    device_target_ = false;
    check(ngicp_set_target(h_, xyz(cloud), cloud->size(), sizeof(PointTarget), id(cloud)), "setInputTarget");
  }
  virtual void clearSource() { input_.reset(); check(ngicp_clear_source(h_), "clearSource"); }
  virtual void clearTarget() { target_.reset(); device_target_ = false; check(ngicp_clear_target(h_), "clearTarget"); }
  virtual void swapSourceAndTarget() {  // :91-98
    if (device_target_) {  // a device-assembled submap has no host cloud to become the input: materialise it first
      std::fprintf(stderr, "[NanoGICP] swapSourceAndTarget(): the target is a device-resident submap; not swapped\n");
      return;
    }
    input_.swap(target_);
    check(ngicp_swap_source_target(h_), "swapSourceAndTarget");
  }
  PointCloudSourceConstPtr getInputSource() const { return input_; }
  PointCloudTargetConstPtr getInputTarget() const { return target_; }

  // ---- covariances (:142-159, nano_gicp.hpp:100-106) ----
  virtual void setSourceCovariances(const CovVector& c) { source_covs_ = c; }
  virtual void setTargetCovariances(const CovVector& c) { target_covs_ = c; }
  virtual bool calculateSourceCovariances() { return check(ngicp_compute_source_covs(h_), "calculateSourceCovariances"); }
  virtual bool calculateTargetCovariances() { return check(ngicp_compute_target_covs(h_), "calculateTargetCovariances"); }
  const CovVector& getSourceCovariances() const { cache_src_ = fetch(true); return cache_src_; }
  const CovVector& getTargetCovariances() const { cache_tgt_ = fetch(false); return cache_tgt_; }

  // ---- pcl::Registration::align: copies input into output, identity final transform, then
  //      computeTransformation; output[i].data[3] = 1 ----
  void align(PointCloudSource& output) { Matrix4 I; set_identity(I); align(output, I); }
  void align(PointCloudSource& output, const Matrix4& guess) {
    converged_ = false;
    set_identity(final_transformation_);
    if (!h_ || !input_ || !haveTarget()) {  // PCL's initCompute() fails silently
      std::fprintf(stderr, "[NanoGICP] align(): no input source/target\n");
      return;
    }
    output = *input_;
    int conv = 0, nit = 0;
    std::vector<float> xyz_out(input_->size() * 3);
    int rc = ngicp_align(h_, guess.data(), final_transformation_.data(), &conv, &nit, final_hessian_.data(), xyz_out.data(), 12);
    converged_ = conv != 0;
    nr_iterations_ = nit;
    if (rc != NGICP_OK) {
      std::fprintf(stderr, "[NanoGICP] align(): %s\n", ngicp_last_error(h_));
      return;
    }
    if (lm_debug_print_) print_lm_table();
    for (size_t i = 0; i < output.size(); ++i) {  // transformed xyz; the other fields stay as in the input
      output.points[i].data[0] = xyz_out[i * 3 + 0];
      output.points[i].data[1] = xyz_out[i * 3 + 1];
      output.points[i].data[2] = xyz_out[i * 3 + 2];
      output.points[i].data[3] = 1.0f;
    }
  }
  // same, without materialising the aligned cloud (DLO never reads it: odom.cc:799-837)
  void alignPoseOnly(const Matrix4& guess) {
    converged_ = false;
    set_identity(final_transformation_);
    if (!h_ || !input_ || !haveTarget()) return;
    int conv = 0, nit = 0;
    int rc = ngicp_align(h_, guess.data(), final_transformation_.data(), &conv, &nit, final_hessian_.data(), nullptr, 0);
    converged_ = conv != 0;
    nr_iterations_ = nit;
    if (rc != NGICP_OK) std::fprintf(stderr, "[NanoGICP] align(): %s\n", ngicp_last_error(h_));
    else if (lm_debug_print_) print_lm_table();
  }
  // setDebugPrint(true): the reference prints a banner per align() and one row per LM trial while it optimises
  // (impl/lsq_registration_impl.hpp:95-99,183-189: boost::format "%5d %15g %15g %15g %15g %15g %5c" of i, y0, yi, rho, lambda,
  // |delta|, 'x' when rho > 0, a header in front of trial 0).  The loop runs on the device here, so the same table is printed
  // from the engine's trace once align() has returned.
  void print_lm_table() const {
    size_t n = 0;
    if (ngicp_get_lm_trace(h_, nullptr, 0, &n) != NGICP_OK) return;
    std::vector<double> rows(n * 8);
    if (n && ngicp_get_lm_trace(h_, rows.data(), n, &n) != NGICP_OK) return;
    std::printf("********************************************\n***************** optimize *****************\n********************************************\n");
    for (size_t r = 0; r < n; ++r) {
      const double* q = &rows[r * 8];  // {outer iteration, trial, y0, yi, rho, lambda, |delta|, accepted}
      if ((int)q[1] == 0) std::printf("--- LM optimization ---\n%5s %15s %15s %15s %15s %15s %5s\n", "i", "y0", "yi", "rho", "lambda", "|delta|", "dec");
      std::printf("%5d %15g %15g %15g %15g %15g %5c\n", (int)q[1], q[2], q[3], q[4], q[5], q[6], q[4] > 0.0 ? 'x' : ' ');
    }
    std::fflush(stdout);
  }
  Matrix4 getFinalTransformation() const { return final_transformation_; }
  bool hasConverged() const { return converged_; }
  const types::Matrix6d& getFinalHessian() const { return final_hessian_; }
  int getNrIterations() const { return nr_iterations_; }
  // pcl::Registration::getFitnessScore(max_range): the mean squared 1-NN distance of the source transformed by
  // final_transformation_ over the points with a squared distance <= max_range (a SQUARED distance); DBL_MAX when none counts.
  // Computed on the GPU from the device-resident clouds (csrc/ngicp_query.h).  The reference would dereference the null search tree
  // DLO hands PCL (odom.cc:116-120); this returns what PCL computes with a built tree.
  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) {
    double score = std::numeric_limits<double>::max();
    if (h_) check(ngicp_fitness_score(h_, final_transformation_.data(), max_range, &score, nullptr), "getFitnessScore");
    return score;
  }
  ngicp_t* handle() { return h_; }

  // ---- voxelized GICP (no counterpart in the reference; include/ngicp.h "voxelized GICP") ----
  // setVoxelResolution(res > 0): align() matches every source point against the Gaussian of the target voxel (edge `res`) it falls into -
  // one table lookup instead of an exact nearest-neighbour search; the voxel map is built on the device at the first align() after the
  // target, its covariances or the resolution changed.  0 (the default) is exact GICP.  A different algorithm with different results:
  // setMaxCorrespondenceDistance is not consulted, and alignBatch is not available while it is on (alignBatchVoxel is).  getVoxelMapSize:
  // occupied voxels.
  void setVoxelResolution(double res) {
    if (h_ && check(ngicp_set_voxel_resolution(h_, res), "setVoxelResolution")) voxel_resolution_ = res;
  }
  double getVoxelResolution() const { return voxel_resolution_; }
  size_t getVoxelMapSize() {
    size_t n = 0;
    if (h_) check(ngicp_voxelmap_size(h_, &n), "getVoxelMapSize");
    return n;
  }
  // The voxels a source point is matched against: its own (DIRECT1, the default), its own and the 6 face neighbours (DIRECT7), or all 27
  // (DIRECT27); the terms of the occupied ones are summed.  Remembered while the voxel mode is off.  A change keeps the voxel map.
  void setNeighborSearchMethod(NeighborSearchMethod m) {
    if (h_) check(ngicp_set_voxel_neighbors(h_, static_cast<int>(m)), "setNeighborSearchMethod");
  }
  NeighborSearchMethod getNeighborSearchMethod() const {
    int m = NGICP_VOX_DIRECT1;
    if (h_) check(ngicp_get_voxel_neighbors(h_, &m), "getNeighborSearchMethod");
    return static_cast<NeighborSearchMethod>(m);
  }
  // the voxel numbers of every slot of the last linearisation, row-major n x K in the source's order, -1 where a slot is empty; K is
  // getNeighborSearchMethod()'s value.  Empty on error (and while the voxel mode is off).
  std::vector<int> voxelCorrespondences() {
    std::vector<int> out;
    if (!h_ || !input_) return out;
    out.resize(input_->size() * static_cast<size_t>(getNeighborSearchMethod()));
    int K = 0;
    if (!check(ngicp_voxel_correspondences(h_, out.data(), out.size(), &K), "voxelCorrespondences")) out.clear();
    return out;
  }
  // A robust kernel on every term of the cost (include/ngicp.h "robust kernel"): Huber, Cauchy or Geman-McClure of the given width on
  // s = e^T M e; NONE (the default) is the plain cost.  It holds for align() on every route - exact, voxelized with any neighbourhood,
  // rolling map - and is remembered across mode switches; alignBatch / alignBatchVoxel are not available while it is set.  A bad kind
  // or width is reported and changes nothing.
  void setRobustKernel(RobustKernel kind, double width = 1.0) {
    if (h_) check(ngicp_set_robust_kernel(h_, static_cast<int>(kind), width), "setRobustKernel");
  }
  RobustKernel getRobustKernel(double* width = nullptr) const {
    int k = NGICP_ROBUST_NONE;
    double w = 1.0;
    if (h_) check(ngicp_get_robust_kernel(h_, &k, &w), "getRobustKernel");
    if (width) *width = w;
    return static_cast<RobustKernel>(k);
  }
  // Per term, at the pose T under the correspondences and matrices of the last linearisation: s = e^T M e and the weight the kernel
  // gives it, row-major n x K in the source's order (K = 1 for exact GICP, else getNeighborSearchMethod()'s value); s = -1, w = 0 where
  // a slot has no correspondence.  What the kernel down-weighted - e.g. to keep a moving object out of insertIntoVoxelMap.  False (and
  // both empty) on error.
  bool robustTerms(const types::Matrix4d& T, std::vector<double>& s, std::vector<double>& w) {
    s.clear();
    w.clear();
    if (!h_ || !input_) return false;
    const size_t K = voxel_resolution_ > 0.0 ? static_cast<size_t>(getNeighborSearchMethod()) : 1;
    s.resize(input_->size() * K);
    w.resize(s.size());
    int k_out = 0;
    if (!check(ngicp_robust_terms(h_, T.data(), s.data(), w.data(), s.size(), &k_out), "robustTerms")) {
      s.clear();
      w.clear();
      return false;
    }
    return true;
  }
  // A Gaussian prior on the pose (include/ngicp.h "pose prior"): the cost of every align() - exact, voxelized with any neighbourhood,
  // rolling map, alignBatch / alignBatchVoxel - gains r^T info r, r = (log_SO3(R R_p^T), t - t_p), with T_prior = (R_p, t_p) and info a
  // symmetric 6x6 information matrix, rotation first (rad^-2, m^-2).  E.g. an IMU or wheel-odometry prediction with its inverse
  // covariance; info = diag(w, w, 0, 0, 0, w) at T_prior = guess holds roll, pitch and height (planar motion).  Remembered across mode
  // switches.  A bad argument is reported and changes nothing (false).  (With Eigen: Matrix4d, Matrix<double, 6, 6>.)
  bool setPosePrior(const types::Matrix4d& T_prior, const types::Matrix6d& info) {
    return h_ && check(ngicp_set_pose_prior(h_, T_prior.data(), info.data()), "setPosePrior");
  }
  void clearPosePrior() {
    if (h_) check(ngicp_set_pose_prior(h_, nullptr, nullptr), "clearPosePrior");
  }
  // true when a prior is set (then T_prior and info, where not null, receive it)
  bool getPosePrior(types::Matrix4d* T_prior = nullptr, types::Matrix6d* info = nullptr) const {
    int set = 0;
    if (h_) check(ngicp_get_pose_prior(h_, &set, T_prior ? T_prior->data() : nullptr, info ? info->data() : nullptr), "getPosePrior");
    return set != 0;
  }
  // The prior's share alone at the pose T: the residual r (6), the cost r^T info r, H_p = J_p^T info J_p and b_p = J_p^T info r (6),
  // evaluated on the device by the solver's own functions.  Any output may be null.  False on error (no prior set).
  bool posePriorTerms(const types::Matrix4d& T, double* r6, double* cost, types::Matrix6d* H, double* b6) {
    return h_ && check(ngicp_pose_prior_terms(h_, T.data(), r6, cost, H ? H->data() : nullptr, b6), "posePriorTerms");
  }
  // setVoxelSubmapMerge(true): the voxel map of a submap assembled by setSubmapKeyframes is merged from per-keyframe voxel sums, which
  // every keyframe carries and which are built once per keyframe and resolution, instead of being summed over all points of the submap
  // at every change (include/ngicp.h "merged voxel map").  The voxels, their numbers and their counts are the same; means and covariances
  // differ in rounding only (the sums are grouped by keyframe).  OFF by default; with it off nothing changes.  Every other target, and a
  // submap whose covariances were replaced, is summed over its points as before.  Remembered while the voxel mode is off; a change
  // drops the voxel map.
  void setVoxelSubmapMerge(bool on) {
    if (h_) check(ngicp_set_voxel_submap_merge(h_, on ? 1 : 0), "setVoxelSubmapMerge");
  }
  bool getVoxelSubmapMerge() const {
    int on = 0;
    if (h_) check(ngicp_get_voxel_submap_merge(h_, &on), "getVoxelSubmapMerge");
    return on != 0;
  }
  // maps built by the merged route and keyframe parts built since this object was created; device time of the last merged build
  struct VoxelMapMergeStats {
    long long merged_builds = 0, parts_built = 0;
    double last_parts_ms = 0.0, last_merge_ms = 0.0;
  };
  VoxelMapMergeStats voxelMapMergeStats() const {
    VoxelMapMergeStats s;
    if (h_) check(ngicp_voxelmap_merge_stats(h_, &s.merged_builds, &s.parts_built, &s.last_parts_ms, &s.last_merge_ms), "voxelMapMergeStats");
    return s;
  }
  // the voxel part of keyframe `id` at the current resolution (built if absent): per voxel in ascending (iz, iy, ix) the index, the sum
  // of the points, the sum of the covariances {xx, xy, xz, yy, yz, zz} and the count.  Empty on error (and while the voxel mode is off).
  struct KeyframeVoxelMap {
    std::vector<int> ijk;         // n x 3
    std::vector<double> sum;      // n x 3
    std::vector<double> covsum;   // n x 6
    std::vector<int> count;       // n
    size_t size() const { return count.size(); }
  };
  KeyframeVoxelMap keyframeVoxelMap(int id) {
    KeyframeVoxelMap m;
    size_t n = 0;
    if (!h_ || !check(ngicp_keyframe_voxelmap_get(h_, id, &n, nullptr, nullptr, nullptr, nullptr), "keyframeVoxelMap")) return m;
    m.ijk.resize(3 * n); m.sum.resize(3 * n); m.covsum.resize(6 * n); m.count.resize(n);
    if (!check(ngicp_keyframe_voxelmap_get(h_, id, &n, m.ijk.data(), m.sum.data(), m.covsum.data(), m.count.data()), "keyframeVoxelMap")) m = KeyframeVoxelMap();
    return m;
  }

  // ---- the rolling voxel map (no counterpart in the reference; include/ngicp.h "rolling voxel map") ----
  // setVoxelRolling(true) with setVoxelResolution(res > 0): align() and alignBatchVoxel() use a voxel map that lives on the device across
  // frames - insertIntoVoxelMap adds a scan at a pose, evictVoxelMap drops voxels by distance or age - instead of a map built from the
  // target, which is then not read at all (it need not be set).  Remembered while the voxel mode is off; switching off keeps the map.
  void setVoxelRolling(bool on) {
    if (h_ && check(ngicp_set_voxel_rolling(h_, on ? 1 : 0), "setVoxelRolling")) voxel_rolling_ = on;
  }
  bool getVoxelRolling() const { return voxel_rolling_; }
  // what an insert did: voxels it created, voxels of the scan (created or added to); ok false when it was refused (nothing changed)
  struct VoxelMapInsert {
    bool ok = false;
    size_t n_new = 0, n_touched = 0;
  };
  // add `producer`'s current source cloud (the producer may be *this: align, then insert at the result), transformed by T on the device,
  // with its source covariances (computed if missing, as addKeyframe does)
  VoxelMapInsert insertIntoVoxelMap(NanoGICP& producer, const Matrix4& T) {
    VoxelMapInsert r;
    r.ok = h_ && check(ngicp_voxel_rolling_insert(h_, producer.h_, T.data(), &r.n_new, &r.n_touched), "insertIntoVoxelMap");
    return r;
  }
  // remove the voxels whose centre is farther than max_dist from `centre` (max_dist > 0) or whose last insert is older than min_stamp
  // (min_stamp > 0; inserts count from 1); returns how many went
  size_t evictVoxelMap(const float centre[3], double max_dist, long long min_stamp = 0) {
    size_t n = 0;
    if (h_) check(ngicp_voxel_rolling_evict(h_, centre, max_dist, min_stamp, &n), "evictVoxelMap");
    return n;
  }
  void clearVoxelMap() {
    if (h_) check(ngicp_voxel_rolling_clear(h_), "clearVoxelMap");
  }
  // the map's state, voxels in order of first insertion: the index, the sums of the points and of the (rotated) covariances
  // {xx, xy, xz, yy, yz, zz}, the count and the number of the last insert that added a point.  Empty on error.
  struct RollingVoxelMap {
    std::vector<int> ijk;          // n x 3
    std::vector<double> sum;       // n x 3
    std::vector<double> covsum;    // n x 6
    std::vector<int> count;        // n
    std::vector<long long> stamp;  // n
    size_t size() const { return count.size(); }
  };
  RollingVoxelMap rollingVoxelMap() {
    RollingVoxelMap m;
    size_t n = 0;
    if (!h_ || !check(ngicp_voxel_rolling_get(h_, &n, nullptr, nullptr, nullptr, nullptr, nullptr), "rollingVoxelMap")) return m;
    m.ijk.resize(3 * n); m.sum.resize(3 * n); m.covsum.resize(6 * n); m.count.resize(n); m.stamp.resize(n);
    if (!check(ngicp_voxel_rolling_get(h_, &n, m.ijk.data(), m.sum.data(), m.covsum.data(), m.count.data(), m.stamp.data()), "rollingVoxelMap")) m = RollingVoxelMap();
    return m;
  }
  // accepted inserts since the last clear, voxels, capacity of the per-voxel arrays, table slots; device time of the last insert / eviction
  struct VoxelRollingStats {
    long long inserts = 0;
    size_t n_vox = 0, capacity_vox = 0, table_slots = 0;
    double last_insert_ms = 0.0, last_evict_ms = 0.0;
  };
  VoxelRollingStats voxelRollingStats() const {
    VoxelRollingStats s;
    if (h_) check(ngicp_voxel_rolling_stats(h_, &s.inserts, &s.n_vox, &s.capacity_vox, &s.table_slots, &s.last_insert_ms, &s.last_evict_ms), "voxelRollingStats");
    return s;
  }
  // ---- the rolling map from voxel records (include/ngicp.h "rolling voxel map: records"): restore, merge, move ----
  // The map becomes exactly `m` (what rollingVoxelMap() returned, here or in another session, on a handle of the same resolution) and
  // the insert counter `inserts` (voxelRollingStats().inserts).  false: refused, nothing changed.
  bool setRollingVoxelMap(const RollingVoxelMap& m, long long inserts) {
    const size_t n = m.size();
    if (m.ijk.size() != 3 * n || m.sum.size() != 3 * n || m.covsum.size() != 6 * n || m.stamp.size() != n) {
      std::fprintf(stderr, "[NanoGICP] setRollingVoxelMap: arrays of different lengths\n");
      return false;
    }
    return h_ && check(ngicp_voxel_rolling_set(h_, n, m.ijk.data(), m.sum.data(), m.covsum.data(), m.count.data(), m.stamp.data(), inserts), "setRollingVoxelMap");
  }
  // Add the records of `m` (its ijk and stamps are not read) at the float pose T: every record lands, whole, in the voxel of its moved
  // mean.  Taking a map to another resolution is this at identity after setVoxelResolution - not the map the points would have built.
  VoxelMapInsert insertVoxelsIntoVoxelMap(const RollingVoxelMap& m, const Matrix4& T) {
    VoxelMapInsert r;
    const size_t n = m.size();
    if (m.sum.size() != 3 * n || m.covsum.size() != 6 * n) {
      std::fprintf(stderr, "[NanoGICP] insertVoxelsIntoVoxelMap: arrays of different lengths\n");
      return r;
    }
    r.ok = h_ && check(ngicp_voxel_rolling_insert_voxels(h_, n, m.sum.data(), m.covsum.data(), m.count.data(), T.data(), &r.n_new, &r.n_touched), "insertVoxelsIntoVoxelMap");
    return r;
  }
  // The same with the records of `other`'s rolling map, read on the device; `other` (not *this) is left unchanged.
  VoxelMapInsert insertVoxelMapFrom(NanoGICP& other, const Matrix4& T) {
    VoxelMapInsert r;
    r.ok = h_ && check(ngicp_voxel_rolling_insert_map(h_, other.h_, T.data(), &r.n_new, &r.n_touched), "insertVoxelMapFrom");
    return r;
  }
  // Move the map by T in place (after a loop closure, say): the insert counter stays, a voxel keeps the largest stamp of the records
  // that landed in it.  Returns the voxels after the move; `ok` false when it was refused (the map is as it was).
  size_t transformVoxelMap(const Matrix4& T, bool* ok = nullptr) {
    size_t n = 0;
    const bool good = h_ && check(ngicp_voxel_rolling_transform(h_, T.data(), &n), "transformVoxelMap");
    if (ok) *ok = good;
    return n;
  }
  // ---- clearing the rolling map along a scan's rays (include/ngicp.h "rolling voxel map: clearing along rays") ----
  // Per voxel of the map: the rays of `producer`'s current source cloud at the float pose T that pass through it (miss) and that end in
  // it (hit), from `origin` (three floats in the map frame; nullptr: T's translation).  The voxels with at least min_miss misses, no hit
  // and (keep_stamp > 0) a stamp below keep_stamp are removed.  In a frame loop: align, clear with the aligned scan, then insert it.
  struct RayClearOptions {
    int near_cells = 1;         // the first counted step of a ray
    int back_cells = 2;         // steps before the end cell that are not counted
    int max_steps = 4096;       // the last step a ray may count (1 .. 65536): what bounds a ray's cost
    int min_miss = 2;
    double radius_cells = 0.25; // a miss needs the voxel's mean within radius_cells * res of the ray's line; 0: every occupied cell
    long long keep_stamp = 0;
    bool dry_run = false;       // count only: the map, the correspondences and the hooks' state stay
  };
  struct RayClearResult {
    bool ok = false;            // false: refused, nothing changed
    size_t n_removed = 0;
    long long steps = 0, occupied = 0, misses = 0;  // counted steps; of them in occupied cells; of those, misses
    double kernel_ms = 0.0;
  };
  RayClearResult clearVoxelMapAlongRays(NanoGICP& producer, const Matrix4& T, const float* origin = nullptr, const RayClearOptions& options = RayClearOptions()) {
    RayClearResult r;
    ngicp_ray_clear_options o;
    o.near_cells = options.near_cells;
    o.back_cells = options.back_cells;
    o.max_steps = options.max_steps;
    o.min_miss = options.min_miss;
    o.radius_cells = options.radius_cells;
    o.keep_stamp = options.keep_stamp;
    o.dry_run = options.dry_run ? 1 : 0;
    ngicp_ray_clear_result res;
    r.ok = h_ && check(ngicp_voxel_rolling_ray_clear(h_, producer.h_, T.data(), origin, &o, &res), "clearVoxelMapAlongRays");
    if (r.ok) {
      r.n_removed = res.n_removed;
      r.steps = res.steps;
      r.occupied = res.occupied;
      r.misses = res.misses;
      r.kernel_ms = res.kernel_ms;
    }
    return r;
  }
  // miss and hit of the last clearVoxelMapAlongRays, per voxel in the numbering from before its removal; false (and both empty) when
  // no call has been accepted or anything else has changed the map since
  bool voxelMapRayCounts(std::vector<uint32_t>& miss, std::vector<uint32_t>& hit) {
    miss.clear(); hit.clear();
    size_t n = 0;
    if (!h_ || !check(ngicp_voxel_rolling_ray_counts(h_, nullptr, nullptr, 0, &n), "voxelMapRayCounts")) return false;
    miss.resize(n); hit.resize(n);
    if (!check(ngicp_voxel_rolling_ray_counts(h_, miss.data(), hit.data(), n, &n), "voxelMapRayCounts")) {
      miss.clear(); hit.clear();
      return false;
    }
    return true;
  }
  // ---- the gated insert into the rolling map (include/ngicp.h "rolling voxel map: gated insert") ----
  // insertIntoVoxelMap of the points the map does not contradict: every point of `producer`'s current source cloud is classified against
  // the rolling map at the float pose T, and the EXPLAINED points, the NEW ones (insert_new) and the UNJUDGED ones (insert_unjudged) are
  // inserted exactly as insertIntoVoxelMap would insert them alone.  In a frame loop: align, clearVoxelMapAlongRays, insertIntoVoxelMapGated.
  enum InsertClass : uint8_t {
    INSERT_NEW = NGICP_GATE_NEW,              // no occupied slot around the point
    INSERT_EXPLAINED = NGICP_GATE_EXPLAINED,  // the best Mahalanobis term against the map is within the gate
    INSERT_CONFLICT = NGICP_GATE_CONFLICT,    // it is above the gate: never inserted
    INSERT_UNJUDGED = NGICP_GATE_UNJUDGED     // occupied slots, but no voxel of min_voxel_count points gave a finite term
  };
  struct GatedInsertOptions {
    double max_mahalanobis = std::numeric_limits<double>::max();  // the gate on voxelFitness' m (chi-square-like, 3 degrees of freedom); the largest double: no gate
    int min_voxel_count = 1;      // a voxel judges only with at least this many points
    bool insert_new = true;
    bool insert_unjudged = true;
    bool dry_run = false;         // classify only: the map, the counter, the correspondences and the hooks' state stay
  };
  struct GatedInsert {
    bool ok = false;              // false: refused, nothing changed
    size_t n_points = 0;
    size_t n_class[4] = {0, 0, 0, 0};  // by InsertClass
    size_t n_kept = 0, n_new = 0, n_touched = 0;
    double kernel_ms = 0.0;
  };
  GatedInsert insertIntoVoxelMapGated(NanoGICP& producer, const Matrix4& T, const GatedInsertOptions& options) {
    GatedInsert r;
    ngicp_gate_options o;
    o.max_mahalanobis = options.max_mahalanobis;
    o.min_voxel_count = options.min_voxel_count;
    o.insert_new = options.insert_new ? 1 : 0;
    o.insert_unjudged = options.insert_unjudged ? 1 : 0;
    o.dry_run = options.dry_run ? 1 : 0;
    ngicp_gate_result res;
    r.ok = h_ && check(ngicp_voxel_rolling_insert_gated(h_, producer.h_, T.data(), &o, &res), "insertIntoVoxelMapGated");
    if (r.ok) {
      r.n_points = res.n_points;
      for (int k = 0; k < 4; ++k) r.n_class[k] = res.n_class[k];
      r.n_kept = res.n_kept;
      r.n_new = res.n_new;
      r.n_touched = res.n_touched;
      r.kernel_ms = res.kernel_ms;
    }
    return r;
  }
  // the classes (InsertClass values) of the last insertIntoVoxelMapGated, dry or not, in the scan's original order; false (and empty)
  // before the first such call and after clearVoxelMap
  bool voxelMapInsertClasses(std::vector<uint8_t>& classes) {
    classes.clear();
    size_t n = 0;
    if (!h_ || !check(ngicp_voxel_rolling_insert_classes(h_, nullptr, 0, &n), "voxelMapInsertClasses")) return false;
    classes.resize(n);
    if (!check(ngicp_voxel_rolling_insert_classes(h_, classes.data(), n, &n), "voxelMapInsertClasses")) {
      classes.clear();
      return false;
    }
    return true;
  }

  // ---- the spaciousness metric (dlo::OdomNode::computeSpaciousness, odom.cc:990-1010) without downloading the scan ----
  // rangeSelect: the range (float)sqrt((double)x*x + y*y + z*z) of 0-based rank `rank` among the cloud's ranges in ascending order (NaN
  // after +inf); medianRange: rank n / 2, the reference's median_curr.  which: 0 = the input source, 1 = the target, 2 = the scan
  // preprocessPoints left on the device.  NaN (and a line on stderr) on failure.  Computed on the GPU (csrc/ngicp_range.h).
  float rangeSelect(size_t rank, int which = 0) {
    float v = std::numeric_limits<float>::quiet_NaN();
    if (h_) check(ngicp_range_select(h_, which, rank, &v, nullptr), "rangeSelect");
    return v;
  }
  float medianRange(int which = 0) {
    float v = std::numeric_limits<float>::quiet_NaN();
    if (h_) check(ngicp_range_median(h_, which, &v, nullptr), "medianRange");
    return v;
  }

  // ---- more than one candidate pose (no counterpart in the reference; include/ngicp.h "more than one initial guess") ----
  // alignBatch: every guess aligned on the current source / target pair in the same kernel launches; result g is bit for bit what
  // alignPoseOnly(guesses[g]) leaves in the getters.  The getters themselves (getFinalTransformation, hasConverged, ...) keep the
  // results of the last align().  getFitnessScores: getFitnessScore for each transform, one launch.  Recipe: INTEGRATION.md.
  struct BatchResult {
    Matrix4 transformation;
    bool converged = false;
    int nr_iterations = 0;
    types::Matrix6d hessian;
  };
  std::vector<BatchResult> alignBatch(const std::vector<Matrix4>& guesses) { return alignBatchThrough(ngicp_align_batch, "alignBatch", guesses); }
  // alignBatch against the voxelized target (setVoxelResolution > 0, any setNeighborSearchMethod): result g is bit for bit what
  // alignPoseOnly(guesses[g]) leaves in the getters in that mode.  Empty (and a line on stderr) while the voxel mode is off.
  std::vector<BatchResult> alignBatchVoxel(const std::vector<Matrix4>& guesses) { return alignBatchThrough(ngicp_voxel_align_batch, "alignBatchVoxel", guesses); }
  template <class Entry>
  std::vector<BatchResult> alignBatchThrough(Entry entry, const char* name, const std::vector<Matrix4>& guesses) {
    std::vector<BatchResult> out;
    if (!h_ || !input_ || !haveTarget() || guesses.empty()) return out;
    const size_t n = guesses.size();
    std::vector<float> g(n * 16), T(n * 16);
    std::vector<int> conv(n), nit(n);
    std::vector<double> H(n * 36);
    for (size_t i = 0; i < n; ++i) std::memcpy(&g[i * 16], guesses[i].data(), 16 * sizeof(float));
    if (entry(h_, n, g.data(), T.data(), conv.data(), nit.data(), H.data()) != NGICP_OK) {
      std::fprintf(stderr, "[NanoGICP] %s(): %s\n", name, ngicp_last_error(h_));
      return out;
    }
    out.resize(n);
    for (size_t i = 0; i < n; ++i) {
      std::memcpy(out[i].transformation.data(), &T[i * 16], 16 * sizeof(float));
      out[i].converged = conv[i] != 0;
      out[i].nr_iterations = nit[i];
      std::memcpy(out[i].hessian.data(), &H[i * 36], 36 * sizeof(double));
    }
    return out;
  }
  std::vector<double> getFitnessScores(const std::vector<Matrix4>& transforms, double max_range = std::numeric_limits<double>::max()) {
    std::vector<double> scores(transforms.size(), std::numeric_limits<double>::max());
    if (!h_ || transforms.empty()) return scores;
    std::vector<float> T(transforms.size() * 16);
    for (size_t i = 0; i < transforms.size(); ++i) std::memcpy(&T[i * 16], transforms[i].data(), 16 * sizeof(float));
    check(ngicp_fitness_score_batch(h_, transforms.size(), T.data(), max_range, scores.data(), nullptr), "getFitnessScores");
    return scores;
  }

  // ---- voxel fitness (include/ngicp.h "voxel fitness"): a pose scored against the voxel map the voxelized entries align against - the
  //      target's, the merged one or the rolling one.  getFitnessScore(s) need a target cloud and its exact index; these need neither, so
  //      they are what scores a pose on a rolling map.  Per source point the best neighbourhood slot's e^T (cov_v + R C_a R^T)^-1 e (no
  //      voxel-count factor) and squared distance to the voxel mean; a point is an inlier iff that term is <= max_mahalanobis; both
  //      scores are means over the inliers, DBL_MAX without any; n_matched / (source size) is the overlap.  ok false (and a line on
  //      stderr): the voxel mode is off, the rolling map is empty or there is no source.  Recipe: INTEGRATION.md.
  struct VoxelFitness {
    bool ok = false;
    double mahalanobis = std::numeric_limits<double>::max(), sqdist = std::numeric_limits<double>::max();
    size_t n_inliers = 0, n_matched = 0;
  };
  // the final transformation of the last align()
  VoxelFitness getVoxelFitness(double max_mahalanobis = std::numeric_limits<double>::max()) {
    VoxelFitness f;
    ngicp_voxel_fitness_t r;
    if (h_ && check(ngicp_voxel_fitness(h_, final_transformation_.data(), max_mahalanobis, &r), "getVoxelFitness")) f = fromRecord(r);
    return f;
  }
  // every transform in the same launches; entry i is bit for bit what the single call gives for transforms[i]
  std::vector<VoxelFitness> getVoxelFitnessScores(const std::vector<Matrix4>& transforms, double max_mahalanobis = std::numeric_limits<double>::max()) {
    std::vector<VoxelFitness> out(transforms.size());
    if (!h_ || transforms.empty()) return out;
    std::vector<float> T(transforms.size() * 16);
    std::vector<ngicp_voxel_fitness_t> r(transforms.size());
    for (size_t i = 0; i < transforms.size(); ++i) std::memcpy(&T[i * 16], transforms[i].data(), 16 * sizeof(float));
    if (check(ngicp_voxel_fitness_batch(h_, transforms.size(), T.data(), max_mahalanobis, r.data()), "getVoxelFitnessScores"))
      for (size_t i = 0; i < r.size(); ++i) out[i] = fromRecord(r[i]);
    return out;
  }
  // every source point's value at T, in the source cloud's order: the winning slot's term, squared distance and voxel number; -1 / -1 / -1
  // where the map has no voxel for the point.  Cleared (false) on an error.
  bool voxelFitnessPoints(const Matrix4& T, std::vector<double>& m, std::vector<double>& sqd, std::vector<int>& voxel) {
    const size_t n = input_ ? input_->size() : 0;
    m.assign(n, -1.0);
    sqd.assign(n, -1.0);
    voxel.assign(n, -1);
    if (h_ && check(ngicp_voxel_fitness_points(h_, T.data(), m.data(), sqd.data(), voxel.data(), n), "voxelFitnessPoints")) return true;
    m.clear();
    sqd.clear();
    voxel.clear();
    return false;
  }

  // ---- scan context (include/ngicp.h "scan context"): which earlier keyframe a scan revisits, and at what yaw.  A polar height
  //      descriptor of a cloud that is already on the device (which: 0 = the input source, 1 = the target, 2 = the scan preprocessPoints
  //      left there), a device-resident database of descriptors with dense ids in insertion order, and an exhaustive match over every
  //      column shift.  On an error: a line on stderr and false / -1 / an empty vector.  Recipe: INTEGRATION.md.
  struct ScanContextParams {
    int n_rings = 20, n_sectors = 60;
    float max_radius = 80.0f, z_offset = 2.0f;
  };
  struct ScanContextMatch {
    int id;
    double distance;
    int shift;
  };
  // a change clears the database; a refused value changes nothing
  bool setScanContextParams(int n_rings, int n_sectors, float max_radius, float z_offset) {
    return h_ && check(ngicp_scan_context_set_params(h_, n_rings, n_sectors, max_radius, z_offset), "setScanContextParams");
  }
  ScanContextParams getScanContextParams() const {
    ScanContextParams p;
    if (h_) check(ngicp_scan_context_get_params(h_, &p.n_rings, &p.n_sectors, &p.max_radius, &p.z_offset), "getScanContextParams");
    return p;
  }
  // the engine's tables: the squared ring edges (n_rings + 1) and the sector boundary directions (n_sectors floats, x and y interleaved)
  bool scanContextTables(std::vector<float>& ring_edges_squared, std::vector<float>& boundary_directions) {
    const ScanContextParams p = getScanContextParams();
    ring_edges_squared.assign((size_t)p.n_rings + 1, 0.f);
    boundary_directions.assign((size_t)p.n_sectors, 0.f);
    return h_ && check(ngicp_scan_context_tables(h_, ring_edges_squared.data(), boundary_directions.data()), "scanContextTables");
  }
  // n_rings x n_sectors floats, row-major by ring
  std::vector<float> computeScanContext(int which = 0) {
    const ScanContextParams p = getScanContextParams();
    std::vector<float> d((size_t)p.n_rings * p.n_sectors);
    if (!h_ || !check(ngicp_scan_context_compute(h_, which, d.data()), "computeScanContext")) d.clear();
    return d;
  }
  int addScanContext(int which = 0) {
    int id = -1;
    if (h_) check(ngicp_scan_context_add(h_, which, &id), "addScanContext");
    return id;
  }
  int addScanContextDescriptor(const std::vector<float>& desc) {
    const ScanContextParams p = getScanContextParams();
    int id = -1;
    if (desc.size() != (size_t)p.n_rings * p.n_sectors) {
      std::fprintf(stderr, "[NanoGICP] addScanContextDescriptor: the descriptor must hold n_rings x n_sectors floats\n");
      return id;
    }
    if (h_) check(ngicp_scan_context_add_descriptor(h_, desc.data(), &id), "addScanContextDescriptor");
    return id;
  }
  size_t numScanContexts() const {
    size_t n = 0;
    if (h_) ngicp_scan_context_count(h_, &n);
    return n;
  }
  std::vector<float> scanContext(int id) {
    const ScanContextParams p = getScanContextParams();
    std::vector<float> d((size_t)p.n_rings * p.n_sectors);
    if (!h_ || !check(ngicp_scan_context_get(h_, id, d.data()), "scanContext")) d.clear();
    return d;
  }
  void clearScanContexts() {
    if (h_) check(ngicp_scan_context_clear(h_), "clearScanContexts");
  }
  // distance and shift of the slot's cloud / of a host descriptor to every entry of [begin, end): entry g describes id begin + g (its id
  // is filled in); in id order, not ranked
  std::vector<ScanContextMatch> scanContextDistances(int which, size_t begin, size_t end) { return scanContextDistancesOf(which, nullptr, begin, end); }
  std::vector<ScanContextMatch> scanContextDistances(const std::vector<float>& desc, size_t begin, size_t end) {
    return descriptorFits(desc, "scanContextDistances") ? scanContextDistancesOf(-1, desc.data(), begin, end) : std::vector<ScanContextMatch>();
  }
  // the first min(top_k, end - begin) entries of [begin, end) ascending by (distance, id), selected on the device; top_k 1..64
  std::vector<ScanContextMatch> matchScanContext(int which, size_t begin, size_t end, int top_k = 1) { return matchScanContextOf(which, nullptr, begin, end, top_k); }
  std::vector<ScanContextMatch> matchScanContext(const std::vector<float>& desc, size_t begin, size_t end, int top_k = 1) {
    return descriptorFits(desc, "matchScanContext") ? matchScanContextOf(-1, desc.data(), begin, end, top_k) : std::vector<ScanContextMatch>();
  }
  // the rotation about z by shift * 2 pi / n_sectors: the guess that carries the query scan into the matched entry's frame when both
  // were taken at about the same place - for align() or, with its neighbours, alignBatch()
  Matrix4 scanContextGuess(int shift) const {
    const double a = (double)shift * (6.283185307179586476925286766559 / (double)getScanContextParams().n_sectors);
    Matrix4 T;
    set_identity(T);
    T(0, 0) = T(1, 1) = (float)std::cos(a);
    T(1, 0) = (float)std::sin(a);
    T(0, 1) = -T(1, 0);
    return T;
  }
  double scanContextKernelMs() const {
    double ms = 0.0;
    if (h_) ngicp_scan_context_kernel_ms(h_, &ms);
    return ms;
  }

  // ---- voxel pose search (include/ngicp.h "voxel pose search"): a lattice of poses - the base poses times a window of whole-voxel
  //      shifts - scored by the number of source points that land in occupied voxels of the map in force; the best few come back with
  //      their candidate poses, for alignBatchVoxel.  Scan context gives the yaw, this the translation.  On an error: a
  //      line on stderr and an empty vector.  Recipe: INTEGRATION.md.
  struct PoseSearchCandidate {
    int pose;       // index into the base poses
    int shift[3];   // (sx, sy, sz) in voxels
    int score;      // source points in occupied voxels, counted on cells
    Matrix4 T;      // the candidate pose: the base pose with its translation replaced by (float)((double)t + (double)s * resolution)
  };
  // T0 . Rz(k * step_rad), k = 0..n-1, the product taken in double and rounded once: base poses for voxelPoseSearch
  static std::vector<Matrix4> yawLattice(const Matrix4& T0, int n, double step_rad) {
    std::vector<Matrix4> out;
    for (int k = 0; k < n; ++k) {
      const double c = std::cos((double)k * step_rad), s = std::sin((double)k * step_rad);
      Matrix4 T = T0;
      for (int r = 0; r < 4; ++r) {
        const double a = (double)T0(r, 0), b = (double)T0(r, 1);
        T(r, 0) = (float)(a * c + b * s);
        T(r, 1) = (float)(b * c - a * s);
      }
      out.push_back(T);
    }
    return out;
  }
  static Matrix4 poseSearchCandidate(const Matrix4& T, const int shift[3], double resolution) {
    Matrix4 out = T;
    for (int a = 0; a < 3; ++a) {
      volatile double step = (double)shift[a] * resolution;  // (rounded on its own: never fused into the addition)
      out(a, 3) = (float)((double)T(a, 3) + step);
    }
    return out;
  }
  // the first min(top_k, B |S|) entries by descending score, then ascending pose, then ascending shift index; top_k 1..64,
  // ex, ey <= 31, ez <= 7, (2 ex + 1)(2 ey + 1)(2 ez + 1) <= 12288, B times that <= 2^24
  std::vector<PoseSearchCandidate> voxelPoseSearch(const std::vector<Matrix4>& poses, int ex, int ey, int ez, int top_k = 8) {
    std::vector<PoseSearchCandidate> out;
    if (!h_) return out;
    std::vector<float> T(poses.size() * 16);
    for (size_t i = 0; i < poses.size(); ++i) std::memcpy(&T[i * 16], poses[i].data(), 16 * sizeof(float));
    const size_t cap = (size_t)std::min(std::max(top_k, 1), 64);
    std::vector<int> pose(cap), shift(3 * cap), score(cap);
    size_t n = 0;
    if (!check(ngicp_voxel_pose_search(h_, poses.size(), poses.empty() ? nullptr : T.data(), ex, ey, ez, top_k, pose.data(), shift.data(), score.data(), &n), "voxelPoseSearch"))
      return out;
    pose_search_entries_ = poses.size() * (size_t)(2 * ex + 1) * (size_t)(2 * ey + 1) * (size_t)(2 * ez + 1);
    for (size_t i = 0; i < n; ++i) {
      PoseSearchCandidate c;
      c.pose = pose[i];
      for (int a = 0; a < 3; ++a) c.shift[a] = shift[3 * i + a];
      c.score = score[i];
      c.T = poseSearchCandidate(poses[(size_t)pose[i]], c.shift, voxel_resolution_);
      out.push_back(c);
    }
    return out;
  }
  // the last search's full volume [B][2 ez + 1][2 ey + 1][2 ex + 1]; empty when there has been none or the map has changed since
  std::vector<int> voxelPoseSearchScores() {
    std::vector<int> v(std::max<size_t>(pose_search_entries_, 1));
    if (!h_ || !check(ngicp_voxel_pose_search_scores(h_, v.data(), v.size()), "voxelPoseSearchScores")) v.clear();
    else v.resize(pose_search_entries_);
    return v;
  }
  double voxelPoseSearchKernelMs() const {
    double ms = 0.0;
    if (h_) ngicp_voxel_pose_search_kernel_ms(h_, &ms);
    return ms;
  }

  // ---- extensions with no reference counterpart (include/ngicp.h "keyframe store", "rigid transform"): the keyframes and the
  //      submap stay on the GPU.  In DLO they replace odom.cc:1174 (`keyframe_normals.push_back(gicp_s2s.getSourceCovariances())`)
  //      and odom.cc:830-833 (`setInputTarget(submap_cloud); setTargetCovariances(submap_normals)`); see INTEGRATION.md ----
  // adopt `producer`'s current source cloud + covariances as the next keyframe; returns its index (== DLO's keyframes.size() - 1)
  int addKeyframe(NanoGICP& producer) {
    int id = -1;
    check(ngicp_keyframe_add(h_, producer.h_, &id), "addKeyframe");
    return id;
  }
  // the same with the keyframe cloud = producer's current source transformed by T on the device (odom.cc:971-974 + 1166-1174)
  int addKeyframeTransformed(NanoGICP& producer, const Matrix4& T) {
    int id = -1;
    check(ngicp_keyframe_add_transformed(h_, producer.h_, T.data(), &id), "addKeyframeTransformed");
    return id;
  }
  // the same with the submap voxel filter in between (DLO's shipped configuration: vf_submap_use_, odom.cc:1160-1163)
  int addKeyframeTransformedFiltered(NanoGICP& producer, const Matrix4& T, float leaf) {
    int id = -1;
    check(ngicp_keyframe_add_transformed_filtered(h_, producer.h_, T.data(), leaf, &id), "addKeyframeTransformedFiltered");
    return id;
  }
  size_t numKeyframes() const { size_t n = 0; ngicp_keyframe_count(h_, &n); return n; }
  // target := concatenation of the given keyframes (cloud + covariances), assembled and indexed on the device; a call with
  // the id list of the current submap is a no-op.  Returns true when the target was rebuilt.
  bool setSubmapKeyframes(const std::vector<int>& ids) {
    int changed = 0;
    if (check(ngicp_submap_set(h_, ids.data(), ids.size(), &changed), "setSubmapKeyframes")) {
      target_.reset();
      device_target_ = true;
    }
    return changed != 0;
  }
  // ---- moving keyframes after a loop closure (include/ngicp.h "moving keyframes"; no counterpart in the reference) ----
  // keyframe ids[j] := Ts[j] applied to it, for all j in one launch on the device: the points by the float matrix as
  // pcl::transformPointCloud, the covariances rotated by its 3x3 block (nothing is recomputed).  All or nothing: false and a message on
  // stderr when the call is refused, and then no keyframe has changed.  The current target is left as it is; *submap_stale (optional)
  // is set when a moved keyframe belongs to the submap that is the target - the next setSubmapKeyframes rebuilds it, even with the same ids.
  bool transformKeyframes(const std::vector<int>& ids, const std::vector<Matrix4>& Ts, bool* submap_stale = nullptr) {
    if (submap_stale) *submap_stale = false;
    if (!h_) return false;
    if (ids.size() != Ts.size()) {
      std::fprintf(stderr, "[NanoGICP] transformKeyframes: one transform per id\n");
      return false;
    }
    std::vector<float> flat(Ts.size() * 16);
    for (size_t j = 0; j < Ts.size(); ++j)
      for (int e = 0; e < 16; ++e) flat[j * 16 + e] = Ts[j].data()[e];  // (column-major, as Eigen stores it)
    int stale = 0;
    if (!check(ngicp_keyframe_transform(h_, ids.data(), ids.size(), flat.data(), &stale), "transformKeyframes")) return false;
    if (submap_stale) *submap_stale = stale != 0;
    return true;
  }
  // keyframe `id` as the store holds it, in its original point order: the points (x, y, z; data[3] = 1) and the covariances
  bool getKeyframe(int id, PointCloudSource& cloud, CovVector& covs) {
    size_t n = 0;
    if (!h_ || !check(ngicp_keyframe_get(h_, id, nullptr, 0, nullptr, &n), "getKeyframe")) return false;
    std::vector<float> xyz(n * 3);
    covs.resize(n);
    if (n && !check(ngicp_keyframe_get(h_, id, xyz.data(), 12, reinterpret_cast<double*>(covs.data()), &n), "getKeyframe")) return false;
    cloud.resize(n);
    for (size_t i = 0; i < n; ++i) {
      PointSource& p = cloud.points[i];
      p.data[0] = xyz[i * 3 + 0]; p.data[1] = xyz[i * 3 + 1]; p.data[2] = xyz[i * 3 + 2]; p.data[3] = 1.0f;
    }
    return true;
  }
  double keyframeTransformKernelMs() const {
    double ms = 0.0;
    if (h_) ngicp_keyframe_transform_kernel_ms(h_, &ms);
    return ms;
  }
  // ---- pose graph (include/ngicp.h "pose graph"; no counterpart in the reference) ----
  // Loop-closure edges in, corrected keyframe poses out, on the device: nodes are world poses (double, column-major 4x4), edges carry the
  // measured T_i^-1 T_j and a symmetric 6x6 information matrix (rotation first).  The graph lives on this instance, survives alignments
  // and touches nothing of them.  Every call is all or nothing: false (or -1) and a line on stderr when it is refused.
  // The array forms come first; the matrix forms below them take types::Matrix4d / Matrix6d (Eigen's, or the stand-ins without Eigen).
  void poseGraphClear() {
    if (h_) check(ngicp_pose_graph_clear(h_), "poseGraphClear");
  }
  void poseGraphSize(size_t* nodes, size_t* edges) const {
    if (nodes) *nodes = 0;
    if (edges) *edges = 0;
    if (h_) ngicp_pose_graph_size(h_, nodes, edges);
  }
  // -> the first new id, or -1
  int poseGraphAddNodes(const double* T_colmajor_n16, const unsigned char* fixed_or_null, size_t n) {
    int first = -1;
    if (!h_ || !check(ngicp_pose_graph_add_nodes(h_, T_colmajor_n16, fixed_or_null, n, &first), "poseGraphAddNodes")) return -1;
    return first;
  }
  // info: n x 36, each exactly symmetric.  -> the first new edge id, or -1
  int poseGraphAddEdges(const int* ij_n2, const double* Z_colmajor_n16, const double* info_n36, const unsigned char* robust_or_null, size_t n) {
    int first = -1;
    if (!h_ || !check(ngicp_pose_graph_add_edges(h_, ij_n2, Z_colmajor_n16, info_n36, robust_or_null, n, &first), "poseGraphAddEdges")) return -1;
    return first;
  }
  bool poseGraphGetEdges(int first, size_t n, int* ij_n2, double* Z_colmajor_n16, double* info_n36, unsigned char* robust) {
    return h_ && check(ngicp_pose_graph_get_edges(h_, first, n, ij_n2, Z_colmajor_n16, info_n36, robust), "poseGraphGetEdges");
  }
  bool poseGraphSetFixed(const std::vector<int>& ids, const std::vector<unsigned char>& flags) {
    if (!h_ || ids.size() != flags.size()) return false;
    return check(ngicp_pose_graph_set_fixed(h_, ids.data(), flags.data(), ids.size()), "poseGraphSetFixed");
  }
  bool poseGraphGetFixed(int first, size_t n, unsigned char* flags) { return h_ && check(ngicp_pose_graph_get_fixed(h_, first, n, flags), "poseGraphGetFixed"); }
  // the kernel of the FLAGGED edges: NGICP_ROBUST_NONE / _HUBER / _CAUCHY / _GEMAN_MCCLURE and its width (whitened residual units)
  bool poseGraphSetRobust(int kind, double width) { return h_ && check(ngicp_pose_graph_set_robust(h_, kind, width), "poseGraphSetRobust"); }
  bool poseGraphGetPoses(int first, size_t n, double* T_colmajor_n16) { return h_ && check(ngicp_pose_graph_get_poses(h_, first, n, T_colmajor_n16), "poseGraphGetPoses"); }
  bool poseGraphSetPoses(int first, size_t n, const double* T_colmajor_n16) {
    return h_ && check(ngicp_pose_graph_set_poses(h_, first, n, T_colmajor_n16), "poseGraphSetPoses");
  }
  // test hooks: the linearisation at the current poses (any output may be null), and y = (H + lambda I) x
  bool poseGraphLinearize(double* chi2, double* edge_r_m6, double* edge_s_w_m2, double* grad_n6, double* diag_n36) {
    return h_ && check(ngicp_pose_graph_linearize(h_, chi2, edge_r_m6, edge_s_w_m2, grad_n6, diag_n36), "poseGraphLinearize");
  }
  bool poseGraphMultiply(double lambda, const double* x_n6, double* y_n6) { return h_ && check(ngicp_pose_graph_multiply(h_, lambda, x_n6, y_n6), "poseGraphMultiply"); }
  // Levenberg-Marquardt on the whole graph (options null: the defaults); refused while a connected component holds no fixed node
  bool poseGraphOptimize(const ngicp_pg_options* options, ngicp_pg_result* result) {
    return h_ && check(ngicp_pose_graph_optimize(h_, options, result), "poseGraphOptimize");
  }
  // C_k = T_k * T_k_old^-1 as float column-major 4x4s, what transformKeyframes / transformVoxelMap take; T_old null: the poses the last
  // poseGraphOptimize started from
  bool poseGraphCorrections(const int* ids, size_t n, const double* T_old_colmajor_n16_or_null, float* C_colmajor_n16) {
    return h_ && check(ngicp_pose_graph_corrections(h_, ids, n, T_old_colmajor_n16_or_null, C_colmajor_n16), "poseGraphCorrections");
  }
  double poseGraphKernelMs() const {
    double ms = 0.0;
    if (h_) ngicp_pose_graph_kernel_ms(h_, &ms);
    return ms;
  }
  // the matrix forms
  struct PoseGraphEdge {
    int i, j;
    types::Matrix4d Z;       // the measured T_i^-1 T_j
    types::Matrix6d info;    // exactly symmetric
    bool robust;
  };
  int poseGraphAddNodes(const std::vector<types::Matrix4d>& T, const std::vector<unsigned char>& fixed = std::vector<unsigned char>()) {
    if (!fixed.empty() && fixed.size() != T.size()) return -1;
    std::vector<double> flat(T.size() * 16);
    for (size_t k = 0; k < T.size(); ++k)
      for (int e = 0; e < 16; ++e) flat[k * 16 + e] = T[k].data()[e];
    return poseGraphAddNodes(flat.data(), fixed.empty() ? nullptr : fixed.data(), T.size());
  }
  int poseGraphAddEdges(const std::vector<PoseGraphEdge>& edges) {
    const size_t n = edges.size();
    std::vector<int> ij(n * 2);
    std::vector<double> Z(n * 16), L(n * 36);
    std::vector<unsigned char> f(n);
    for (size_t e = 0; e < n; ++e) {
      ij[2 * e] = edges[e].i, ij[2 * e + 1] = edges[e].j;
      for (int q = 0; q < 16; ++q) Z[e * 16 + q] = edges[e].Z.data()[q];
      for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) L[e * 36 + a * 6 + b] = edges[e].info(a, b);
      f[e] = edges[e].robust ? 1 : 0;
    }
    return poseGraphAddEdges(ij.data(), Z.data(), L.data(), f.data(), n);
  }
  bool poseGraphPoses(std::vector<types::Matrix4d>& out) {
    size_t n = 0;
    poseGraphSize(&n, nullptr);
    out.assign(n, types::Matrix4d::Identity());
    if (n == 0) return h_ != nullptr;
    std::vector<double> flat(n * 16);
    if (!poseGraphGetPoses(0, n, flat.data())) return false;
    for (size_t k = 0; k < n; ++k)
      for (int e = 0; e < 16; ++e) out[k].data()[e] = flat[k * 16 + e];
    return true;
  }
  bool poseGraphCorrections(const std::vector<int>& ids, std::vector<Matrix4>& Cs, const std::vector<types::Matrix4d>* T_old = nullptr) {
    if (T_old && T_old->size() != ids.size()) return false;
    std::vector<double> old(T_old ? ids.size() * 16 : 0);
    for (size_t k = 0; T_old && k < ids.size(); ++k)
      for (int e = 0; e < 16; ++e) old[k * 16 + e] = (*T_old)[k].data()[e];
    std::vector<float> flat(ids.size() * 16);
    if (!poseGraphCorrections(ids.data(), ids.size(), T_old ? old.data() : nullptr, flat.data())) return false;
    Cs.assign(ids.size(), Matrix4::Identity());
    for (size_t k = 0; k < ids.size(); ++k)
      for (int e = 0; e < 16; ++e) Cs[k].data()[e] = flat[k * 16 + e];
    return true;
  }
  // The edge an alignment yields.  Scan j was aligned against keyframe i, which is held in the world frame at T_i; the alignment ended at the
  // world pose T_aligned with getFinalHessian() = H, the information in the aligner's left perturbation of the world pose.  Z = T_i^-1
  // T_aligned, and Lambda = J^-T H J^-1 expresses H in the edge's residual coordinates: at the measurement r = J d with
  // J = [[A, 0], [-A [t]x, A]], A = R_aligned^T, t = t_aligned, so J^-1 = [[A^T, 0], [[t]x A^T, A^T]].  Lambda is
  // symmetrised exactly, as poseGraphAddEdges demands.
  static void edgeFromAlignment(const types::Matrix4d& T_i, const types::Matrix4d& T_aligned, const types::Matrix6d& H, types::Matrix4d& Z, types::Matrix6d& Lambda) {
    Z = types::Matrix4d::Identity();
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s += T_i(k, r) * T_aligned(k, c);
        Z(r, c) = s;
      }
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += T_i(k, r) * (T_aligned(k, 3) - T_i(k, 3));
      Z(r, 3) = s;
    }
    const double t[3] = {T_aligned(0, 3), T_aligned(1, 3), T_aligned(2, 3)};
    const double S[3][3] = {{0.0, -t[2], t[1]}, {t[2], 0.0, -t[0]}, {-t[1], t[0], 0.0}};
    double Ji[6][6] = {};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        Ji[r][c] = Ji[3 + r][3 + c] = T_aligned(r, c);
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s += S[r][k] * T_aligned(k, c);
        Ji[3 + r][c] = s;
      }
    double HJ[6][6], L[6][6];
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += H(a, k) * Ji[k][b];
        HJ[a][b] = s;
      }
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += Ji[k][a] * HJ[k][b];
        L[a][b] = s;
      }
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) Lambda(a, b) = 0.5 * (L[a][b] + L[b][a]);
  }
  // dlo::OdomNode::preprocessPoints (odom.cc:443-465): removeNaN -> CropBox(negative, +-crop_size) -> VoxelGrid(voxel_res), each
  // optional (crop_size / voxel_res <= 0: off), on the GPU; `cloud` is replaced by the filtered cloud (x, y, z, intensity;
  // data[3] = 1).  With set_as_source the filtered cloud, still on the device, also becomes this instance's input source.
  void preprocessPoints(PointCloudSource& cloud, bool remove_nan, float crop_size, float voxel_res, bool set_as_source = false) {
    if (!h_ || cloud.empty()) return;
    std::vector<float> out(cloud.size() * 4);
    size_t m = 0;
    const long ioff = (long)((const char*)&cloud.points[0].intensity - (const char*)cloud.points[0].data);
    if (!check(ngicp_preprocess_scan(h_, cloud.points[0].data, cloud.size(), sizeof(PointSource), ioff, remove_nan ? 1 : 0, crop_size, voxel_res, out.data(),
                                     cloud.size(), &m), "preprocessPoints"))
      return;
    cloud.resize(m);
    for (size_t i = 0; i < m; ++i) {
      PointSource& p = cloud.points[i];
      p.data[0] = out[i * 4 + 0]; p.data[1] = out[i * 4 + 1]; p.data[2] = out[i * 4 + 2]; p.data[3] = 1.0f;
      p.intensity = out[i * 4 + 3];
    }
    if (set_as_source) check(ngicp_set_source_preprocessed(h_, 0), "set_source_preprocessed");
  }
  // Motion deskew (ngicp.h "motion deskew"): every point of `cloud` moved by the trajectory's pose at its own time into the
  // trajectory's reference frame, on the GPU; `out` is `cloud` with new x, y, z.  false (and a line on stderr) on a refused argument.
  bool deskewCloud(const PointCloudSource& cloud, const DeskewTrajectory& traj, PointCloudSource& out) {
    if (!h_) return false;
    if (&out != &cloud) out = cloud;
    if (cloud.empty()) return true;
    const ngicp_deskew_t d = traj.describe();
    std::vector<float> xyz(cloud.size() * 3);
    if (!check(ngicp_deskew_cloud(h_, cloud.points[0].data, cloud.size(), sizeof(PointSource), &d, xyz.data(), 12), "deskewCloud")) return false;
    for (size_t i = 0; i < out.size(); ++i) {
      out.points[i].data[0] = xyz[i * 3 + 0];
      out.points[i].data[1] = xyz[i * 3 + 1];
      out.points[i].data[2] = xyz[i * 3 + 2];
    }
    return true;
  }
  // preprocessPoints with the deskew applied where the scan is unpacked on the device: the deskewed scan never exists on the host.
  // With remove_nan, points whose time is not finite are dropped.  false on a refused argument: `cloud` is left as it was.
  bool preprocessScanDeskewed(PointCloudSource& cloud, const DeskewTrajectory& traj, bool remove_nan, float crop_size, float voxel_res, bool set_as_source = false) {
    if (!h_) return false;
    if (cloud.empty()) return true;
    const ngicp_deskew_t d = traj.describe();
    std::vector<float> out(cloud.size() * 4);
    size_t m = 0;
    const long ioff = (long)((const char*)&cloud.points[0].intensity - (const char*)cloud.points[0].data);
    if (!check(ngicp_preprocess_scan_deskewed(h_, cloud.points[0].data, cloud.size(), sizeof(PointSource), ioff, &d, remove_nan ? 1 : 0, crop_size, voxel_res,
                                              out.data(), cloud.size(), &m), "preprocessScanDeskewed"))
      return false;
    cloud.resize(m);
    for (size_t i = 0; i < m; ++i) {
      PointSource& p = cloud.points[i];
      p.data[0] = out[i * 4 + 0]; p.data[1] = out[i * 4 + 1]; p.data[2] = out[i * 4 + 2]; p.data[3] = 1.0f;
      p.intensity = out[i * 4 + 3];
    }
    if (set_as_source) return check(ngicp_set_source_preprocessed(h_, 0), "set_source_preprocessed");
    return true;
  }
  // dlo::MapNode (map.cc:100-131): `*dlo_map += *keyframe` and `voxelgrid.filter(*dlo_map)` on a device-resident map
  void mapAdd(const PointCloudSource& keyframe) {
    if (!h_ || keyframe.empty()) return;
    const long ioff = (long)((const char*)&keyframe.points[0].intensity - (const char*)keyframe.points[0].data);
    check(ngicp_map_add(h_, keyframe.points[0].data, keyframe.size(), sizeof(PointSource), ioff), "mapAdd");
  }
  size_t mapVoxelFilter(float leaf) { size_t m = 0; check(ngicp_map_voxel_filter(h_, leaf, &m), "mapVoxelFilter"); return m; }
  void mapGet(PointCloudSource& out) {
    size_t n = 0;
    ngicp_map_size(h_, &n);
    std::vector<float> buf(n * 4);
    if (n && !check(ngicp_map_get(h_, buf.data(), n), "mapGet")) return;
    out.resize(n);
    for (size_t i = 0; i < n; ++i) {
      PointSource& p = out.points[i];
      p.data[0] = buf[i * 4 + 0]; p.data[1] = buf[i * 4 + 1]; p.data[2] = buf[i * 4 + 2]; p.data[3] = 1.0f;
      p.intensity = buf[i * 4 + 3];
    }
  }
  // pcl::transformPointCloud(*getInputSource(), out, T) computed from the device-resident source (odom.cc:971-974)
  void transformSource(PointCloudSource& out, const Matrix4& T) {
    if (!h_ || !input_) return;
    out = *input_;
    std::vector<float> xyz_out(input_->size() * 3);
    if (!check(ngicp_transform_source(h_, T.data(), xyz_out.data(), 12), "transformSource")) return;
    for (size_t i = 0; i < out.size(); ++i) {
      out.points[i].data[0] = xyz_out[i * 3 + 0];
      out.points[i].data[1] = xyz_out[i * 3 + 1];
      out.points[i].data[2] = xyz_out[i * 3 + 2];
    }
  }

 public:  // the reference's public data members (nano_gicp.hpp:120-125)
  IndexRef source_kdtree_, target_kdtree_;
  CovRef source_covs_, target_covs_;

 protected:
  CovVector fetch(bool source) const {
    size_t n = 0;
    if (source) ngicp_source_covs_size(h_, &n); else ngicp_target_covs_size(h_, &n);
    CovVector v(n);
    static_assert(sizeof(typename CovVector::value_type) == 16 * sizeof(double), "Matrix4d must be 16 doubles");
    if (n) (source ? ngicp_get_source_covs : ngicp_get_target_covs)(h_, reinterpret_cast<double*>(v.data()));
    return v;
  }
  // is there something to align against: a host target, a device submap, or (voxel mode with the rolling setting) the rolling map
  bool haveTarget() const { return target_ || device_target_ || (voxel_rolling_ && voxel_resolution_ > 0.0); }
  bool check(int rc, const char* what) const {
    if (rc != NGICP_OK) std::fprintf(stderr, "[NanoGICP] %s: %s\n", what, h_ ? ngicp_last_error(h_) : "no engine");
    return rc == NGICP_OK;
  }
  void push() {
    if (!h_) return;
    check(ngicp_set_params(h_, k_correspondences_, corr_dist_threshold_, max_iterations_, transformation_epsilon_, rotation_epsilon_,
                           lsq_optimizer_type_ == LSQ_OPTIMIZER_TYPE::LevenbergMarquardt ? 1 : 0, lm_max_iterations_, lm_init_lambda_factor_,
                           (int)regularization_method_, num_threads_), "set_params");
  }
  template <class CloudPtr> static const float* xyz(const CloudPtr& c) { return c->size() ? c->points[0].data : nullptr; }
  template <class CloudPtr> static uint64_t id(const CloudPtr& c) { return (uint64_t)(uintptr_t)c.get(); }
  static VoxelFitness fromRecord(const ngicp_voxel_fitness_t& r) {
    VoxelFitness f;
    f.ok = true;
    f.mahalanobis = r.mahalanobis;
    f.sqdist = r.sqdist;
    f.n_inliers = r.n_inliers;
    f.n_matched = r.n_matched;
    return f;
  }
  bool descriptorFits(const std::vector<float>& desc, const char* what) const {
    const ScanContextParams p = getScanContextParams();
    if (desc.size() == (size_t)p.n_rings * p.n_sectors) return true;
    std::fprintf(stderr, "[NanoGICP] %s: the descriptor must hold n_rings x n_sectors floats\n", what);
    return false;
  }
  std::vector<ScanContextMatch> scanContextDistancesOf(int which, const float* desc, size_t begin, size_t end) {
    std::vector<ScanContextMatch> out;
    if (!h_) return out;
    const size_t n = end > begin ? end - begin : 0;
    std::vector<double> dist(n + 1);
    std::vector<int> shift(n + 1);
    if (!check(ngicp_scan_context_distances(h_, which, desc, begin, end, dist.data(), shift.data()), "scanContextDistances")) return out;
    for (size_t g = 0; g < n; ++g) out.push_back(ScanContextMatch{(int)(begin + g), dist[g], shift[g]});
    return out;
  }
  std::vector<ScanContextMatch> matchScanContextOf(int which, const float* desc, size_t begin, size_t end, int top_k) {
    std::vector<ScanContextMatch> out;
    if (!h_) return out;
    int ids[64], shift[64];
    double dist[64];
    size_t n = 0;
    if (!check(ngicp_scan_context_match(h_, which, desc, begin, end, top_k, ids, dist, shift, &n), "matchScanContext")) return out;
    for (size_t g = 0; g < n; ++g) out.push_back(ScanContextMatch{ids[g], dist[g], shift[g]});
    return out;
  }
  static void set_identity(Matrix4& m) { for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m(r, c) = r == c ? 1.f : 0.f; }

  ngicp_t* h_ = nullptr;
  PointCloudSourceConstPtr input_;
  PointCloudTargetConstPtr target_;
  bool device_target_ = false;  // the target is a device-assembled submap (setSubmapKeyframes): no host cloud behind it
  // defaults: impl/nano_gicp_impl.hpp:50-64, impl/lsq_registration_impl.hpp:50-63
  int num_threads_ = 0;
  int k_correspondences_ = 20;
  RegularizationMethod regularization_method_ = RegularizationMethod::PLANE;
  double corr_dist_threshold_ = (double)std::numeric_limits<float>::max();
  int max_iterations_ = 64;
  double transformation_epsilon_ = 5e-4;
  double rotation_epsilon_ = 2e-3;
  LSQ_OPTIMIZER_TYPE lsq_optimizer_type_ = LSQ_OPTIMIZER_TYPE::LevenbergMarquardt;
  int lm_max_iterations_ = 10;
  double lm_init_lambda_factor_ = 1e-9;
  bool lm_debug_print_ = false;
  Matrix4 final_transformation_;
  types::Matrix6d final_hessian_;
  bool converged_ = false;
  int nr_iterations_ = 0;
  double voxel_resolution_ = 0.0;
  size_t pose_search_entries_ = 0;  // B |S| of the last successful voxelPoseSearch: what voxelPoseSearchScores asks for
  bool voxel_rolling_ = false;
  mutable CovVector cache_src_, cache_tgt_;
};

}  // namespace nano_gicp
