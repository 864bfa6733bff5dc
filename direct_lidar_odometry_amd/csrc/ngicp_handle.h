// The handle behind the C ABI (include/ngicp.h) and what its host code is written with: the error types, grow-only device buffers,
// indexed clouds and their pools, the registry of live handles, struct ngicp itself and the guard every entry point runs under.
// Part of ngicp_api.hip's translation unit (included there, after the kernel headers).
#pragma once

namespace {

thread_local std::string g_create_error;

struct HipError {
  hipError_t code;
  const char* what;
  const char* file;
  int line;
};

#define HIP_TRY(expr)                                          \
  do {                                                         \
    hipError_t _e = (expr);                                    \
    if (_e != hipSuccess) throw HipError{_e, #expr, __FILE__, __LINE__}; \
  } while (0)

struct ArgError {
  int code;
  std::string msg;
};

double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

std::atomic<long long> g_device_allocs{0};  // hipMalloc calls of the engine's buffers (ngicp_stats::device_allocs)

// grow-only device buffer
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    if (p) HIP_TRY(hipFree(p));
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 4 + 256;
    HIP_TRY(hipMalloc(&p, want));
    g_device_allocs.fetch_add(1, std::memory_order_relaxed);
    cap = want;
  }
  bool ensure_grew(size_t bytes) {  // true when the buffer was (re)allocated: its contents are gone
    const void* before = p;
    ensure(bytes);
    return p != before;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

// An uploaded, cell-sorted, indexed cloud.  Shared between handles (odom.cc:525) and between the
// source/target slots (swapSourceAndTarget) through shared_ptr.
struct DeviceCloud {
  size_t n = 0;
  DevBuf sorted;      // float4[kSortedPad + n + kSortedPad]: the cell-sorted points between two runs of far-away sentinels, so
                      // that the 8-point windows of the search may overhang the array's ends without index clamps
  float4* pts() const { return sorted.as<float4>() + kSortedPad; }
  DevBuf sorted3;     // Xyz[kSortedPad + n + kSortedPad]: the same points and sentinels, 12 bytes each (the pass kernel's walks)
  Xyz* xyz3() const { return sorted3.as<Xyz>() + kSortedPad; }
  DevBuf sortedp;     // float4[kSortedPad + n + kSortedPad]: the same points and sentinels, w = sorted position (what the staged pass copies to LDS)
  float4* xyzp() const { return sortedp.as<float4>() + kSortedPad; }
  DevBuf perm;        // int[n]    sorted position -> original index
  DevBuf inv_perm;    // int[n]    original index -> sorted position (lazily built)
  bool has_inv = false;
  DevBuf cell_start;  // int[kCellPad + ncells + 1 + kCellPad]: the exclusive prefix of points per cell, framed by kCellPad entries on each side (0 in
                      // front, n behind) so that the pass may fetch the four bounds around a cell with ONE 16-byte load at any cell
  int* cells() const { return cell_start.as<int>() + kCellPad; }
  DevBuf cell_box;    // uint[kCellPad + ncells + kCellPad]: the (y,z) extent of every cell's points inside the cell (k_cell_boxes), framed by
                      // empty boxes; only when the building handle had NGICP_CELL_BOXES on
  bool has_boxes = false;
  DevBuf qpts;        // float4[n]  the points in Morton-tile query order, w = sorted position
  DevBuf batches;     // int2[n_batches] {first qpts index, count <= 32}: tile-aligned query batches
  DevBuf n_batches_dev;
  DevBuf batch_boxes; // float[n_batches][6] centre + half extents of each batch (cloud frame)
  int n_batches = 0;
  Grid grid{};
  float bb_min[3] = {0.f, 0.f, 0.f}, bb_max[3] = {0.f, 0.f, 0.f};  // bounding box of the points (a submap's box is the union of its keyframes')
  double build_ms = 0.0;
  int device = 0;
  // STORAGE ONLY (a keyframe that ngicp_keyframe_transform moved): `sorted` holds the points in the order the keyframe had
  // before the move (w = original index; the pads unwritten), n and the box are valid, and NOTHING else is - no grid, no permutation, no
  // batches.  Such a cloud is read by position only (ngicp_submap_set, the voxel part, ngicp_keyframe_get); refuse_storage_only() guards
  // every place a cloud is about to be searched.  It is made outside the pool below and freed, not recycled, with its keyframe.
  bool storage_only = false;
};

void refuse_storage_only(const DeviceCloud& dc, const char* what) {
  if (dc.storage_only) throw ArgError{NGICP_ERR_STATE, std::string(what) + ": the cloud is a moved keyframe's storage and has no index"};
}

// Index objects are recycled: a LiDAR pipeline builds a new source index per scan, and hipMalloc / hipFree of its nine
// buffers (both synchronise the device) cost more than building the index.  The last owner hands the object back to a
// per-process pool; a build takes one of the right device from it and only grows the buffers that are too small.
struct CloudPool {
  std::mutex m;
  std::vector<DeviceCloud*> free_list;
};
CloudPool& cloud_pool() {
  static CloudPool* p = new CloudPool;  // never destroyed: device memory must not be freed after the HIP runtime has shut down
  return *p;
}
// the same for covariance sets (one per scan, 48 bytes per point)
struct BufPool {
  std::mutex m;
  std::vector<std::pair<int, DevBuf*>> free_list;  // {device, buffer}
};
BufPool& buf_pool() {
  static BufPool* p = new BufPool;
  return *p;
}
// A recycled object may still be read by work that ANOTHER handle has in flight (a shared source index, a keyframe's covariance
// set).  Instead of a device-wide, host-blocking hipDeviceSynchronize() the acquiring handle's stream waits - on the device - for
// what every live handle of the same GPU has enqueued so far: one event record + one stream wait per handle (DLO has two).
struct HandleRegistry {
  std::mutex m;
  std::vector<ngicp*> live;
};
HandleRegistry& registry() {
  static HandleRegistry* r = new HandleRegistry;
  return *r;
}
void fence_engine_streams(ngicp* h);  // defined below struct ngicp

std::shared_ptr<DevBuf> acquire_buf(ngicp* h, int device, size_t bytes) {
  DevBuf* b = nullptr;
  {
    BufPool& bp = buf_pool();
    std::lock_guard<std::mutex> lock(bp.m);
    size_t best = bp.free_list.size();
    for (size_t i = 0; i < bp.free_list.size(); ++i)  // best fit: a scan's set must not take the submap's buffer
      if (bp.free_list[i].first == device && bp.free_list[i].second->cap >= bytes &&
          (best == bp.free_list.size() || bp.free_list[i].second->cap < bp.free_list[best].second->cap))
        best = i;
    if (best < bp.free_list.size()) {
      b = bp.free_list[best].second;
      bp.free_list.erase(bp.free_list.begin() + (long)best);
    }
  }
  if (b) {
    fence_engine_streams(h);  // previous owners' work on other streams
  } else {
    b = new DevBuf;
    b->ensure(bytes);
  }
  return std::shared_ptr<DevBuf>(b, [device](DevBuf* p) {
    BufPool& bp = buf_pool();
    std::lock_guard<std::mutex> lock(bp.m);
    if (bp.free_list.size() < 12) bp.free_list.emplace_back(device, p);
    else delete p;
  });
}

std::shared_ptr<DeviceCloud> acquire_cloud(ngicp* h, int device) {
  DeviceCloud* dc = nullptr;
  {
    CloudPool& cp = cloud_pool();
    std::lock_guard<std::mutex> lock(cp.m);
    for (size_t i = 0; i < cp.free_list.size(); ++i)
      if (cp.free_list[i]->device == device) {
        dc = cp.free_list[i];
        cp.free_list.erase(cp.free_list.begin() + (long)i);
        break;
      }
  }
  if (dc) {
    // its previous owners may still have work in flight on their streams that reads the buffers
    fence_engine_streams(h);
    dc->n = 0;
    dc->has_inv = false;
    dc->n_batches = 0;
    dc->build_ms = 0.0;
  } else {
    dc = new DeviceCloud;
    dc->device = device;
  }
  return std::shared_ptr<DeviceCloud>(dc, [](DeviceCloud* p) {
    CloudPool& cp = cloud_pool();
    std::lock_guard<std::mutex> lock(cp.m);
    if (cp.free_list.size() < 8) cp.free_list.push_back(p);
    else delete p;
  });
}

// Covariances, packed symmetric FP64 [n][6], stored in the sorted order of `order`.
struct CovSet {
  std::shared_ptr<DevBuf> data;
  size_t n = 0;
  std::shared_ptr<DeviceCloud> order;
  void clear() {
    data.reset();
    order.reset();
    n = 0;
  }
};

struct Slot {
  std::shared_ptr<DeviceCloud> dev;
  const float* host = nullptr;  // pending (registered, not yet uploaded) cloud
  size_t n = 0;
  size_t stride = 0;
  uint64_t identity = 0;
  bool present = false;
  void clear() {
    dev.reset();
    host = nullptr;
    n = stride = 0;
    identity = 0;
    present = false;
  }
};

// What a voxelized pass reads of a voxel map, whoever filled it: the target's map (ngicp::VoxelMap) or the rolling map (ngicp::RollMap).
struct VoxelMapView {
  const ulonglong2* table;
  unsigned int mask;
  const double* rec;
  const unsigned long long* vkeys;
  size_t n_vox;
};

struct LoopCtx;  // the per-alignment launch arguments (defined with the registration loop)
using route::kMaxPersistPasses;
constexpr int kMaxTickPasses = 1024;  // passes of an alignment whose timestamps the persistent kernel records when profiling is on
constexpr int kShardSlots = 4, kShardLag = 2;  // point-sharded stepping: the `done` word of step k is read at step k + kShardLag
constexpr float kIdentity16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

struct Params {
  int k = 20;                                                       // impl/nano_gicp_impl.hpp:57
  double max_corr_dist = (double)std::numeric_limits<float>::max(); // :59
  int max_iter = 64;                                                // impl/lsq_registration_impl.hpp:52
  double trans_eps = 5e-4;                                          // :54
  double rot_eps = 2e-3;                                            // :53
  int optimizer = NGICP_OPT_LEVENBERG_MARQUARDT;                    // :56
  int lm_max_iter = 10;                                             // :58
  double lm_init_lambda_factor = 1e-9;                              // :59
  int regularization = NGICP_REG_PLANE;                             // impl/nano_gicp_impl.hpp:61
  int num_threads = 0;
};
// the most passes an alignment can take: one per Gauss-Newton iteration; one per LM trial, and the linearisation the last trial leaves
inline long max_passes(const Params& p) { return p.optimizer == NGICP_OPT_GAUSS_NEWTON ? (long)p.max_iter : (long)p.max_iter * std::max(1, p.lm_max_iter) + 1; }
// rows the LM trace is sized for (one more of 256 bytes each: the persistent kernel's ring of per-pass views)
inline int max_trace_rows(const Params& p) { return std::max(1, p.max_iter) * std::max(1, p.lm_max_iter) + 1; }

// Working set of ngicp_align_batch and ngicp_voxel_align_batch (4.9): everything an alignment writes, once per lane, in
// buffers of its own - the handle's single-alignment state is not touched.  Grow-only, reused from call to call.  The two entries share
// the records, the rows, the traces and the pinned words (one call runs at a time on a handle); each has its own correspondence state.
struct BatchWs {
  DevBuf recs;      // the lane records, one upload per call: [cap] LmState images, then [cap] PassArgs or VoxelPassArgs, then [cap] SolveArgs
  DevBuf tpt, mahal;  // [lanes][2][n_src] float4 / [lanes][2][n_src][6] double
  DevBuf partials, order, cost, far, trace;  // [lanes][groups][32]; [lanes][groups] launch order / cost; [lanes][batches]; [lanes][rows][8]
  DevBuf flags;     // [lanes] x {order flag, ticket, -, -}
  DevBuf vox_corr, vox_mahal;  // ngicp_voxel_align_batch: [lanes][2][K][n_src] voxel numbers / [lanes][2][K][n_src][6] n_v M (2 * K * 52 bytes a point and lane)
  DevBuf fit_T, fit_part, fit_out;  // ngicp_fitness_score_batch
  unsigned char* pin_recs = nullptr;  // pinned image of `recs` (kBatchMaxLanes lanes)
  int* pin_progress = nullptr;        // pinned [kBatchMaxLanes] x kProgressStride: a lane's {passes done | kProgressDone}
  LmHot* pin_final = nullptr;         // pinned [kBatchMaxLanes]: a lane's state image when it is done
  const void* order_src = nullptr;    // source index / group count / lanes the launch orders on the device were built for
  int order_groups = -1, order_lanes = 0;
  int lanes = 0;                      // lanes of the last call of either entry (ngicp_batch_get_lm_trace)
  size_t trace_stride = 0;            // doubles between two lanes' traces
  std::vector<size_t> trace_rows;     // rows of each lane's trace on the device
  static constexpr int kProgressStride = 16;  // a 64-byte line per lane's word
};

}  // namespace

struct ngicp {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  hipEvent_t ev_cov_a = nullptr, ev_cov_b = nullptr;  // around the last covariance kernel; read lazily (ngicp_get_stats)
  hipEvent_t ev_fence = nullptr;                       // stream_wait_for()
  bool cov_timing_pending = false;
  std::string err;
  Params p;
  route::HandleSwitches sw;  // the NGICP_* switches read in ngicp_create (ngicp_route.h); never written afterwards
  double voxel_size = 0.0;  // the grid's voxel edge, 0 = auto: sw.voxel until ngicp_set_tuning writes it
  int host_wait = 0;        // 0: poll without giving the core up, 1: sched_yield between polls (ngicp_set_host_wait)
  CovSet shard_covs[2];     // covariance sets being computed in blocks by several ranks (ngicp_covs_shard_*), uncommitted
  // {cloud size, auto voxel edge} of recent builds, one entry per size class (a factor of two around the size): a DLO pipeline has three
  // or four - the scan, the voxel-filtered keyframe made from it, the submap - and each would otherwise pay the refinement passes again
  std::pair<size_t, double> voxel_memo[4] = {{0, 0.0}, {0, 0.0}, {0, 0.0}, {0, 0.0}};
  int voxel_memo_next = 0;
  bool profiling = false;
  int prof_stride = 1;      // time every prof_stride-th pass launch (events between kernels cost a few microseconds each)

  Slot src, tgt;
  CovSet src_covs, tgt_covs;

  // workspaces
  DevBuf raw, unsorted, keys, counts, fill, tile_sums, tile_sq, tmp, bbox, occ;
  int pass_slots = 768;  // blocks of the 3-waves-per-SIMD pass kernel resident on this device at once
  int persist_slots = 0; // blocks of the persistent pass kernel resident at once (its grid), 0: not available
  int queue_slots[2] = {768, 1024};  // blocks of k_gicp_queue<2, 3> / <2, 4> resident at once
  int persist = 0;       // sw.persist until a persistent launch fails or gives up (align_persistent clears it): ONE launch per alignment
                         // (k_gicp_persist).  Exact and complete, but measured no faster than one launch per pass: off by default
  int order_sel = 0;     // which of the two launch-order buffers (and flag words) the next alignment reads
  DevBuf grp_order_alt;  // the second order buffer: the persistent kernel's solver builds the NEXT alignment's order there
  DevBuf gen_lines;      // the persistent kernel's release word, kGenLines copies (PassArgs::gen)
  DevBuf state_alt;      // k_gicp_head: the second state buffer (a launch's solver block writes the one its blocks are not reading)
  DevBuf head_ws;        // k_gicp_head: {done flag (64 B), subset tickets (128 B), subset rows of even / odd launches (2 x 8 KB)}
  unsigned long long* pin_ticks = nullptr;  // pinned [2 * kMaxTickPasses]: per pass {last block arrived, next pass released} (profiling)
  double prev_staged_fraction = -1.0;  // share of the queries the previous alignment served through row lists (-1: none yet)
  DevBuf dbg, dbg_q, dbg_s, dbg_span, grp_order, grp_cost, batch_far;
  const void* order_src = nullptr;  // source index / group count the contents of grp_order were built for
  int order_groups = -1;
  DevBuf tpt[2], mahal[2], partials, state, trace, tfinal, out_xyz, scratch16, queries, knn_idx, knn_d2, sums, ticket;
  // queries on the indexed clouds (ngicp_query.h): fitness score, radius search (results of the last search stay on the device)
  DevBuf fit_T, fit_part, fit_out, rad_counts, rad_offsets, rad_keys, rad_long;
  size_t rad_total = 0;
  bool rad_valid = false;
  DevBuf range_ws;  // ngicp_range_select (ngicp_range.h): three rounds' histograms + the record; nothing else lives here
  hipEvent_t ev_q_a = nullptr, ev_q_b = nullptr;  // around the kernels of the last query call (ngicp_stats::query_ms)
  std::vector<hipEvent_t> prof_events;  // pairs around each pass launch when profiling is on
  int* h_progress = nullptr;  // pinned: {passes done | kProgressDone}, written by the solver (SolveArgs::progress_host)
  LmState* pin_state = nullptr;  // pinned [2]: the state image an align uploads / the one it reads back (no staging copies)
  LmHot* pin_final = nullptr;    // pinned: the state image the solver writes when an alignment is done (SolveArgs::final_host)
  DevBuf order_flag, t_first;    // device words {order flag 0, ticket, gen, order flag 1}: grp_order / grp_order_alt holds a complete order, the
                                 // fused / persistent kernels' ticket and released-pass counter; 100 MHz stamp of the alignment's first pass
  int hook_valid = 0;     // 1: the linearize hook has produced correspondences; 2: an align has (indices of its last linearisation)

  // results of the last align
  float final_T[16];
  double final_hessian[36];
  int converged = 0, nr_iterations = 0;
  std::vector<double> trace_host;
  size_t trace_rows_dev = 0;  // rows of the last align's LM trace still on the device
  ngicp_stats stats{};

  BatchWs batch;  // ngicp_align_batch / ngicp_fitness_score_batch

  // sharded stepping
  bool sharded_active = false;
  std::shared_ptr<LoopCtx> shard_ctx;      // the loop context of the alignment being stepped (one prepare_loop per alignment)
  hipEvent_t ev_shard[kShardSlots] = {};   // behind the copy of the `done` word of step k (slot k mod kShardSlots)
  int* h_shard_done = nullptr;             // pinned [kShardSlots]
  long shard_steps = 0;
  hipStream_t shard_stream = nullptr;      // the stream the last step was enqueued on

  // scan preprocessing / map voxel filter
  FilterWorkspace fws;
  DevBuf xyzi, map_pts;      // the unpacked input of a filter call; the accumulated map, float4 {x, y, z, intensity}
  size_t map_n = 0;
  const float4* filt_out = nullptr;  // result of the last preprocess call (device memory of fws / xyzi), filt_n points
  int filt_n = 0;

  // device-resident keyframe store (src/dlo/odom.cc keyframes + keyframe_normals) and the submap assembled from it
  // A keyframe's voxel part: its own per-voxel sums at one resolution, 88 bytes per occupied voxel.  Built lazily, by a
  // merged voxel-map build or ngicp_keyframe_voxelmap_get; replaced when the resolution differs; gone with the keyframe.
  struct VoxelPart {
    double res = 0.0;
    size_t n_vox = 0;
    DevBuf keys, rec;                    // [n_vox] keys ascending, [n_vox][kVoxRec] {sum p 3, sum C 6, count}
  };
  struct Keyframe {
    std::shared_ptr<DeviceCloud> cloud;  // indexed, cell-sorted
    std::shared_ptr<DevBuf> covs;        // [n][6] FP64 in the cloud's sorted order
    std::shared_ptr<VoxelPart> part;     // null until asked for
  };
  std::vector<Keyframe> keyframes;
  std::vector<int> submap_ids;           // keyframes of the submap that is the current target (valid while submap_cloud is the target)
  const DeviceCloud* submap_cloud = nullptr;
  bool submap_moved = false;             // ngicp_keyframe_transform moved a keyframe of submap_ids since ngicp_submap_set built the target from them
  std::weak_ptr<DevBuf> submap_covs;     // the covariance set ngicp_submap_set installed with it (weak: a recycled buffer is another object)

  // robust kernel (include/ngicp.h "robust kernel"): remembered across mode switches, read when a pass's arguments are filled
  int robust_kind = NGICP_ROBUST_NONE;
  double robust_width = 1.0;
  DevBuf robust_s, robust_w;             // ngicp_robust_terms: [n_src][K] doubles each

  // pose prior (include/ngicp.h "pose prior"): remembered across mode switches; every SolveArgs is filled from it
  bool prior_set = false;
  double prior_T[16] = {}, prior_info[36] = {};  // as given (column-major), for ngicp_get_pose_prior
  DevBuf prior_dev, prior_out;           // the record the solver reads (kPriorDoubles); ngicp_pose_prior_terms' 28 + 6 doubles

  // voxelized GICP (ngicp_voxel.h)
  double voxel_res = 0.0;  // ngicp_set_voxel_resolution: > 0 selects the mode
  int voxel_nbr = NGICP_VOX_DIRECT1;  // ngicp_set_voxel_neighbors: slots per source point (1, 7, 27); remembered while the mode is off
  long long voxel_builds = 0;         // voxel maps built on this handle (ngicp_voxelmap_builds): only ensure_voxel_map adds to it
  struct VoxelMap {
    bool valid = false;
    double res = 0.0;                    // the resolution it was built with
    std::shared_ptr<DeviceCloud> cloud;  // the target and the covariance set it was built from, HELD: a recycled object cannot take their addresses
    std::shared_ptr<DevBuf> covs;
    size_t n_vox = 0;
    int merged = 0;                      // the route it was built by: 0 from the target's points, 1 from the submap's keyframe parts
    unsigned int mask = 0;               // hash table slots - 1
    DevBuf rec, vkeys, table;            // [n_vox][kVoxRec] doubles, [n_vox] keys, [mask + 1] {key, voxel number}
    void invalidate() {
      valid = false;
      cloud.reset();
      covs.reset();
      n_vox = 0;
    }
  } vmap;
  FilterWorkspace vox_ws;                // the radix sort's scratch (its own: a preprocess result lives in fws)
  DevBuf vox_keys, vox_vals, vox_scan, vox_flag, vox_corr[2];
  DevBuf vox_mahal[2], vox_corr_out;     // DIRECT7 / DIRECT27: [K][n_src][6] n_v M per slot (DIRECT1 uses the exact path's mahal); the n x K export
  hipEvent_t ev_vox_a = nullptr, ev_vox_b = nullptr;
  // the submap's map merged from keyframe parts (ngicp_set_voxel_submap_merge)
  int voxel_merge = 0;                   // the setting; remembered while the voxel mode is off
  long long merged_builds = 0, parts_built = 0;  // maps built by the merged route / keyframe parts built, since the handle was created
  double last_parts_ms = 0.0, last_merge_ms = 0.0;  // event times of the last merged build: its part builds, the merge itself
  DevBuf vox_part_tab;                   // a merged build's table: [m + 1] int offsets, then (8-byte aligned) [m] record pointers
  hipEvent_t ev_vox_c = nullptr;         // between the parts and the merge
  // the rolling voxel map (ngicp_voxel_roll.h): a map that inserts and evictions maintain instead of a build from the target
  int voxel_roll = 0;                    // ngicp_set_voxel_rolling; remembered while the voxel mode is off
  struct RollMap {
    size_t n_vox = 0, cap = 0, slots = 0;  // voxels, capacity of the per-voxel arrays (doubling), hash table slots (>= 2 * n_vox, a power of two)
    long long inserts = 0;                 // accepted inserts since the last clear: the stamp of the last one
    long long gen = 0;                     // bumped wherever the map is written (insert, evict, clear, restore, move): what a kept result was computed against
    DevBuf sums, rec, vkeys, stamps, table;  // [cap][kVoxRec] {S 3, C 6, n}, [cap][kVoxRec] records, [cap] keys, [cap] stamps, [slots] {key, voxel number}
    double last_insert_ms = 0.0, last_evict_ms = 0.0;  // device event times
  } roll;
  DevBuf roll_q, roll_sums, roll_hit, roll_tmp;  // an insert's transformed points, per-scan-voxel sums and lookup results; an eviction's compaction workspace
  // the record routes: the uploaded arrays of a restore / a record insert, a move's per-voxel stamps
  DevBuf roll_up, roll_seg_stamp;
  hipEvent_t ev_rec_a = nullptr, ev_rec_b = nullptr;  // around a record insert, whose commit is left in the stream:
  bool rec_time_pending = false;                      // its time is read when it is next asked for (roll_resolve_time)
  // clearing along rays (csrc/ngicp_voxel_ray.h): two grow-only pairs of per-voxel counters {miss [n], hit [n]} - a call
  // counts into the pair that does not hold the last accepted call's, so a refused call leaves those readable - and the totals
  // {counted steps, occupied, misses} as three 64-bit integers
  DevBuf roll_ray[2], roll_ray_tot;
  int ray_cur = 0;                       // the pair of the last accepted call
  bool ray_valid = false;                // a call has been accepted ...
  long long ray_gen = 0;                 // ... and left the map at this generation (anything else that writes the map moves it on)
  size_t ray_n = 0;                      // voxels before that call's removal: the length of its counters
  // the gated insert (csrc/ngicp_voxel_gate.h): two grow-only class arrays (one byte per scan point, original order) - a
  // call classifies into the one that does not hold the last accepted call's, so a refused call leaves those readable - and the four
  // class counts behind a flag word of their own
  DevBuf roll_gate_cls[2], roll_gate_cnt;
  int gate_cur = 0;                      // the array of the last accepted call
  bool gate_valid = false;               // a call has been accepted since the last ngicp_voxel_rolling_clear
  size_t gate_n = 0;                     // the points of that call's scan
  // motion deskew (csrc/ngicp_deskew.h): the separately uploaded times, the uploaded trajectory and the table k_deskew_prepare makes of it
  DevBuf dsk_times, dsk_in, dsk_table;
  std::vector<double> dsk_host;          // the trajectory as uploaded: [M times][M x 16 poses][16 T_ref] (outlives the asynchronous copy)
  // voxel fitness (csrc/ngicp_voxel_fitness.h): a query's own workspace, grow-only - nothing of an alignment lives here
  DevBuf vfit_T, vfit_part, vfit_out;    // a chunk's poses [chunk][16], block partials [chunk][blocks][4], sums [chunk][4]
  DevBuf vfit_pts;                       // ngicp_voxel_fitness_points: [n_src] m, [n_src] d, [n_src] v
  hipEvent_t ev_vfit_a = nullptr, ev_vfit_b = nullptr;  // around a chunk's two kernels (its own pair: ngicp_stats is left alone)
  double vfit_kernel_ms = 0.0;           // device time of the last call's kernels, all chunks (ngicp_voxel_fitness_kernel_ms)
  // scan context (csrc/ngicp_scan_context.h): parameters, tables, the descriptor database and a query's own workspace
  struct ScanContext {
    int R = 20, S = 60;                  // rings, sectors
    float L = 80.0f, z0 = 2.0f;          // max_radius, z_offset
    std::vector<float> tab;              // the host tables (sc_make_tables), valid while tab_valid; tab_dev holds them while tab_on_device
    bool tab_valid = false, tab_on_device = false;
    DevBuf tab_dev;
    size_t count = 0, cap = 0;           // entries, capacity of the two arrays in entries (doubling; recounted when a parameter change alters the entry size)
    DevBuf db_desc, db_norm;             // [cap][R][S] floats, [cap][S] column norms
    DevBuf q_desc, q_norm, res;          // a query's descriptor and norms; [n] distances, [n] shifts and the top-k record of the last query
    hipEvent_t ev_a = nullptr, ev_b = nullptr;  // around a call's kernels (created on first use; its own pair: ngicp_stats is left alone)
    double kernel_ms = 0.0;              // ngicp_scan_context_kernel_ms
  } sc;
  // voxel pose search (csrc/ngicp_pose_search.h): a query's own workspace, grow-only
  struct PoseSearch {
    DevBuf T, box, grid, score, cand;    // the base poses [B][16]; the two cell boxes (12 ints); the occupancy bit grid; the score volume [B][|S|]; the top-k levels' keys
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // around the box kernels and around everything behind their read-back (created on first use)
    double kernel_ms = 0.0;              // ngicp_voxel_pose_search_kernel_ms
    bool valid = false;                  // `score` holds the volume of a finished search of `entries` ints ...
    size_t entries = 0;
    bool stamp_rolling = false;          // ... computed against this map: the rolling one at generation stamp_gen, or build number stamp_gen of the target's
    long long stamp_gen = 0;
  } ps;
  // moving keyframes (csrc/ngicp_keyframe_move.h): a call's table on the host (it outlives the asynchronous copy) and on the device
  std::vector<unsigned char> kfm_host;
  DevBuf kfm_table;
  hipEvent_t ev_kfm_a = nullptr, ev_kfm_b = nullptr;  // around the kernel (created on first use; its own pair: ngicp_stats is left alone)
  double kfm_kernel_ms = 0.0;            // ngicp_keyframe_transform_kernel_ms
  // pose graph (csrc/ngicp_pose_graph.h): the graph as given on the host (what the getters return), its device images and the
  // optimiser's workspace, grow-only.  Independent of the clouds; nothing of an alignment lives here
  struct PoseGraph {
    std::vector<double> poses, snapshot;   // [n][16] column-major: the current poses; those at the start of the last optimize
    std::vector<unsigned char> fixed, eflag;  // [n] fixed flags, [m] robust flags
    std::vector<int> ij;                   // [m][2]
    std::vector<double> Z, info;           // [m][16] column-major, [m][36]
    int robust_kind = NGICP_ROBUST_NONE;
    double robust_width = 1.0;
    bool topo_dirty = true, poses_dirty = true;  // the device images of edges / flags / lists, of the poses, are older than the host's
    int cur = 0;                           // which of d_poses holds the current poses
    DevBuf d_ij, d_Z, d_info, d_eflag, d_fixed, d_off, d_ent;  // the graph: edges, flags, the incidence lists
    DevBuf d_lin[2], d_poses[2];           // [m][36] linearised edges of the current / the trial poses; [n][12] poses likewise
    DevBuf d_diag, d_grad, d_minv, d_x, d_r, d_z, d_p, d_q;  // [n][36] / [n][6] per-node arrays of the normal equations and of CG
    DevBuf d_part, d_sc, d_corr;           // block results; the PgScalars record; a corrections call's poses and result
    unsigned char* pin = nullptr;          // pinned: the CG's done word (first 4 bytes), the scalars' read-back image (from byte 64)
    hipEvent_t ev_a = nullptr, ev_b = nullptr;  // around an optimize (created on first use; its own pair: ngicp_stats is left alone)
    double kernel_ms = 0.0;                // ngicp_pose_graph_kernel_ms
  } pg;
};

namespace {

// h's stream waits, on the device, for what `other`'s stream (same device) holds now; the host does not wait
void stream_wait_for(ngicp* h, ngicp* other) {
  HIP_TRY(hipEventRecord(h->ev_fence, other->stream));
  HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_fence, 0));
}

void fence_engine_streams(ngicp* h) {
  HandleRegistry& r = registry();
  std::lock_guard<std::mutex> lock(r.m);
  for (ngicp* o : r.live)
    if (o != h && o->device == h->device) stream_wait_for(h, o);  // (work on h's own stream is ordered before anything h enqueues next)
}

template <class F>
int guarded(ngicp* h, F&& f) {
  if (!h) return NGICP_ERR_ARG;
  try {
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) throw HipError{e, "hipSetDevice", __FILE__, __LINE__};
    f();
    return NGICP_OK;
  } catch (const HipError& e) {
    char buf[512];
    std::snprintf(buf, sizeof(buf), "HIP error %d (%s) in `%s` at %s:%d", (int)e.code, hipGetErrorString(e.code), e.what, e.file, e.line);
    h->err = buf;
    (void)hipGetLastError();
    return NGICP_ERR_HIP;
  } catch (const ArgError& e) {
    h->err = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    h->err = e.what();
    return NGICP_ERR_ARG;
  } catch (...) {
    h->err = "unknown error";
    return NGICP_ERR_ARG;
  }
}

}  // namespace
