// C-ABI implementation (include/ngicp.h) — host driver for the HIP kernels.
// One handle == one nano_gicp::NanoGICP instance (/root/reference/include/nano_gicp/nano_gicp.hpp:58-137).
// Built for gfx950 only:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
#include "../../include/ngicp.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <sched.h>
#include <string>
#include <vector>

#include "ngicp_pass.h"
#include "ngicp_cloudops.h"
#include "ngicp_filters.h"
#include "ngicp_query.h"
#include "ngicp_range.h"
#include "ngicp_batch.h"
#include "ngicp_voxel.h"
#include "ngicp_voxel_batch.h"

using namespace ngk;

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
};

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

struct LoopCtx;  // the per-alignment launch arguments (defined with the registration loop)
constexpr int kMaxPersistPasses = 2048;  // alignments with more possible passes than this take one launch per pass (the ring of views is 512 bytes per pass)
constexpr int kMaxTickPasses = 1024;  // passes of an alignment whose timestamps the persistent kernel records when profiling is on
constexpr int kShardSlots = 4, kShardLag = 2;  // point-sharded stepping: the `done` word of step k is read at step k + kShardLag

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
  hipEvent_t ev_fence = nullptr;                       // fence_engine_streams()
  bool cov_timing_pending = false;
  std::string err;
  Params p;
  double voxel_size = 0.0;  // 0 = auto
  double target_occupancy = 24.0;  // mean points a random point sees in its own cell; tuned on MI355X (c2/c3/c5 workloads)
  int host_wait = 0;        // 0: poll without giving the core up, 1: sched_yield between polls (ngicp_set_host_wait)
  CovSet shard_covs[2];     // covariance sets being computed in blocks by several ranks (ngicp_covs_shard_*), uncommitted
  int chunk_pairs = 3;      // (pass, solve) pairs kept in flight ahead of the solver's published progress (env NGICP_CHUNK)
  int stage_grow = 6;       // upper limit of rings served from the LDS stage
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
  int persist = 0;       // env NGICP_PERSIST=1: ONE launch per alignment (k_gicp_persist).  Exact and complete, but measured no faster than one
                         // launch per pass: off by default
  int order_sel = 0;     // which of the two launch-order buffers (and flag words) the next alignment reads
  DevBuf grp_order_alt;  // the second order buffer: the persistent kernel's solver builds the NEXT alignment's order there
  DevBuf gen_lines;      // the persistent kernel's release word, kGenLines copies (PassArgs::gen)
  int cell_boxes = 0;    // env NGICP_CELL_BOXES=1: per-cell (y,z) extents built with every index and used by the pass (see "Index build")
  int head = 0;          // env NGICP_HEAD=1: k_gicp_head - no solver launch, every block steps the optimiser at its head
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
  std::weak_ptr<DevBuf> submap_covs;     // the covariance set ngicp_submap_set installed with it (weak: a recycled buffer is another object)

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
};

namespace {

void fence_engine_streams(ngicp* h) {
  HandleRegistry& r = registry();
  std::lock_guard<std::mutex> lock(r.m);
  for (ngicp* o : r.live) {
    if (o == h || o->device != h->device) continue;  // (work on h's own stream is ordered before anything h enqueues next)
    HIP_TRY(hipEventRecord(h->ev_fence, o->stream));
    HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_fence, 0));
  }
}

int pick_blocks(size_t work_items, int per_block, int max_blocks) {
  size_t b = (work_items + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > (size_t)max_blocks) b = max_blocks;
  return (int)b;
}

// ------------------------------------------------------------------------------------------
// Index build
// ------------------------------------------------------------------------------------------
// NGICP_CELL_BOXES=1 (experiment, round 3): per-cell (y,z) extents of the points, built with every index; the pass cuts and prunes its
// ring-1 (query, row) pairs with them.  Exact, a quarter fewer candidates (c3 68.4 -> 52.2 per query, c5 25.9 -> 23.8), 25 % fewer
// ring-1 units per wave - and the launch exactly as long as before (c3 33.7 us either way, c5 41.3 -> 42.5: the second load per row):
// the units it removes were served in parallel by lanes that would otherwise idle.  Off by default.
// (read at ngicp_create: ngicp::cell_boxes; an index carries boxes when the handle that built it had the switch on)

Grid make_grid(const float mn[3], const float mx[3], double h, int max_cells) {
  Grid g{};
  double ext[3];
  for (int d = 0; d < 3; ++d) ext[d] = std::max(0.0, (double)mx[d] - (double)mn[d]);
  for (;;) {
    double nx = std::floor(ext[0] / h) + 1, ny = std::floor(ext[1] / h) + 1, nz = std::floor(ext[2] / h) + 1;
    // (the pass kernel packs a listed row as y | z << 16 in one int: y < 65536, z < 32768)
    if (nx * ny * nz <= (double)max_cells && ny < 65536.0 && nz < 32768.0) {
      g.nx = (int)nx;
      g.ny = (int)ny;
      g.nz = (int)nz;
      break;
    }
    h *= 1.26;
  }
  g.ox = mn[0];
  g.oy = mn[1];
  g.oz = mn[2];
  g.h = (float)h;
  g.inv_h = 1.0f / g.h;
  g.ncells = g.nx * g.ny * g.nz;
  double span = std::max(ext[0], std::max(ext[1], ext[2]));
  g.slack = (float)(1e-3 * h + 4e-6 * (span + std::fabs(mn[0]) + std::fabs(mn[1]) + std::fabs(mn[2])));
  return g;
}

// occ_host: where to put sum(count^2) (synchronous read-back), or null.  occ_device_only: compute it into h->occ but leave it
// on the device (the caller reads it later, when it synchronises anyway).
// stride > 1: an occupancy ESTIMATE from every stride-th point (the cell-start table written is then meaningless)
void count_and_scan(ngicp* h, DeviceCloud& dc, int n, unsigned long long* occ_host, bool occ_device_only = false, int stride = 1) {
  const Grid& g = dc.grid;
  h->counts.ensure((size_t)(g.ncells + 1) * sizeof(int));
  HIP_TRY(hipMemsetAsync(h->counts.p, 0, (size_t)(g.ncells + 1) * sizeof(int), h->stream));
  hipLaunchKernelGGL(k_cell_count, dim3(pick_blocks((size_t)(n / stride + 1), 256, 2048)), dim3(256), 0, h->stream, h->unsorted.as<float4>(), n, g, h->keys.as<int>(), h->counts.as<int>(),
                     h->fill.as<int>(), stride);
  const int ntiles = (g.ncells + kScanTile - 1) / kScanTile;
  h->tile_sums.ensure((size_t)ntiles * sizeof(int));
  h->tile_sq.ensure((size_t)ntiles * sizeof(unsigned long long));
  dc.cell_start.ensure((size_t)(g.ncells + 1 + 2 * kCellPad) * sizeof(int));
  HIP_TRY(hipMemsetAsync(dc.cell_start.p, 0, kCellPad * sizeof(int), h->stream));  // front pad (k_scan_apply writes the back pad)
  unsigned long long* tsq = (occ_host || occ_device_only) ? h->tile_sq.as<unsigned long long>() : nullptr;
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(kScanBlock), 0, h->stream, h->counts.as<int>(), g.ncells, h->tile_sums.as<int>(), tsq);
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(kScanBlock), 0, h->stream, h->tile_sums.as<int>(), ntiles, (const unsigned long long*)tsq,
                     h->occ.as<unsigned long long>());
  hipLaunchKernelGGL(k_scan_apply, dim3(ntiles), dim3(kScanBlock), 0, h->stream, h->counts.as<int>(), g.ncells, h->tile_sums.as<int>(), dc.cells());
  if (occ_host) {
    HIP_TRY(hipMemcpyAsync(occ_host, h->occ.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
}

// Host cloud -> h->unsorted (float4 {x, y, z, bitcast(original index)}) + its bounding box.  The only host read-back of the build
// (the grid dimensions size the allocations).
void stage_host_cloud(ngicp* h, const float* xyz, size_t n, size_t stride, float mn[3], float mx[3]) {
  if (n == 0) throw ArgError{NGICP_ERR_ARG, "empty cloud"};
  if (n > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "cloud too large for int indices"};
  if (stride < 12 || (stride % 4) != 0) throw ArgError{NGICP_ERR_ARG, "stride_bytes must be a multiple of 4 and >= 12"};
  const int ni = (int)n;
  const double t0 = now_ms();
  const size_t raw_bytes = (n - 1) * stride + 12;
  h->raw.ensure(raw_bytes);
  HIP_TRY(hipMemcpyAsync(h->raw.p, xyz, raw_bytes, hipMemcpyHostToDevice, h->stream));
  h->unsorted.ensure(n * sizeof(float4));
  const int bbox_blocks = pick_blocks(n, 1024, 512);
  h->bbox.ensure((size_t)bbox_blocks * 8 * sizeof(float));
  hipLaunchKernelGGL(k_unpack_bbox, dim3(bbox_blocks), dim3(256), 0, h->stream, h->raw.as<unsigned char>(), stride, ni, h->unsorted.as<float4>(), h->bbox.as<float>());
  std::vector<float> bb((size_t)bbox_blocks * 8);
  HIP_TRY(hipMemcpyAsync(bb.data(), h->bbox.p, bb.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->stats.upload_ms = now_ms() - t0;  // copy + unpack + bounding box (one synchronisation)
  for (int d = 0; d < 3; ++d) mn[d] = 3.0e38f, mx[d] = -3.0e38f;
  float bad = 0.f;
  for (int b = 0; b < bbox_blocks; ++b) {
    for (int d = 0; d < 3; ++d) {
      mn[d] = std::min(mn[d], bb[(size_t)b * 8 + d]);
      mx[d] = std::max(mx[d], bb[(size_t)b * 8 + 3 + d]);
    }
    bad += bb[(size_t)b * 8 + 6];
  }
  // the reference assumes NaNs were removed upstream (src/dlo/odom.cc:443-447); make it an explicit error
  if (bad > 0.f) throw ArgError{NGICP_ERR_ARG, "cloud contains non-finite coordinates"};
  for (int d = 0; d < 3; ++d)
    if (!std::isfinite(mn[d]) || !std::isfinite(mx[d]) || mn[d] > mx[d]) throw ArgError{NGICP_ERR_ARG, "cloud contains non-finite coordinates"};
}

// h->unsorted[0..n) -> an indexed DeviceCloud.  Everything stays on the device; one synchronisation at the end.
std::shared_ptr<DeviceCloud> index_unsorted(ngicp* h, size_t n, const float mn[3], const float mx[3]) {
  auto dc = acquire_cloud(h, h->device);
  dc->n = n;
  for (int d = 0; d < 3; ++d) dc->bb_min[d] = mn[d], dc->bb_max[d] = mx[d];
  const int ni = (int)n;
  HIP_TRY(hipEventRecord(h->ev_a, h->stream));
  h->keys.ensure(n * sizeof(int));
  h->tmp.ensure(n * sizeof(float4));
  h->occ.ensure(2 * sizeof(unsigned long long));
  const int max_cells = 1 << 25;
  double hh;
  const bool auto_h = !(h->voxel_size > 0.0);
  bool memo_hit = false;
  if (!auto_h) {
    hh = h->voxel_size;
  } else {
    double vol = 1.0;
    for (int d = 0; d < 3; ++d) vol *= std::max(0.05, (double)mx[d] - (double)mn[d]);
    hh = std::cbrt(vol / (double)n) * 1.5;  // first guess; refined from measured occupancy below
    hh = std::max(hh, 0.02);
    // consecutive scans / submaps look alike: start from the voxel the last cloud of similar size ended with
    // (saves the refinement passes, each a histogram + scan + host read-back)
    for (const auto& e : h->voxel_memo)
      if (e.second > 0.0 && (double)n > 0.5 * (double)e.first && (double)n < 2.0 * (double)e.first) {
        hh = e.second;
        memo_hit = true;
      }
  }
  dc->grid = make_grid(mn, mx, hh, max_cells);
  unsigned long long occ = 0;
  h->fill.ensure(n * sizeof(int));  // (arrival rank of every point inside its cell: k_cell_count -> k_cell_scatter)
  // with a memoised voxel the occupancy is only checked AFTER the build (it corrects the memo for the next cloud): the
  // read-back then rides on the build's final synchronisation instead of stalling the pipeline here
  count_and_scan(h, *dc, ni, (auto_h && !memo_hit) ? &occ : nullptr, auto_h && memo_hit);
  if (auto_h && !memo_hit) {
    // the first cloud of a size class: refine the voxel edge until the mean occupancy seen by a random point (sum c^2 / n) is near
    // the target.  (Round 3 tried estimating it from every 8th / 32nd point: consecutive points of a LiDAR ring share their cells, a
    // strided sample is not a thinned copy of the cloud, and the estimate settled on cells 2.4x too small - measured, withdrawn.)
    for (int it = 0; it < 4; ++it) {
      const double lam = (double)occ / (double)n;
      const double ratio = h->target_occupancy / std::max(lam, 1.0);
      if (ratio > 0.75 && ratio < 1.33) break;
      double scale = std::pow(ratio, 1.0 / 1.5);
      scale = std::min(4.0, std::max(0.25, scale));
      hh = std::max(0.01, (double)dc->grid.h * scale);
      dc->grid = make_grid(mn, mx, hh, max_cells);
      count_and_scan(h, *dc, ni, &occ);
    }
  }
  const Grid& g = dc->grid;
  dc->sorted.ensure((n + 2 * kSortedPad) * sizeof(float4));
  hipLaunchKernelGGL(k_fill_sentinels, dim3(1), dim3(2 * kSortedPad), 0, h->stream, dc->sorted.as<float4>(), ni);
  dc->perm.ensure(n * sizeof(int));
  hipLaunchKernelGGL(k_cell_scatter, dim3(pick_blocks(n, 256, 2048)), dim3(256), 0, h->stream, h->unsorted.as<float4>(), h->keys.as<int>(), h->fill.as<int>(), ni, dc->cells(),
                     h->tmp.as<float4>());
  hipLaunchKernelGGL(k_cell_rank, dim3(pick_blocks(n, 256, 4096)), dim3(256), 0, h->stream, h->tmp.as<float4>(), ni, g, dc->cells(), dc->pts(),
                     dc->perm.as<int>());
  dc->has_boxes = h->cell_boxes != 0;
  if (dc->has_boxes) {
  dc->cell_box.ensure((size_t)(g.ncells + 2 * kCellPad) * sizeof(unsigned int));
  hipLaunchKernelGGL(k_fill_u32, dim3(1), dim3(2 * kCellPad), 0, h->stream, dc->cell_box.as<unsigned int>(), dc->cell_box.as<unsigned int>() + kCellPad + g.ncells, kCellPad, kCellBoxEmpty);
  hipLaunchKernelGGL(k_cell_boxes, dim3((unsigned)((g.ncells + 255) / 256)), dim3(256), 0, h->stream, dc->pts(), dc->cells(), g, dc->cell_box.as<unsigned int>() + kCellPad);
  }
  dc->sorted3.ensure((n + 2 * kSortedPad) * sizeof(Xyz));
  hipLaunchKernelGGL(k_pack_xyz, dim3((unsigned)((n + 2 * kSortedPad + 255) / 256)), dim3(256), 0, h->stream, dc->sorted.as<float4>(), ni + 2 * kSortedPad, dc->sorted3.as<Xyz>());
  dc->sortedp.ensure((n + 2 * kSortedPad) * sizeof(float4));
  hipLaunchKernelGGL(k_pack_pos, dim3((unsigned)((n + 2 * kSortedPad + 255) / 256)), dim3(256), 0, h->stream, dc->sorted.as<float4>(), ni + 2 * kSortedPad, kSortedPad, dc->sortedp.as<float4>());
  {
    // query order (Morton over tiles of 2^shift cells; <= 128 tiles per axis => <= 2M histogram bins)
    int shift = 2;
    while (((std::max(g.nx, std::max(g.ny, g.nz)) - 1) >> shift) >= 128) ++shift;
    int bits = 1;
    while ((1 << bits) <= ((std::max(g.nx, std::max(g.ny, g.nz)) - 1) >> shift)) ++bits;
    const int nbins = 1 << (3 * bits);
    h->counts.ensure((size_t)(nbins + 1) * sizeof(int));
    h->fill.ensure((size_t)(nbins + 1 + kCellPad) * sizeof(int));  // reused as tile_start (k_scan_apply pads its output)
    HIP_TRY(hipMemsetAsync(h->counts.p, 0, (size_t)(nbins + 1) * sizeof(int), h->stream));
    hipLaunchKernelGGL(k_tile_count, dim3(pick_blocks(n, 256, 2048)), dim3(256), 0, h->stream, dc->pts(), ni, g, shift, h->counts.as<int>());
    // where every tile's queries start and where its batches start: one scan of packed {count, ceil(count / 32)} pairs
    const int ntiles = (nbins + kScanTile - 1) / kScanTile;
    h->tile_sums.ensure((size_t)ntiles * sizeof(unsigned long long));
    h->tmp.ensure(std::max(n * sizeof(float4), (size_t)(nbins + 1 + kCellPad) * sizeof(int)));  // (k_cell_rank is done with it) batches before every tile
    dc->n_batches_dev.ensure(sizeof(int));
    hipLaunchKernelGGL(k_scan2_tiles, dim3(ntiles), dim3(kScanBlock), 0, h->stream, h->counts.as<int>(), nbins, h->tile_sums.as<unsigned long long>());
    hipLaunchKernelGGL(k_scan2_tile_sums, dim3(1), dim3(kScanBlock), 0, h->stream, h->tile_sums.as<unsigned long long>(), ntiles);
    hipLaunchKernelGGL(k_scan2_apply, dim3(ntiles), dim3(kScanBlock), 0, h->stream, h->counts.as<int>(), nbins, h->tile_sums.as<unsigned long long>(), h->fill.as<int>(),
                       h->tmp.as<int>(), dc->n_batches_dev.as<int>());
    dc->qpts.ensure(n * sizeof(float4));
    hipLaunchKernelGGL(k_tile_place, dim3(pick_blocks(n, 256, 4096)), dim3(256), 0, h->stream, dc->pts(), ni, g, shift, dc->cells(),
                       h->fill.as<int>(), dc->qpts.as<float4>());
    // tile-aligned query batches
    dc->batches.ensure((n + 1) * sizeof(int2));
    hipLaunchKernelGGL(k_batch_fill, dim3((nbins + 255) / 256), dim3(256), 0, h->stream, h->counts.as<int>(), h->fill.as<int>(), h->tmp.as<int>(), nbins,
                       dc->batches.as<int2>());
    dc->batch_boxes.ensure((n + 1) * 6 * sizeof(float));
    hipLaunchKernelGGL(k_batch_boxes, dim3((unsigned)std::min<size_t>((n + 3) / 4, 4096)), dim3(256), 0, h->stream, dc->qpts.as<float4>(), dc->batches.as<int2>(), dc->n_batches_dev.as<int>(),
                       dc->batch_boxes.as<float>());  // (a wave per batch, grid-strided)
    HIP_TRY(hipMemcpyAsync(&dc->n_batches, dc->n_batches_dev.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  }
  // with a memoised voxel the occupancy read-back rides on the build's final synchronisation (it steers the memo for the
  // next cloud of this size class, not this build)
  if (auto_h && memo_hit) HIP_TRY(hipMemcpyAsync(&occ, h->occ.p, sizeof(occ), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipEventRecord(h->ev_b, h->stream));
  HIP_TRY(hipEventSynchronize(h->ev_b));
  if (auto_h) {  // remember the voxel for the next cloud of this size class (two entries: scan-sized and submap-sized)
    double next_h = (double)dc->grid.h;
    if (memo_hit) {
      HIP_TRY(hipStreamSynchronize(h->stream));
      const double lam = (double)occ / (double)n, ratio = h->target_occupancy / std::max(lam, 1.0);
      if (!(ratio > 0.75 && ratio < 1.33)) next_h = std::max(0.01, next_h * std::min(4.0, std::max(0.25, std::pow(ratio, 1.0 / 1.5))));
    }
    int slot = -1;
    for (int i = 0; i < 4; ++i)  // the entry of this size class, else an empty one, else the oldest
      if (h->voxel_memo[i].second > 0.0 && (double)n > 0.5 * (double)h->voxel_memo[i].first && (double)n < 2.0 * (double)h->voxel_memo[i].first) slot = i;
    if (slot < 0)
      for (int i = 0; i < 4 && slot < 0; ++i)
        if (!(h->voxel_memo[i].second > 0.0)) slot = i;
    if (slot < 0) {
      slot = h->voxel_memo_next;
      h->voxel_memo_next = (h->voxel_memo_next + 1) % 4;
    }
    h->voxel_memo[slot] = {n, next_h};
  }
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->ev_a, h->ev_b));
  dc->build_ms = ms;
  h->stats.index_build_ms = ms;
  HIP_TRY(hipGetLastError());
  return dc;
}

std::shared_ptr<DeviceCloud> upload_and_index(ngicp* h, const float* xyz, size_t n, size_t stride) {
  float mn[3], mx[3];
  stage_host_cloud(h, xyz, n, stride, mn, mx);
  return index_unsorted(h, n, mn, mx);
}

void ensure_inv_perm(ngicp* h, DeviceCloud& dc) {
  if (dc.has_inv) return;
  dc.inv_perm.ensure(dc.n * sizeof(int));
  hipLaunchKernelGGL(k_invert_perm, dim3((unsigned)((dc.n + 255) / 256)), dim3(256), 0, h->stream, dc.perm.as<int>(), (int)dc.n, dc.inv_perm.as<int>());
  dc.has_inv = true;
}

void ensure_slot_ready(ngicp* h, Slot& s, const char* what) {
  if (!s.present) throw ArgError{NGICP_ERR_STATE, std::string("no ") + what + " cloud set"};
  if (s.dev) return;
  if (!s.host) throw ArgError{NGICP_ERR_STATE, std::string(what) + " cloud has no data"};
  s.dev = upload_and_index(h, s.host, s.n, s.stride);
}

// ------------------------------------------------------------------------------------------
// Covariances
// ------------------------------------------------------------------------------------------
template <int K>
void launch_cov(ngicp* h, DeviceCloud& dc, int k, int reg, double* out, size_t lo, size_t hi, hipStream_t s) {
  if (hi <= lo) return;
  const dim3 grid((unsigned)((hi - lo + kKnnPairs - 1) / kKnnPairs)), block(kKnnBlock);
  // window size by cloud size (see knn_take_window): a scan that does not fill the chip is as slow as one wave's chain of round
  // trips - wider windows; a large cloud is bound by what its waves fetch and insert - narrow ones
  if (dc.n < 160000)
    hipLaunchKernelGGL((k_covariances<K, 6>), grid, block, 0, s, dc.pts(), dc.cells(), dc.grid, (int)lo, (int)hi, k, reg, out);
  else
    hipLaunchKernelGGL((k_covariances<K, 4>), grid, block, 0, s, dc.pts(), dc.cells(), dc.grid, (int)lo, (int)hi, k, reg, out);
}

// covariances of the points at sorted positions [lo, hi) into `out` ([n][6], sorted order)
void launch_cov_range(ngicp* h, DeviceCloud& dc, double* out, size_t lo, size_t hi, hipStream_t s) {
  const int k = h->p.k, reg = h->p.regularization;
  if (k <= 0) throw ArgError{NGICP_ERR_ARG, "k must be positive"};
  if (k > 32 || (size_t)k > dc.n) throw ArgError{NGICP_ERR_K_TOO_LARGE, "k exceeds the cloud size or the engine limit of 32"};
  if (k <= 10)
    launch_cov<10>(h, dc, k, reg, out, lo, hi, s);
  else if (k <= 20)
    launch_cov<20>(h, dc, k, reg, out, lo, hi, s);
  else
    launch_cov<32>(h, dc, k, reg, out, lo, hi, s);
}

void compute_covs(ngicp* h, Slot& slot, CovSet& cs, const char* what) {
  ensure_slot_ready(h, slot, what);
  DeviceCloud& dc = *slot.dev;
  const int k = h->p.k;
  if (k <= 0) throw ArgError{NGICP_ERR_ARG, "k must be positive"};
  if (k > 32 || (size_t)k > dc.n) throw ArgError{NGICP_ERR_K_TOO_LARGE, "k exceeds the cloud size or the engine limit of 32"};
  auto buf = acquire_buf(h, h->device, dc.n * 6 * sizeof(double));
  HIP_TRY(hipEventRecord(h->ev_cov_a, h->stream));
  launch_cov_range(h, dc, buf->as<double>(), 0, dc.n, h->stream);
  HIP_TRY(hipEventRecord(h->ev_cov_b, h->stream));
  HIP_TRY(hipGetLastError());
  h->cov_timing_pending = true;  // no synchronisation here: the covariances are consumed on this same stream
  cs.data = buf;
  cs.n = dc.n;
  cs.order = slot.dev;
}

// make `cs` usable with cloud `dc` (same n): returns device pointer to [n][6] in dc's sorted order
const double* covs_for(ngicp* h, CovSet& cs, const std::shared_ptr<DeviceCloud>& dc) {
  if (cs.order.get() == dc.get()) return cs.data->as<double>();
  // covariances are logically indexed by ORIGINAL point index (the reference's vector index):
  // re-order from the donor cloud's sorted order to this cloud's sorted order
  ensure_inv_perm(h, *cs.order);
  auto buf = acquire_buf(h, h->device, dc->n * 6 * sizeof(double));
  hipLaunchKernelGGL(k_covs_reorder, dim3((unsigned)((dc->n + 255) / 256)), dim3(256), 0, h->stream, cs.data->as<double>(), cs.order->inv_perm.as<int>(), dc->perm.as<int>(),
                     (int)dc->n, buf->as<double>());
  cs.data = buf;
  cs.order = dc;
  return cs.data->as<double>();
}

void get_covs(ngicp* h, CovSet& cs, double* out) {
  if (cs.n == 0) return;
  h->scratch16.ensure(cs.n * 16 * sizeof(double));
  hipLaunchKernelGGL(k_covs_expand, dim3((unsigned)((cs.n + 255) / 256)), dim3(256), 0, h->stream, cs.data->as<double>(), cs.order->perm.as<int>(), (int)cs.n,
                     h->scratch16.as<double>());
  HIP_TRY(hipMemcpyAsync(out, h->scratch16.p, cs.n * 16 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
}

void set_covs(ngicp* h, Slot& slot, CovSet& cs, const double* in, size_t n, const char* what) {
  if (n == 0) {
    cs.clear();
    return;
  }
  // The reference accepts any vector; sizes are reconciled at align() (impl/nano_gicp_impl.hpp:163-168).
  // The packed image needs an ordering cloud: require the slot's cloud with the same size.
  if (!slot.present || slot.n != n) throw ArgError{NGICP_ERR_STATE, std::string("set covariances: ") + what + " cloud missing or of different size"};
  ensure_slot_ready(h, slot, what);
  h->scratch16.ensure(n * 16 * sizeof(double));
  HIP_TRY(hipMemcpyAsync(h->scratch16.p, in, n * 16 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  auto buf = acquire_buf(h, h->device, n * 6 * sizeof(double));
  hipLaunchKernelGGL(k_covs_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->scratch16.as<double>(), slot.dev->perm.as<int>(), (int)n, buf->as<double>());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  cs.data = buf;
  cs.n = n;
  cs.order = slot.dev;
}

// ------------------------------------------------------------------------------------------
// Registration loop
// ------------------------------------------------------------------------------------------
// start / stop: events attached to the dispatch itself (they take the kernel's own begin / end timestamps: no extra packets in
// the stream, unlike hipEventRecord before and after), or null
std::mutex& persist_mutex(int device) {  // one persistent alignment per device at a time (its grid fills the device and its blocks wait for each other)
  static std::mutex m[64];
  return m[(unsigned)device % 64u];
}

int pass_impl() {
  static const int impl = std::getenv("NGICP_PASS_IMPL") ? std::atoi(std::getenv("NGICP_PASS_IMPL")) : 0;
  return impl;
}

void launch_pass(ngicp* h, const PassArgs& a, int nblocks, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr) {
  // 32-query batches, 2 lanes per query.  Two builds of the kernel: 3 waves per SIMD (129 VGPRs), and 4 (128 VGPRs, two spilled
  // dwords, 4 blocks per CU) for grids of more than two rounds of blocks, where the launch is bound by how many blocks pass through
  // the chip rather than by its slowest block.
  static const int force = std::getenv("NGICP_PASS_WPS") ? std::atoi(std::getenv("NGICP_PASS_WPS")) : 0;  // (A/B timing only)
  const int impl = pass_impl();  // 0: walks in global memory (default), 1: the staged search of ngicp_pass_st.h (round 3 experiment: exact, slower - DESIGN.md §5)
  const bool four = force ? force == 4 : nblocks > 2 * h->pass_slots;
  if (impl == 1) {
    PassArgs b = a;
    b.fused = 0;
    // cells that cover the distance gate around a query's own cell (its reach box is clamped there; beyond it the shell walk takes over)
    int need = kStGrowMax;
    if (h->p.max_corr_dist < 1e30) need = (int)std::ceil(h->p.max_corr_dist / (double)a.grid.h);
    b.stage_grow = std::max(1, std::min(kStGrowMax, need));
    if (force ? force == 4 : true)  // (128 VGPRs either way; the 4-wave build's smaller tables leave room for a fourth block per CU)
      hipExtLaunchKernelGGL((k_gicp_pass_st<4>), dim3(nblocks), dim3(256), 0, s, start, stop, 0, b);
    else
      hipExtLaunchKernelGGL((k_gicp_pass_st<3>), dim3(nblocks), dim3(256), 0, s, start, stop, 0, b);
    return;
  }
  // NGICP_QUEUE=1 (experiment, round 3): a grid of resident blocks that draw their groups from a counter (k_gicp_queue)
  static const int queue_env = std::getenv("NGICP_QUEUE") ? std::atoi(std::getenv("NGICP_QUEUE")) : 0;
  if (queue_env && !a.fused && !(a.mode & 4) && !a.dbg_stamps && !a.dbg_span && !a.dbg_qstats) {
    if (four)
      hipExtLaunchKernelGGL((k_gicp_queue<2, 4>), dim3((unsigned)std::min(nblocks, h->queue_slots[1])), dim3(256), 0, s, start, stop, 0, a);
    else
      hipExtLaunchKernelGGL((k_gicp_queue<2, 3>), dim3((unsigned)std::min(nblocks, h->queue_slots[0])), dim3(256), 0, s, start, stop, 0, a);
    return;
  }
  if (a.fused) {  // (the solver in the tail of the launch: a build of its own)
    if (four)
      hipExtLaunchKernelGGL((k_gicp_pass<2, 4, true>), dim3(nblocks), dim3(256), 0, s, start, stop, 0, a);
    else
      hipExtLaunchKernelGGL((k_gicp_pass<2, 3, true>), dim3(nblocks), dim3(256), 0, s, start, stop, 0, a);
    return;
  }
  if (four)
    hipExtLaunchKernelGGL((k_gicp_pass<2, 4>), dim3(nblocks), dim3(256), 0, s, start, stop, 0, a);
  else
    hipExtLaunchKernelGGL((k_gicp_pass<2, 3>), dim3(nblocks), dim3(256), 0, s, start, stop, 0, a);
}

struct LoopCtx {
  PassArgs pa;
  SolveArgs sa;
  int nblocks;
};

// own_buffers false (ngicp_align_batch): slots and covariances are readied and the fields every lane shares are filled in, but none of
// the handle's single-alignment buffers is sized or referred to (the caller supplies every per-alignment pointer) and no stats field is
// written: what the getters of the last ngicp_align read stays where it is.
void prepare_loop(ngicp* h, LoopCtx& c, bool own_buffers = true) {
  ensure_slot_ready(h, h->src, "source");
  ensure_slot_ready(h, h->tgt, "target");
  // lazy covariances (impl/nano_gicp_impl.hpp:163-168)
  if (h->src_covs.n != h->src.dev->n) compute_covs(h, h->src, h->src_covs, "source");
  if (h->tgt_covs.n != h->tgt.dev->n) compute_covs(h, h->tgt, h->tgt_covs, "target");
  DeviceCloud& S = *h->src.dev;
  DeviceCloud& T = *h->tgt.dev;
  const size_t n = S.n;
  const int nblocks = std::max(1, (S.n_batches + 3) / 4);  // one block per group of four batches
  const int max_rows = std::max(1, h->p.max_iter) * std::max(1, h->p.lm_max_iter) + 1;
  if (own_buffers) {
    for (int i = 0; i < 2; ++i) {
      h->tpt[i].ensure(n * sizeof(float4));
      h->mahal[i].ensure(n * 6 * sizeof(double));
    }
    h->partials.ensure((size_t)kNumSlots * nblocks * sizeof(double));
    h->grp_order.ensure((size_t)nblocks * sizeof(int));
    h->grp_order_alt.ensure((size_t)nblocks * sizeof(int));
    h->grp_cost.ensure((size_t)nblocks * sizeof(int));
    {
      // (the persistent kernel's ring of per-pass views continues behind the state: one 256-byte entry per possible pass)
      const long ring = (long)std::max(1, h->p.max_iter) * std::max(1, h->p.lm_max_iter) + 2;
      h->state.ensure(sizeof(LmState) + (ring <= kMaxPersistPasses ? (size_t)ring * kViewWords * sizeof(int) : 0));
    }
    if (h->trace.ensure_grew((size_t)max_rows * kTraceCols * sizeof(double))) h->trace_rows_dev = 0;  // an unfetched trace went with the old buffer
    h->sums.ensure(kPartialStride * sizeof(double));
    h->batch_far.ensure((size_t)S.n_batches + 16);
    h->gen_lines.ensure((size_t)kGenLines * kGenStride * sizeof(int));
  }

  PassArgs& a = c.pa;
  a.qpts = S.qpts.as<float4>();
  a.batches = S.batches.as<int2>();
  a.batch_boxes = S.batch_boxes.as<float>();
  int* const order_buf[2] = {own_buffers ? h->grp_order.as<int>() : nullptr, own_buffers ? h->grp_order_alt.as<int>() : nullptr};
  int* const ctl = own_buffers ? h->order_flag.as<int>() : nullptr;  // {order flag 0, ticket, gen, order flag 1}
  int* const order_flag[2] = {ctl, ctl ? ctl + 3 : nullptr};
  a.grp_order = order_buf[h->order_sel];
  a.grp_cost = own_buffers ? h->grp_cost.as<int>() : nullptr;
  a.n_batches = S.n_batches;
  a.cov_src = covs_for(h, h->src_covs, h->src.dev);
  a.n_src = (int)n;
  a.tgt = T.pts();
  a.tgt3 = T.xyz3();
  a.tgtp = T.xyzp();
  a.tgt_cell_start = T.cells();
  a.tgt_cell_box = (h->cell_boxes && T.has_boxes) ? T.cell_box.as<unsigned int>() + kCellPad : nullptr;
  a.cov_tgt = covs_for(h, h->tgt_covs, h->tgt.dev);
  a.grid = T.grid;
  for (int i = 0; i < 2; ++i) {
    a.tpt[i] = own_buffers ? h->tpt[i].as<float4>() : nullptr;
    a.mahal[i] = own_buffers ? h->mahal[i].as<double>() : nullptr;
  }
  a.gate_sq = h->p.max_corr_dist * h->p.max_corr_dist;
  {
    float f = (float)a.gate_sq;  // may round down or overflow to inf
    if ((double)f < a.gate_sq) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    a.gate_sq_f = f;
  }
  a.batch_far = own_buffers ? h->batch_far.as<unsigned char>() : nullptr;
  a.st = own_buffers ? h->state.as<LmState>() : nullptr;
  a.partials = own_buffers ? h->partials.as<double>() : nullptr;
  a.mode = 3;
  a.dbg_stamps = nullptr;
  a.dbg_qstats = nullptr;
  a.dbg_span = nullptr;
  a.order_valid = order_flag[h->order_sel];
  a.t_first = nullptr;
  a.fused = 0;
  a.persist = 0;
  a.first_pass = 0;
  a.max_passes = 0;
  a.ticket = ctl ? ctl + 1 : nullptr;
  a.gen = own_buffers ? h->gen_lines.as<int>() : nullptr;
  {
    // rings worth staging: enough to cover the distance gate (the search never looks farther), at most kStageMaxGrow
    int need = kStageMaxGrow;
    if (h->p.max_corr_dist < 1e30) need = (int)std::ceil(h->p.max_corr_dist / (double)T.grid.h);
    a.stage_grow = h->stage_grow <= 0 ? 0 : std::max(1, std::min(std::min(kStageMaxGrow, h->stage_grow), need));  // 0: search straight from global memory
  }

  SolveArgs& s = c.sa;
  s.st = a.st;
  s.cfg.max_iterations = h->p.max_iter;
  s.cfg.lm_max_iterations = h->p.lm_max_iter;
  s.cfg.optimizer = h->p.optimizer;
  s.cfg.rot_eps = h->p.rot_eps;
  s.cfg.trans_eps = h->p.trans_eps;
  s.cfg.lm_init_lambda_factor = h->p.lm_init_lambda_factor;
  s.partials = a.partials;
  s.nblocks = nblocks;
  s.grp_order = order_buf[h->order_sel];
  s.grp_cost = a.grp_cost;
  s.trace = own_buffers ? h->trace.as<double>() : nullptr;
  s.max_trace_rows = max_rows;
  s.mode = 0;
  s.sums_out = nullptr;
  s.dbg_stamps = nullptr;
  s.progress_host = nullptr;
  s.final_host = nullptr;
  s.order_valid = order_flag[h->order_sel];
  s.t_first = nullptr;
  s.persist = 0;
  s.pass_ticks = nullptr;
  s.st_out = nullptr;
  s.nrows = 0;
  a.crow_in = nullptr;
  a.crow_out = nullptr;
  a.cluster_ticket = nullptr;
  a.done_flag = nullptr;
  c.nblocks = nblocks;
  if (!own_buffers) return;
  h->stats.lanes_per_query = 2;
  h->stats.voxel_size = T.grid.h;
  h->stats.grid_dims[0] = T.grid.nx;
  h->stats.grid_dims[1] = T.grid.ny;
  h->stats.grid_dims[2] = T.grid.nz;
}

void init_state_from_pose(LmState& st, const Pose& x0) {
  std::memset(&st, 0, sizeof(st));
  st.hot.x0 = x0;
  st.hot.xi = x0;
  pose_identity(st.hot.delta);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) st.xi_f[r * 4 + c] = (float)x0.R[r * 3 + c];
    st.xi_f[r * 4 + 3] = (float)x0.t[r];
  }
  std::memcpy(&st.view[kViewXi], &st.hot.xi, sizeof(Pose));
  std::memcpy(&st.view[kViewXiF], st.xi_f, sizeof(st.xi_f));
  static_assert(sizeof(Pose) == 24 * sizeof(int) && kViewXiF == 24 && sizeof(LmState::xi_f) == 12 * sizeof(int), "LmState::view layout");
  st.hot.lambda = -1.0;  // impl/lsq_registration_impl.hpp:92
  st.hot.nu = 2.0;
  for (int i = 0; i < 6; ++i) st.hot.final_H[i * 6 + i] = 1.0;
}

Pose pose_from_colmajor_f(const float m[16]) {  // Isometry3d(guess.cast<double>()), impl/lsq_registration_impl.hpp:90
  Pose p;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) p.R[r * 3 + c] = (double)m[c * 4 + r];
    p.t[r] = (double)m[12 + r];
  }
  return p;
}
Pose pose_from_colmajor_d(const double m[16]) {
  Pose p;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) p.R[r * 3 + c] = m[c * 4 + r];
    p.t[r] = m[12 + r];
  }
  return p;
}
void pose_to_colmajor_f(const Pose& p, float m[16]) {  // x0.cast<float>().matrix(), :113
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) m[c * 4 + r] = (float)p.R[r * 3 + c];
    m[12 + r] = (float)p.t[r];
    m[r * 4 + 3] = 0.f;
  }
  m[15] = 1.f;
}

// h->out_xyz (packed xyz on the device) -> host xyz at a byte stride
void download_xyz(ngicp* h, size_t n, float* out, size_t out_stride) {
  if (out_stride == 12) {
    HIP_TRY(hipMemcpyAsync(out, h->out_xyz.p, n * 12, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  } else {
    std::vector<float> tmp(n * 3);
    HIP_TRY(hipMemcpyAsync(tmp.data(), h->out_xyz.p, n * 12, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; ++i) {
      float* o = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(out) + i * out_stride);
      o[0] = tmp[i * 3 + 0];
      o[1] = tmp[i * 3 + 1];
      o[2] = tmp[i * 3 + 2];
    }
  }
  HIP_TRY(hipGetLastError());
}

// device-resident cloud, transformed by a float matrix (pcl::transformPointCloud), to the host in ORIGINAL point order
void download_transformed(ngicp* h, DeviceCloud& dc, const float T_colmajor[16], float* out, size_t out_stride) {
  const size_t n = dc.n;
  h->tfinal.ensure(16 * sizeof(float));
  h->out_xyz.ensure(n * 3 * sizeof(float));
  HIP_TRY(hipMemcpyAsync(h->tfinal.p, T_colmajor, 16 * sizeof(float), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_transform_sorted_to_original, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, dc.pts(), (int)n, h->tfinal.as<float>(), h->out_xyz.as<float>());
  download_xyz(h, n, out, out_stride);
}

// ---- what do_align and do_align_voxel share: the host's wait on the device's progress, and what an alignment leaves on the handle ----
// One turn of the wait for the solver's published progress: give up after 30 s, otherwise yield or pause.
inline void wait_for_the_loop(ngicp* h, unsigned long& spins, double t_loop) {
  if ((++spins & (h->host_wait ? 0xfff : 0xfffff)) == 0 && now_ms() - t_loop > 30000.0) throw ArgError{NGICP_ERR_HIP, "the registration loop did not finish within 30 s"};
  if (h->host_wait) sched_yield(); else __builtin_ia32_pause();
}

// The final state's results, the transformed cloud if asked for, and the statistics that do not depend on the pass kernel.
void publish_alignment(ngicp* h, const LmState& st, float loop_ms, float* aligned, size_t out_stride) {
  pose_to_colmajor_f(st.hot.x0, h->final_T);
  h->converged = st.hot.converged;
  h->nr_iterations = st.hot.nr_iterations;
  for (int r = 0; r < 6; ++r)
    for (int cc = 0; cc < 6; ++cc) h->final_hessian[cc * 6 + r] = st.hot.final_H[r * 6 + cc];
  if (st.hot.lm_failed) std::fprintf(stderr, "lm not converged!!\n");  // impl/lsq_registration_impl.hpp:106
  h->trace_host.clear();  // fetched on demand (ngicp_get_lm_trace): a diagnostic should not cost every align a synchronous copy
  h->trace_rows_dev = (size_t)st.hot.n_trace;
  if (aligned) download_transformed(h, *h->src.dev, h->final_T, aligned, out_stride);  // K5: pcl::transformPointCloud(*input_, output, final_transformation_)
  if (st.hot.have_lin) h->hook_valid = 2;  // ngicp_get_correspondences: the correspondences of the last adopted linearisation
  ngicp_stats& s = h->stats;
  s.loop_ms = loop_ms;
  s.passes = st.hot.passes;
  s.outer_iterations = st.hot.nr_iterations + 1;
  s.lm_trials = st.hot.n_trace;
  s.mean_candidates = st.hot.passes > 0 ? st.hot.cand_total / ((double)st.hot.passes * (double)h->src.dev->n) : 0.0;
  s.valid_fraction = st.hot.passes > 0 ? st.hot.valid_total / ((double)st.hot.passes * (double)h->src.dev->n) : 0.0;
  s.pass_ms_total = 0.0;
  s.passes_timed = 0;
}

// With profiling on: HIP events on the handle's own stream around every prof_stride-th pass launch that did work.
void sum_event_pass_times(ngicp* h, long passes) {
  if (!h->profiling) return;
  ngicp_stats& s = h->stats;
  const long timed = std::min<long>(passes, (long)h->prof_events.size() / 2);
  int counted = 0;
  for (long i = h->prof_stride / 2; i < timed; i += h->prof_stride) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->prof_events[2 * i], h->prof_events[2 * i + 1]) == hipSuccess) {
      s.pass_ms_total += ms;
      ++counted;
    }
  }
  s.passes_timed = counted;
}

void do_align(ngicp* h, const float guess[16], float* aligned, size_t out_stride) {
  const double t_begin = now_ms();
  h->hook_valid = 0;
  h->converged = 0;
  h->nr_iterations = 0;
  const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::memcpy(h->final_T, I, sizeof(I));  // PCL align(): final_transformation_ = Identity before computeTransformation
  LoopCtx c;
  prepare_loop(h, c);
  LmState st;
  init_state_from_pose(st, pose_from_colmajor_f(guess));
  // the launch order the previous align ended with is still a good guess when the source index is the same one
  // (same batches; the costs come mostly from where the batches lie): the first pass then starts sorted as well
  // (the flag lives in a device word of its own: the solver sets it when an order is complete, the host only clears it when the
  // source index or the group count changed - it never has to read it back)
  if (!(h->order_src == h->src.dev.get() && h->order_groups == c.sa.nblocks)) HIP_TRY(hipMemsetAsync(h->order_flag.p, 0, 4 * sizeof(int), h->stream));  // (both flags)
  // NGICP_ORDER=xcd (experiment): instead of the cost-sorted launch order, a FIXED order that hands every XCD (blocks b, b + 8, ...
  // are observed to share one) a contiguous eighth of the Morton-ordered groups: each XCD's L2 then sees an eighth of the target.
  static const bool xcd_order = std::getenv("NGICP_ORDER") && std::string(std::getenv("NGICP_ORDER")) == "xcd";
  if (xcd_order) {
    const int nb = c.nblocks, per = (nb + 7) / 8;
    std::vector<int> ord((size_t)nb);
    std::vector<int> lists[8];
    for (int g = 0; g < nb; ++g) lists[std::min(7, g / per)].push_back(g);
    size_t taken[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int b = 0;
    for (int placed = 0; placed < nb; ++b) {  // block b belongs to XCD b % 8: the next group of that XCD's list, or of the fullest one left
      int x = b % 8;
      if (taken[x] >= lists[x].size()) {
        x = 0;
        for (int y = 1; y < 8; ++y)
          if (lists[y].size() - taken[y] > lists[x].size() - taken[x]) x = y;
      }
      ord[(size_t)placed++] = lists[x][taken[x]++];
    }
    HIP_TRY(hipMemcpyAsync(const_cast<int*>(c.pa.grp_order), ord.data(), (size_t)nb * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int one = 1;
    HIP_TRY(hipMemcpy(const_cast<int*>(c.pa.order_valid), &one, sizeof(int), hipMemcpyHostToDevice));
    c.sa.grp_order = nullptr;  // the solver leaves the order alone
  }
  c.pa.mode = (h->p.optimizer == NGICP_OPT_GAUSS_NEWTON) ? 2 : 3;
  // Whether the FIRST pass lists the region rows of every batch (later passes list for the batches that looked beyond ring 1 in the
  // pass before): it pays where many queries do (100k -> 500k with DLO's settings: 22 % of the batches, scan-to-submap 0.67 -> 0.64 ms)
  // and costs where few do (250k -> 2M: first pass 107 -> 72 us without).  Decided from the share of queries the previous alignment
  // of this handle served through lists; yes when there was none.
  if (h->prev_staged_fraction < 0.0 || h->prev_staged_fraction >= 0.12) c.pa.mode |= 32;
  if (const char* dbg = std::getenv("NGICP_DEBUG_MODE")) c.pa.mode |= (std::atoi(dbg) & (8 | 16));  // timing experiments only
  if (h->p.max_iter <= 0) st.hot.done = 1;
  h->pin_state[0] = st;
  HIP_TRY(hipMemcpyAsync(h->state.p, &h->pin_state[0], sizeof(st), hipMemcpyHostToDevice, h->stream));

  const char* stamp_path = std::getenv("NGICP_DEBUG_STAMPS");  // diagnostic only
  if (stamp_path) {
    h->dbg.ensure((size_t)(c.nblocks + 1) * 4 * kStampStride * sizeof(unsigned long long));  // (k_gicp_head has one block more)
    HIP_TRY(hipMemsetAsync(h->dbg.p, 0, (size_t)(c.nblocks + 1) * 4 * kStampStride * sizeof(unsigned long long), h->stream));
    c.pa.dbg_stamps = h->dbg.as<unsigned long long>();
  }
  if (std::getenv("NGICP_DEBUG_SOLVE")) {  // diagnostic only: s_memtime stamps of the last solver launch, printed after the align
    h->dbg_s.ensure(8 * sizeof(unsigned long long));
    HIP_TRY(hipMemsetAsync(h->dbg_s.p, 0, 8 * sizeof(unsigned long long), h->stream));
    c.sa.dbg_stamps = h->dbg_s.as<unsigned long long>();
  }
  const char* span_path = std::getenv("NGICP_DEBUG_SPAN");  // diagnostic only: when and where every block of the last pass ran
  if (span_path) {
    h->dbg_span.ensure((size_t)c.nblocks * 4 * sizeof(unsigned long long));
    HIP_TRY(hipMemsetAsync(h->dbg_span.p, 0, (size_t)c.nblocks * 4 * sizeof(unsigned long long), h->stream));
    c.pa.dbg_span = h->dbg_span.as<unsigned long long>();
  }
  const char* qstat_path = std::getenv("NGICP_DEBUG_QSTATS");  // diagnostic only: per-query search statistics of the last pass
  if (qstat_path) {
    h->dbg_q.ensure((size_t)c.pa.n_src * 2 * sizeof(int4));
    HIP_TRY(hipMemsetAsync(h->dbg_q.p, 0, (size_t)c.pa.n_src * 2 * sizeof(int4), h->stream));
    c.pa.dbg_qstats = h->dbg_q.as<int4>();
  }
  const long max_passes = (h->p.optimizer == NGICP_OPT_GAUSS_NEWTON) ? (long)h->p.max_iter : (long)h->p.max_iter * std::max(1, h->p.lm_max_iter) + 1;
  // The host feeds (pass, solve) pairs to the stream and never blocks on it inside the loop: the solver publishes its progress
  // {passes done, done flag} in PINNED host memory (one system-scope store), the host keeps `depth` pairs in flight and stops
  // feeding when it sees the flag.  At most `depth` pairs are enqueued in vain (they return at once: the state says done);
  // round 1 polled a copied flag one chunk of four pairs behind and wasted up to eight.
  const int depth = h->chunk_pairs;
  *h->h_progress = 0;
  c.sa.progress_host = h->h_progress;
  c.sa.final_host = h->pin_final;
  c.sa.t_first = h->t_first.as<unsigned long long>();
  c.pa.t_first = h->t_first.as<unsigned long long>();
  // NGICP_FUSED=1: one dispatch per iteration - the last block of the pass reduces and advances the optimiser (PassArgs::fused).
  // Measured on MI355X (round 3, profiles/r03_fused_solver.txt): bit-identical results, but no faster than the separate launch (c3
  // 46.3 vs 45.4 us per iteration, c5 70 vs 56): the write-through rows come back from memory, not from L2, through ONE CU
  // (8.7 k cycles for 222 KB against 5.5 k in k_lm_solve), plus the acquire (~1.7 us) - so the default stays two launches.
  static const bool fused_env = std::getenv("NGICP_FUSED") && std::atoi(std::getenv("NGICP_FUSED")) != 0;
  if (fused_env && pass_impl() == 0) {
    c.pa.fused = 1;
    c.pa.sa = c.sa;
    HIP_TRY(hipMemsetAsync(c.pa.ticket, 0, sizeof(int), h->stream));
  }
  long launched = 0;
  bool finished = (h->p.max_iter <= 0), persist_done = false;
  float persist_loop_ms = 0.f;
  const double t_loop = now_ms();
  unsigned long spins = 0;
  // ---- NGICP_PERSIST=1 (experiment, round 3): ONE launch for the whole alignment (k_gicp_persist): as many blocks as are resident
  //      together, each keeping its groups pass after pass; the last block to finish a pass steps the optimiser and releases the next
  //      one.  The idea: no second dispatch, no kernel boundaries - and with them no cold caches (a launch boundary drops every L2, and
  //      ~9 of 10 L2 read requests of a pass go out to the fabric: profiles/r03_c3_pass_counters.json).  Measured (profiles/
  //      r03_persistent_kernel.txt): bit-identical results; the groups run 4 % faster, but every hop of the grid-wide meeting (rows
  //      written through, ticket, state, release word, view) is a ~1-2 us round trip to memory, as long as the launches they replace:
  //      c3 50.7 us per iteration against 48.2, c5 76 against 58 (it has no 4-waves build).  So the default stays one launch per pass.
  //      Launched cooperatively: the runtime guarantees that the grid is resident as a whole (the blocks wait for each other), and
  //      one alignment per device at a time takes this route. ----
  bool persist_lock = false;
  const bool want_persist = h->persist && !finished && h->persist_slots > 0 && pass_impl() == 0 && !c.pa.fused && !xcd_order && !stamp_path && !span_path && !qstat_path &&
                            !c.sa.dbg_stamps && max_passes + 1 <= kMaxPersistPasses;
  if (want_persist) persist_lock = persist_mutex(h->device).try_lock();
  if (persist_lock) {
    struct Unlock {
      std::mutex& m;
      ~Unlock() { m.unlock(); }
    } unlock{persist_mutex(h->device)};
    int* const ctl = h->order_flag.as<int>();
    const int sel = h->order_sel;
    // {flag 0, ticket, gen, flag 1}: ticket and gen start at zero, and so does the flag of the buffer this alignment's solver will fill
    HIP_TRY(hipMemsetAsync(ctl + (sel == 0 ? 1 : 0), 0, 3 * sizeof(int), h->stream));
    HIP_TRY(hipMemsetAsync(h->gen_lines.p, 0, (size_t)kGenLines * kGenStride * sizeof(int), h->stream));
    PassArgs pa = c.pa;
    pa.fused = 1;
    pa.persist = 1;
    pa.max_passes = (int)max_passes;
    pa.sa = c.sa;
    pa.sa.persist = 1;
    pa.sa.grp_order = sel == 0 ? h->grp_order_alt.as<int>() : h->grp_order.as<int>();
    pa.sa.order_valid = sel == 0 ? ctl + 3 : ctl;
    pa.sa.pass_ticks = (h->profiling && max_passes <= kMaxTickPasses) ? h->pin_ticks : nullptr;
    const int grid = std::min(c.nblocks, h->persist_slots);
    void* kargs[] = {&pa};
    static const bool coop = !(std::getenv("NGICP_PERSIST_COOP") && std::atoi(std::getenv("NGICP_PERSIST_COOP")) == 0);
    bool launched_ok = true;
    if (coop) {
      const hipError_t le = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(&k_gicp_persist<2, 3>), dim3((unsigned)grid), dim3(256), kargs, 0, h->stream);
      if (le != hipSuccess) {  // (e.g. the runtime finds the grid too large to be resident: one launch per pass then)
        (void)hipGetLastError();
        launched_ok = false;
      }
    } else {  // (A/B timing only: an ordinary launch relies on nothing else running on the device)
      hipLaunchKernelGGL((k_gicp_persist<2, 3>), dim3((unsigned)grid), dim3(256), 0, h->stream, pa);
    }
    bool ok = false;
    while (launched_ok) {
      const int prog = __atomic_load_n(h->h_progress, __ATOMIC_ACQUIRE);
      if (prog & kProgressDone) {
        ok = true;
        break;
      }
      if ((++spins & 0x3fff) == 0) {
        if (hipStreamQuery(h->stream) == hipSuccess) {  // the kernel has left: done flag (then it is in memory by now), or its blocks gave up waiting
          ok = (__atomic_load_n(h->h_progress, __ATOMIC_ACQUIRE) & kProgressDone) != 0;
          break;
        }
        if (now_ms() - t_loop > 30000.0) throw ArgError{NGICP_ERR_HIP, "the registration loop did not finish within 30 s"};
      }
      if (h->host_wait) sched_yield(); else __builtin_ia32_pause();
    }
    if (ok) {
      finished = true;
      st.hot = *h->pin_final;
      persist_loop_ms = (float)((double)(st.hot.t_done - st.hot.t_first) * 1e-5);
      persist_done = true;
      if (st.hot.passes >= 3 && c.nblocks <= kMaxOrderGroups) h->order_sel = sel ^ 1;  // the solver of the third pass left a fresh order in the other buffer
    } else {
      // (never seen: the blocks' bounded wait ran out - e.g. the grid was not resident as a whole.  The state goes back to the guess and the
      // alignment takes one launch per pass.)
      std::fprintf(stderr, launched_ok ? "ngicp: the persistent registration kernel gave up waiting; falling back to one launch per pass\n"
                                       : "ngicp: the persistent registration kernel could not be launched; falling back to one launch per pass\n");
      h->persist = 0;
      HIP_TRY(hipMemsetAsync(h->order_flag.p, 0, 4 * sizeof(int), h->stream));
      HIP_TRY(hipMemcpyAsync(h->state.p, &h->pin_state[0], sizeof(st), hipMemcpyHostToDevice, h->stream));
      *h->h_progress = 0;
    }
  }
  // ---- NGICP_HEAD=1: no solver launch at all (k_gicp_head): one launch per iteration, and one more whose head consumes the last pass ----
  const bool head_mode = h->head && !finished && pass_impl() == 0 && !c.pa.fused && !xcd_order && !span_path && !qstat_path && !c.sa.dbg_stamps &&
                         c.nblocks <= 2 * h->pass_slots;  // (grids of more rounds: the head's few microseconds are paid once per round)
  LmState* head_state[2] = {nullptr, nullptr};
  double* head_crow[2] = {nullptr, nullptr};
  int *head_tickets = nullptr, *head_done = nullptr, *head_order[2] = {nullptr, nullptr}, *head_flag[2] = {nullptr, nullptr};
  if (head_mode) {
    h->state_alt.ensure(sizeof(LmState));
    const size_t crow_bytes = (size_t)kSolveRowSubsets * kNumSlots * sizeof(double);
    h->head_ws.ensure(64 + 128 + 2 * crow_bytes);
    HIP_TRY(hipMemsetAsync(h->head_ws.p, 0, 64 + 128 + 2 * crow_bytes, h->stream));
    unsigned char* ws = h->head_ws.as<unsigned char>();
    head_done = reinterpret_cast<int*>(ws);
    head_tickets = reinterpret_cast<int*>(ws + 64);
    head_crow[0] = reinterpret_cast<double*>(ws + 192);
    head_crow[1] = reinterpret_cast<double*>(ws + 192 + crow_bytes);
    head_state[0] = h->state.as<LmState>();
    head_state[1] = h->state_alt.as<LmState>();
    int* const ctl = h->order_flag.as<int>();
    head_order[0] = h->grp_order.as<int>();
    head_order[1] = h->grp_order_alt.as<int>();
    head_flag[0] = ctl;
    head_flag[1] = ctl + 3;
  }
  const long max_launches = head_mode ? max_passes + 1 : max_passes;
  while (!finished && launched < max_launches) {
    const int prog = *reinterpret_cast<volatile int*>(h->h_progress);
    if (prog & kProgressDone) break;
    if (launched - (long)(prog & kProgressMask) >= depth) {  // enough in flight: wait for the device to catch up
      wait_for_the_loop(h, spins, t_loop);
      continue;
    }
    const bool timed = h->profiling && launched % h->prof_stride == h->prof_stride / 2 && (size_t)(2 * launched + 1) < h->prof_events.size();
    if (head_mode) {
      // k_gicp_head: launch i reads state / subset rows / launch order [i & 1] and leaves the next ones in [(i + 1) & 1]
      const int par = (int)(launched & 1);
      PassArgs pa = c.pa;
      pa.st = head_state[par];
      pa.crow_in = head_crow[par];
      pa.crow_out = head_crow[par ^ 1];
      pa.cluster_ticket = head_tickets;
      pa.done_flag = head_done;
      pa.grp_order = head_order[par];
      pa.order_valid = head_flag[par];
      pa.sa = c.sa;
      pa.sa.st = head_state[par];
      pa.sa.st_out = head_state[par ^ 1];
      pa.sa.partials = head_crow[par];
      pa.sa.nrows = kSolveRowSubsets;
      pa.sa.grp_order = head_order[par ^ 1];
      pa.sa.order_valid = head_flag[par ^ 1];
      hipExtLaunchKernelGGL((k_gicp_head<2, 3>), dim3((unsigned)c.nblocks + 1), dim3(256), 0, h->stream, timed ? h->prof_events[2 * launched] : nullptr,
                            timed ? h->prof_events[2 * launched + 1] : nullptr, 0, pa);
      ++launched;
      continue;
    }
    static const bool persist_one = std::getenv("NGICP_PERSIST_ONE") != nullptr;  // A/B only: the persistent kernel's code, one launch per pass
    if (persist_one && h->persist_slots > 0 && max_passes + 1 <= kMaxPersistPasses) {
      PassArgs pa = c.pa;
      pa.fused = 1;
      pa.persist = std::atoi(std::getenv("NGICP_PERSIST_ONE")) == 2 ? 2 : 1;
      pa.first_pass = (int)launched;
      pa.max_passes = 1;
      pa.sa = c.sa;
      pa.sa.persist = 1;
      HIP_TRY(hipMemsetAsync(pa.ticket, 0, sizeof(int), h->stream));
      HIP_TRY(hipMemsetAsync(h->gen_lines.p, 0, (size_t)kGenLines * kGenStride * sizeof(int), h->stream));
      hipExtLaunchKernelGGL((k_gicp_persist<2, 3>), dim3((unsigned)std::min(c.nblocks, h->persist_slots)), dim3(256), 0, h->stream,
                            timed ? h->prof_events[2 * launched] : nullptr, timed ? h->prof_events[2 * launched + 1] : nullptr, 0, pa);
      ++launched;
      continue;
    }
    launch_pass(h, c.pa, c.nblocks, h->stream, timed ? h->prof_events[2 * launched] : nullptr, timed ? h->prof_events[2 * launched + 1] : nullptr);
    if (!c.pa.fused) hipLaunchKernelGGL(k_lm_solve, dim3(1), dim3(kSolveThreads), 0, h->stream, c.sa);
    ++launched;
  }
  float loop_ms = 0.f;
  if (persist_done) {
    loop_ms = persist_loop_ms;
  } else if (finished) {
    HIP_TRY(hipStreamSynchronize(h->stream));  // (max_iterations <= 0: nothing was launched; the state is the initial one)
  } else {
    // The solver writes the final state image into pinned memory and THEN raises the done flag (system-scope release): no copy,
    // no event, no stream synchronisation - the few launches enqueued ahead return at once behind the host's back, and whatever
    // this handle enqueues next is ordered behind them on its stream.
    for (;;) {
      const int prog = __atomic_load_n(h->h_progress, __ATOMIC_ACQUIRE);
      if (prog & kProgressDone) break;
      if (launched >= max_launches && launched - (long)(prog & kProgressMask) <= 0) break;  // (cannot happen: the last possible pass sets done)
      wait_for_the_loop(h, spins, t_loop);
    }
    st.hot = *h->pin_final;
    loop_ms = (float)((double)(st.hot.t_done - st.hot.t_first) * 1e-5);  // 100 MHz ticks -> ms
    // (k_gicp_head: the head of launch `passes` ended the alignment and left the final state in the buffer it does not read; the handle's
    // other entry points look for it in h->state)
    if (head_mode && ((st.hot.passes + 1) & 1)) HIP_TRY(hipMemcpyAsync(h->state.p, h->state_alt.p, sizeof(LmState), hipMemcpyDeviceToDevice, h->stream));
  }
  HIP_TRY(hipGetLastError());

  if (stamp_path) {
    std::vector<unsigned long long> hs((size_t)(c.nblocks + 1) * 4 * kStampStride);
    HIP_TRY(hipMemcpy(hs.data(), h->dbg.p, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (FILE* f = std::fopen(stamp_path, "wb")) {
      std::fwrite(hs.data(), sizeof(unsigned long long), hs.size(), f);
      std::fclose(f);
    }
  }
  if (c.sa.dbg_stamps) {
    unsigned long long ts[8];
    HIP_TRY(hipMemcpy(ts, h->dbg_s.p, sizeof(ts), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "k_lm_solve stamps (cycles since entry): loads issued %llu, reduced %llu, state in registers %llu, lm_advance %llu, accept path %llu, stored %llu; launch-order section (wave 1) %llu cycles\n",
                 ts[1] - ts[0], ts[2] - ts[0], ts[3] - ts[0], ts[4] - ts[0], ts[5] - ts[0], ts[6] - ts[0], ts[7]);
  }
  if (span_path) {
    std::vector<unsigned long long> hs((size_t)c.nblocks * 4);
    HIP_TRY(hipMemcpy(hs.data(), h->dbg_span.p, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (FILE* f = std::fopen(span_path, "wb")) {
      std::fwrite(hs.data(), sizeof(unsigned long long), hs.size(), f);
      std::fclose(f);
    }
  }
  if (const char* cost_path = std::getenv("NGICP_DEBUG_COSTS")) {  // diagnostic only: the groups' durations in the last pass (cycles >> 4), the launch order, the partial rows
    std::vector<int> hc((size_t)c.nblocks * 2);
    HIP_TRY(hipMemcpy(hc.data(), h->grp_cost.p, (size_t)c.nblocks * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hc.data() + c.nblocks, h->grp_order.p, (size_t)c.nblocks * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<double> hp((size_t)c.nblocks * kNumSlots);
    HIP_TRY(hipMemcpy(hp.data(), h->partials.p, hp.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (FILE* f = std::fopen(cost_path, "wb")) {
      std::fwrite(hc.data(), sizeof(int), hc.size(), f);
      std::fwrite(hp.data(), sizeof(double), hp.size(), f);
      std::fclose(f);
    }
  }
  if (qstat_path) {
    std::vector<int> hq((size_t)c.pa.n_src * 8);
    HIP_TRY(hipMemcpy(hq.data(), h->dbg_q.p, hq.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (FILE* f = std::fopen(qstat_path, "wb")) {
      std::fwrite(hq.data(), sizeof(int), hq.size(), f);
      std::fclose(f);
    }
  }
  publish_alignment(h, st, loop_ms, aligned, out_stride);
  ngicp_stats& s = h->stats;
  h->order_src = h->src.dev.get();  // (what the order flag on the device, if set, refers to)
  h->order_groups = c.sa.nblocks;
  s.staged_fraction = st.hot.passes > 0 ? st.hot.staged_total / ((double)st.hot.passes * (double)h->src.dev->n) : 0.0;
  if (st.hot.passes > 1) h->prev_staged_fraction = s.staged_fraction;
  if (h->profiling && persist_done) {
    // the persistent kernel's own stamps (100 MHz): a pass lasts from its release (the first: the alignment's first stamp) to the arrival
    // of its last block; the optimiser's step and the release that follows are not part of it
    const long timed = std::min<long>(st.hot.passes, kMaxTickPasses);
    int counted = 0;
    if ((long)h->p.max_iter * std::max(1, h->p.lm_max_iter) + 1 <= kMaxTickPasses) {
      for (long i = 0; i < timed; ++i) {
        const unsigned long long from = i == 0 ? st.hot.t_first : h->pin_ticks[2 * (i - 1) + 1], to = h->pin_ticks[2 * i];
        if (to > from) {
          s.pass_ms_total += (double)(to - from) * 1e-5;
          ++counted;
        }
      }
    }
    s.passes_timed = counted;
    if (std::getenv("NGICP_DEBUG_TICKS")) {  // diagnostic only: every pass and every step of the alignment, in microseconds
      std::fprintf(stderr, "persistent kernel, pass / step us:");
      for (long i = 0; i < timed; ++i) {
        const unsigned long long from = i == 0 ? st.hot.t_first : h->pin_ticks[2 * (i - 1) + 1];
        std::fprintf(stderr, " %.1f/%.1f", (double)(h->pin_ticks[2 * i] - from) * 1e-2, (double)(h->pin_ticks[2 * i + 1] - h->pin_ticks[2 * i]) * 1e-2);
      }
      std::fprintf(stderr, "\n");
    }
  } else {
    sum_event_pass_times(h, st.hot.passes);
  }
  s.n_src = (long long)h->src.dev->n;
  s.n_tgt = (long long)h->tgt.dev->n;
  s.host_wait_spins = (long long)spins;
  s.align_ms = now_ms() - t_begin;
}

// ------------------------------------------------------------------------------------------
// Voxelized GICP (ngicp_voxel.h): a mode the caller selects with ngicp_set_voxel_resolution
// ------------------------------------------------------------------------------------------
void refuse_if_voxelized(ngicp* h, const char* entry) {
  if (h->voxel_res > 0.0) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": not available with a voxelized target (ngicp_set_voxel_resolution(h, 0) selects exact GICP)"};
}

// The target, or its covariances, changed: the voxel map goes, and while the mode is on so do the correspondences, which are its voxel
// numbers (ngicp_get_correspondences would read the next map's records with them).  Exact GICP's correspondences are left as they were.
void drop_voxel_map(ngicp* h) {
  h->vmap.invalidate();
  if (h->voxel_res > 0.0) h->hook_valid = 0;
}

// The working buffers of a voxel build over a list of up to n (key, value) pairs.  Every build sizes them for its longest list before
// its first launch: growing a buffer frees it, and freeing waits for the device.
void size_voxel_work(ngicp* h, size_t n) {
  h->vox_keys.ensure(n * 2 * sizeof(unsigned long long));
  h->vox_vals.ensure(n * 2 * sizeof(int));
  h->vox_scan.ensure((n * 3 + 2 + kCellPad) * sizeof(int));
  h->vox_flag.ensure(64);
  h->tile_sums.ensure(((n + kScanTile - 1) / kScanTile) * sizeof(int));
}

// What a build's numbering step leaves on the device: the keys sorted (stable), the values beside them, where every run of equal keys
// starts (n_seg + 1 entries) and the number of runs.
struct VoxelSegments {
  const unsigned long long* keys;
  const int* order;
  const int* seg_start;
  const int* n_seg_dev;
};

// The n pairs at the front of vox_keys / vox_vals: stable radix sort, segment heads, exclusive scan, segment starts.  Shared by the map
// of a target's points, a keyframe's part and the merge of parts.  Nothing is synchronised.
VoxelSegments voxel_segments(ngicp* h, int n) {
  const unsigned blocks = (unsigned)((n + 255) / 256);
  const int ntiles = (n + kScanTile - 1) / kScanTile;
  unsigned long long* keys_a = h->vox_keys.as<unsigned long long>();
  unsigned long long* keys_b = keys_a + n;
  int* vals_a = h->vox_vals.as<int>();
  int* vals_b = vals_a + n;
  int* head = h->vox_scan.as<int>();
  int* vox_of = head + n;                    // n + 1 + kCellPad
  int* seg_start = vox_of + n + 1 + kCellPad;  // n + 1
  char err[256] = {0};
  int in_a = 1;
  if (ngk_sort_pairs_u64(h->stream, &h->vox_ws, keys_a, keys_b, vals_a, vals_b, n, kVoxKeyBits, &in_a, err, sizeof(err))) throw ArgError{NGICP_ERR_HIP, err};
  const unsigned long long* keys = in_a ? keys_a : keys_b;
  const int* order = in_a ? vals_a : vals_b;
  hipLaunchKernelGGL(k_voxel_map_heads, dim3(blocks), dim3(256), 0, h->stream, keys, n, head);
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(kScanBlock), 0, h->stream, (const int*)head, n, h->tile_sums.as<int>(), (unsigned long long*)nullptr);
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(kScanBlock), 0, h->stream, h->tile_sums.as<int>(), ntiles, (const unsigned long long*)nullptr, (unsigned long long*)nullptr);
  hipLaunchKernelGGL(k_scan_apply, dim3(ntiles), dim3(kScanBlock), 0, h->stream, (const int*)head, n, (const int*)h->tile_sums.as<int>(), vox_of);
  hipLaunchKernelGGL(k_voxel_map_starts, dim3(blocks), dim3(256), 0, h->stream, (const int*)head, (const int*)vox_of, n, seg_start);
  return VoxelSegments{keys, order, seg_start, vox_of + n};
}

// the points of an indexed cloud -> (voxel key, sorted position) pairs in ORIGINAL order at the front of vox_keys / vox_vals, numbered;
// vox_flag is set when a point has no voxel
VoxelSegments voxel_segments_of_cloud(ngicp* h, const DeviceCloud& dc) {
  const int n = (int)dc.n;
  const float inv_res = 1.0f / (float)h->voxel_res;
  HIP_TRY(hipMemsetAsync(h->vox_flag.p, 0, sizeof(int), h->stream));
  hipLaunchKernelGGL(k_voxel_map_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, dc.pts(), n, inv_res, h->vox_keys.as<unsigned long long>(), h->vox_vals.as<int>(),
                     h->vox_flag.as<int>());
  return voxel_segments(h, n);
}

// sizes the map's own buffers for n_vox voxels, clears the table and returns its slot count (the stream is idle: the count was just read)
size_t size_voxel_map(ngicp* h, ngicp::VoxelMap& m, int n_vox) {
  size_t slots = 64;
  while (slots < 2 * (size_t)n_vox) slots <<= 1;
  m.rec.ensure((size_t)n_vox * kVoxRec * sizeof(double));
  m.vkeys.ensure((size_t)n_vox * sizeof(unsigned long long));
  m.table.ensure(slots * sizeof(ulonglong2));
  HIP_TRY(hipMemsetAsync(m.table.p, 0xff, slots * sizeof(ulonglong2), h->stream));
  return slots;
}

// The map from the target's points, "summed in ascending original target index".  Two host synchronisations (the voxel count sizes the
// map; the build time).
void build_voxel_map_from_points(ngicp* h, const double* covs) {
  ngicp::VoxelMap& m = h->vmap;
  DeviceCloud& T = *h->tgt.dev;
  const int n = (int)T.n;
  size_voxel_work(h, (size_t)n);
  HIP_TRY(hipEventRecord(h->ev_vox_a, h->stream));
  const VoxelSegments sg = voxel_segments_of_cloud(h, T);
  int n_vox = 0, bad = 0;
  HIP_TRY(hipMemcpyAsync(&n_vox, sg.n_seg_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(&bad, h->vox_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  if (bad) throw ArgError{NGICP_ERR_ARG, "voxelized target: a point lies 2^20 voxels or more from the origin on some axis (or is not finite); use a coarser resolution"};
  if (n_vox <= 0 || n_vox > n) throw ArgError{NGICP_ERR_HIP, "voxel map build: inconsistent voxel count"};
  const size_t slots = size_voxel_map(h, m, n_vox);
  hipLaunchKernelGGL(k_voxel_map_fill, dim3((unsigned)((n_vox + 255) / 256)), dim3(256), 0, h->stream, sg.keys, sg.order, sg.seg_start, n_vox, T.pts(), covs, m.rec.as<double>(),
                     m.vkeys.as<unsigned long long>(), m.table.as<ulonglong2>(), (unsigned int)(slots - 1));
  HIP_TRY(hipEventRecord(h->ev_vox_b, h->stream));
  HIP_TRY(hipEventSynchronize(h->ev_vox_b));
  HIP_TRY(hipGetLastError());
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, h->ev_vox_a, h->ev_vox_b) == hipSuccess) h->stats.voxelmap_ms = ms;
  m.n_vox = (size_t)n_vox;
  m.mask = (unsigned int)(slots - 1);
}

// ---- the merged route (include/ngicp.h "merged voxel map") ----
bool keyframe_part_current(const ngicp* h, const ngicp::Keyframe& kf) { return kf.part && kf.part->res == h->voxel_res; }

// The voxel part of keyframe `id` at the handle's resolution.  The caller has sized the working buffers for the keyframe's points.
// One host synchronisation (the voxel count sizes the part); the fill is left in the stream.
void build_keyframe_part(ngicp* h, int id) {
  ngicp::Keyframe& kf = h->keyframes[(size_t)id];
  const int n = (int)kf.cloud->n;
  const VoxelSegments sg = voxel_segments_of_cloud(h, *kf.cloud);
  int n_vox = 0, bad = 0;
  HIP_TRY(hipMemcpyAsync(&n_vox, sg.n_seg_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(&bad, h->vox_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  if (bad)
    throw ArgError{NGICP_ERR_ARG, "voxel part of keyframe " + std::to_string(id) +
                                      ": a point lies 2^20 voxels or more from the origin on some axis (or is not finite); use a coarser resolution"};
  if (n_vox <= 0 || n_vox > n) throw ArgError{NGICP_ERR_HIP, "voxel part build: inconsistent voxel count"};
  auto part = std::make_shared<ngicp::VoxelPart>();
  part->keys.ensure((size_t)n_vox * sizeof(unsigned long long));
  part->rec.ensure((size_t)n_vox * kVoxRec * sizeof(double));
  hipLaunchKernelGGL(k_voxel_part_fill, dim3((unsigned)((n_vox + 255) / 256)), dim3(256), 0, h->stream, sg.keys, sg.order, sg.seg_start, n_vox, kf.cloud->pts(),
                     (const double*)kf.covs->as<double>(), part->rec.as<double>(), part->keys.as<unsigned long long>());
  HIP_TRY(hipGetLastError());
  part->res = h->voxel_res;
  part->n_vox = (size_t)n_vox;
  kf.part = part;  // (a part of another resolution goes here)
  ++h->parts_built;
}

// Is the current target the device submap with the covariances ngicp_submap_set gave it?  Only then is the map a function of the
// keyframes' parts; after ngicp_set_target_covs / ngicp_compute_target_covs it is built from the points.
bool merged_route_applies(const ngicp* h) {
  if (!h->voxel_merge || h->submap_ids.empty() || !h->tgt.dev || h->tgt.dev.get() != h->submap_cloud || !h->tgt_covs.data) return false;
  return h->submap_covs.lock() == h->tgt_covs.data;
}

// The map of the submap `submap_ids` from its keyframes' parts: missing parts are built (one synchronisation each), the parts' keys are
// gathered in list order with their global record position, sorted (stable: a voxel's parts stay in list order), numbered, and one
// thread per merged voxel adds its parts and divides.  Two more synchronisations: the merged count, the time.
void build_voxel_map_merged(ngicp* h) {
  ngicp::VoxelMap& m = h->vmap;
  const std::vector<int>& ids = h->submap_ids;
  const size_t mk = ids.size();
  size_t longest = 1, bound = 0;  // the longest list a part build sorts; an upper bound of the gathered list (a missing part: its points)
  for (int id : ids) {
    const ngicp::Keyframe& kf = h->keyframes[(size_t)id];
    const bool have = keyframe_part_current(h, kf);
    if (!have) longest = std::max(longest, kf.cloud->n);
    bound += have ? kf.part->n_vox : kf.cloud->n;
  }
  if (bound > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "merged voxel map: too many keyframe voxels for int indices"};
  size_voxel_work(h, std::max(longest, bound));
  const size_t tab_off = ((mk + 1) * sizeof(int) + 7) / 8 * 8, tab_bytes = tab_off + mk * sizeof(const double*);
  h->vox_part_tab.ensure(tab_bytes);
  HIP_TRY(hipEventRecord(h->ev_vox_a, h->stream));
  for (int id : ids)
    if (!keyframe_part_current(h, h->keyframes[(size_t)id])) build_keyframe_part(h, id);
  HIP_TRY(hipEventRecord(h->ev_vox_c, h->stream));
  std::vector<unsigned char> tab(tab_bytes, 0);  // (lives until the synchronisation below: the copy may read it late)
  int* off = reinterpret_cast<int*>(tab.data());
  const double** recs = reinterpret_cast<const double**>(tab.data() + tab_off);
  size_t total = 0;
  for (size_t i = 0; i < mk; ++i) {
    const ngicp::VoxelPart& part = *h->keyframes[(size_t)ids[i]].part;
    off[i] = (int)total;
    recs[i] = part.rec.as<double>();
    total += part.n_vox;
  }
  off[mk] = (int)total;
  const int G = (int)total;
  HIP_TRY(hipMemcpyAsync(h->vox_part_tab.p, tab.data(), tab_bytes, hipMemcpyHostToDevice, h->stream));
  for (size_t i = 0; i < mk; ++i) {
    const ngicp::VoxelPart& part = *h->keyframes[(size_t)ids[i]].part;
    const int nk = (int)part.n_vox;
    hipLaunchKernelGGL(k_voxel_part_gather, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, h->stream, (const unsigned long long*)part.keys.as<unsigned long long>(), nk, off[i],
                       h->vox_keys.as<unsigned long long>(), h->vox_vals.as<int>());
  }
  VoxelSegments sg{};
  try {
    sg = voxel_segments(h, G);
  } catch (...) {
    (void)hipStreamSynchronize(h->stream);  // the upload of `tab` may still be pending: it must not outlive the vector
    throw;
  }
  int n_vox = 0;
  HIP_TRY(hipMemcpyAsync(&n_vox, sg.n_seg_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  if (n_vox <= 0 || n_vox > G) throw ArgError{NGICP_ERR_HIP, "merged voxel map build: inconsistent voxel count"};
  const size_t slots = size_voxel_map(h, m, n_vox);
  hipLaunchKernelGGL(k_voxel_merge_fill, dim3((unsigned)((n_vox + 255) / 256)), dim3(256), 0, h->stream, sg.keys, sg.order, sg.seg_start, n_vox,
                     (const int*)h->vox_part_tab.as<int>(), reinterpret_cast<const double* const*>(h->vox_part_tab.as<unsigned char>() + tab_off), (int)mk, m.rec.as<double>(),
                     m.vkeys.as<unsigned long long>(), m.table.as<ulonglong2>(), (unsigned int)(slots - 1));
  HIP_TRY(hipEventRecord(h->ev_vox_b, h->stream));
  HIP_TRY(hipEventSynchronize(h->ev_vox_b));
  HIP_TRY(hipGetLastError());
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, h->ev_vox_a, h->ev_vox_b) == hipSuccess) h->stats.voxelmap_ms = ms;
  if (hipEventElapsedTime(&ms, h->ev_vox_a, h->ev_vox_c) == hipSuccess) h->last_parts_ms = ms;
  if (hipEventElapsedTime(&ms, h->ev_vox_c, h->ev_vox_b) == hipSuccess) h->last_merge_ms = ms;
  m.n_vox = (size_t)n_vox;
  m.mask = (unsigned int)(slots - 1);
  ++h->merged_builds;
}

// The voxel map of the current target, its covariances (computed if missing, as for align) and the resolution: built at the first use
// after any of the three changed, or after the route it would be built by did (ngicp_set_voxel_submap_merge).
void ensure_voxel_map(ngicp* h) {
  ensure_slot_ready(h, h->tgt, "target");
  if (h->tgt_covs.n != h->tgt.dev->n) compute_covs(h, h->tgt, h->tgt_covs, "target");
  const double* covs = covs_for(h, h->tgt_covs, h->tgt.dev);
  ngicp::VoxelMap& m = h->vmap;
  const int merged = merged_route_applies(h) ? 1 : 0;
  if (m.valid && m.res == h->voxel_res && m.cloud == h->tgt.dev && m.covs == h->tgt_covs.data && m.merged == merged) return;
  m.invalidate();
  if (merged) build_voxel_map_merged(h);
  else build_voxel_map_from_points(h, covs);
  m.merged = merged;
  m.res = h->voxel_res;
  m.cloud = h->tgt.dev;
  m.covs = h->tgt_covs.data;
  m.valid = true;
  ++h->voxel_builds;
}

struct VoxelCtx {
  VoxelPassArgs pa;
  SolveArgs sa;
  int nblocks;
};

// the pass of the neighbourhood in c.pa.nbr: k_vgicp_pass for DIRECT1, k_vgicp_pass_n<K> for DIRECT7 / DIRECT27; the same grid
void launch_voxel_pass(ngicp* h, const VoxelCtx& c, hipEvent_t start = nullptr, hipEvent_t stop = nullptr) {
  const dim3 grid((unsigned)c.nblocks), block(kVoxBlock);
  switch (c.pa.nbr) {
    case NGICP_VOX_DIRECT1: hipExtLaunchKernelGGL(k_vgicp_pass, grid, block, 0, h->stream, start, stop, 0, c.pa); break;
    case NGICP_VOX_DIRECT7: hipExtLaunchKernelGGL(k_vgicp_pass_n<7>, grid, block, 0, h->stream, start, stop, 0, c.pa); break;
    case NGICP_VOX_DIRECT27: hipExtLaunchKernelGGL(k_vgicp_pass_n<27>, grid, block, 0, h->stream, start, stop, 0, c.pa); break;
    default: throw ArgError{NGICP_ERR_STATE, "voxelized GICP: unknown neighbourhood"};
  }
}

// prepare_loop readies the slots, the covariances, the state, the trace and the solver's arguments exactly as for the exact path; the
// voxelized pass then brings its own grid (256 source points per block), its own rows and correspondence buffers.  The launch order of
// the exact pass's groups (grp_order, its flag) is neither read nor written.
void prepare_voxel_loop(ngicp* h, VoxelCtx& v) {
  LoopCtx c;
  prepare_loop(h, c);
  ensure_voxel_map(h);
  DeviceCloud& S = *h->src.dev;
  const size_t n = S.n;
  const int nblocks = std::max(1, (int)((n + kVoxBlock - 1) / kVoxBlock));
  h->partials.ensure((size_t)kNumSlots * nblocks * sizeof(double));
  // slot-major state of the neighbourhood in use: corr[2][K][n] ints, and for K > 1 mahal[2][K][n][6] doubles (2 * K * 52 bytes a point)
  const size_t K = (size_t)h->voxel_nbr;
  for (int i = 0; i < 2; ++i) {
    h->vox_corr[i].ensure(K * n * sizeof(int));
    if (K > 1) h->vox_mahal[i].ensure(K * n * 6 * sizeof(double));
  }
  VoxelPassArgs& a = v.pa;
  a.src = S.pts();
  a.cov_src = covs_for(h, h->src_covs, h->src.dev);
  a.n_src = (int)n;
  a.table = h->vmap.table.as<ulonglong2>();
  a.mask = h->vmap.mask;
  a.rec = h->vmap.rec.as<double>();
  a.n_vox = (int)h->vmap.n_vox;
  a.inv_res = 1.0f / (float)h->voxel_res;
  for (int i = 0; i < 2; ++i) {
    a.corr[i] = h->vox_corr[i].as<int>();
    a.mahal[i] = K > 1 ? h->vox_mahal[i].as<double>() : h->mahal[i].as<double>();
  }
  a.nbr = (int)K;
  a.slot_stride = (int)n;
  a.st = h->state.as<LmState>();
  a.partials = h->partials.as<double>();
  a.mode = 3;
  a.t_first = nullptr;
  v.sa = c.sa;
  v.sa.partials = a.partials;
  v.sa.nblocks = nblocks;
  v.sa.grp_order = nullptr;  // (the solver sorts nothing)
  v.sa.grp_cost = nullptr;
  v.sa.order_valid = nullptr;
  v.nblocks = nblocks;
}

// do_align for a voxelized target: the same loop - state upload, (pass, solve) pairs fed `chunk_pairs` ahead of the solver's published
// progress, the final state read from pinned memory - with k_vgicp_pass in k_gicp_pass's place.  None of the exact path's kernel-variant
// switches applies.
void do_align_voxel(ngicp* h, const float guess[16], float* aligned, size_t out_stride) {
  const double t_begin = now_ms();
  h->hook_valid = 0;
  h->converged = 0;
  h->nr_iterations = 0;
  const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::memcpy(h->final_T, I, sizeof(I));
  VoxelCtx c;
  prepare_voxel_loop(h, c);
  LmState st;
  init_state_from_pose(st, pose_from_colmajor_f(guess));
  c.pa.mode = (h->p.optimizer == NGICP_OPT_GAUSS_NEWTON) ? 2 : 3;
  if (h->p.max_iter <= 0) st.hot.done = 1;
  h->pin_state[0] = st;
  HIP_TRY(hipMemcpyAsync(h->state.p, &h->pin_state[0], sizeof(st), hipMemcpyHostToDevice, h->stream));
  const long max_passes = (h->p.optimizer == NGICP_OPT_GAUSS_NEWTON) ? (long)h->p.max_iter : (long)h->p.max_iter * std::max(1, h->p.lm_max_iter) + 1;
  const int depth = h->chunk_pairs;
  *h->h_progress = 0;
  c.sa.progress_host = h->h_progress;
  c.sa.final_host = h->pin_final;
  c.sa.t_first = h->t_first.as<unsigned long long>();
  c.pa.t_first = h->t_first.as<unsigned long long>();
  long launched = 0;
  const bool finished = (h->p.max_iter <= 0);
  const double t_loop = now_ms();
  unsigned long spins = 0;
  while (!finished && launched < max_passes) {
    const int prog = *reinterpret_cast<volatile int*>(h->h_progress);
    if (prog & kProgressDone) break;
    if (launched - (long)(prog & kProgressMask) >= depth) {
      wait_for_the_loop(h, spins, t_loop);
      continue;
    }
    const bool timed = h->profiling && launched % h->prof_stride == h->prof_stride / 2 && (size_t)(2 * launched + 1) < h->prof_events.size();
    launch_voxel_pass(h, c, timed ? h->prof_events[2 * launched] : nullptr, timed ? h->prof_events[2 * launched + 1] : nullptr);
    hipLaunchKernelGGL(k_lm_solve, dim3(1), dim3(kSolveThreads), 0, h->stream, c.sa);
    ++launched;
  }
  float loop_ms = 0.f;
  if (finished) {
    HIP_TRY(hipStreamSynchronize(h->stream));
  } else {
    for (;;) {
      const int prog = __atomic_load_n(h->h_progress, __ATOMIC_ACQUIRE);
      if (prog & kProgressDone) break;
      if (launched >= max_passes && launched - (long)(prog & kProgressMask) <= 0) break;
      wait_for_the_loop(h, spins, t_loop);
    }
    st.hot = *h->pin_final;
    loop_ms = (float)((double)(st.hot.t_done - st.hot.t_first) * 1e-5);
  }
  HIP_TRY(hipGetLastError());
  publish_alignment(h, st, loop_ms, aligned, out_stride);  // (mean_candidates: this mode tests no target point, it counts the hash-table slots looked at)
  ngicp_stats& s = h->stats;
  s.staged_fraction = 0.0;
  sum_event_pass_times(h, st.hot.passes);
  s.n_src = (long long)h->src.dev->n;
  s.n_tgt = (long long)h->tgt.dev->n;
  s.host_wait_spins = (long long)spins;
  s.align_ms = now_ms() - t_begin;
}

// ------------------------------------------------------------------------------------------
// Batched registration: several initial guesses on one source / target pair
// ------------------------------------------------------------------------------------------
size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

void ensure_batch_pinned(ngicp* h) {
  BatchWs& w = h->batch;
  if (!w.pin_recs) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&w.pin_recs), (size_t)kBatchMaxLanes * (sizeof(LmState) + sizeof(PassArgs) + sizeof(SolveArgs)), hipHostMallocDefault));
  if (!w.pin_progress) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&w.pin_progress), (size_t)kBatchMaxLanes * BatchWs::kProgressStride * sizeof(int), hipHostMallocDefault));
  if (!w.pin_final) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&w.pin_final), (size_t)kBatchMaxLanes * sizeof(LmHot), hipHostMallocDefault));
}

// The feeding loop of a batch, shared by ngicp_align_batch and ngicp_voxel_align_batch: the lane records are on the device, every
// lane's progress word in pinned memory is 0; launch_pass_batch(bl, n_live) enqueues one pass launch that serves the n_live lanes listed
// in bl.lane, and one k_lm_solve_batch launch behind it steps their optimisers.  result[g]: lane g's final state image.
template <class LaunchPass>
void feed_batch(ngicp* h, int B, BatchLaunch& bl, long max_passes, std::vector<LmHot>& result, LaunchPass&& launch_pass_batch) {
  BatchWs& w = h->batch;
  // The feeding discipline of do_align: (pass, solve) pairs kept `depth` ahead of the slowest live lane's progress word.  A lane that
  // reports done leaves the list; its blocks in the launches already enqueued return at their head.
  const int depth = h->chunk_pairs;
  const double t_loop = now_ms();
  unsigned long spins = 0;
  bool idle_seen = false;
  // Every so many polls the stream is asked for its status: an asynchronous error comes out as its HIP error, not as the timeout.
  // true: the stream has nothing left to run.
  auto look_at_stream = [&]() -> bool {
    const hipError_t q = hipStreamQuery(h->stream);
    if (q == hipErrorNotReady) {
      (void)hipGetLastError();
    } else if (q != hipSuccess) {
      throw HipError{q, "hipStreamQuery(h->stream)", __FILE__, __LINE__};
    }
    if (now_ms() - t_loop > 30000.0) throw ArgError{NGICP_ERR_HIP, "the batched registration loop did not finish within 30 s"};
    return q == hipSuccess;
  };
  auto relax = [&]() {
    // (idle at the last look: every launch enqueued had run, so the words the caller has just read again were final)
    if (idle_seen) throw ArgError{NGICP_ERR_HIP, "the batched registration loop: the stream is idle but a lane has not reported"};
    if ((++spins & (h->host_wait ? 0xff : 0xfff)) == 0 && look_at_stream()) {
      idle_seen = true;
      return;
    }
    if (h->host_wait) sched_yield(); else __builtin_ia32_pause();
  };
  long launched = 0;
  int n_live = B;
  std::vector<int> live((size_t)B);
  for (int g = 0; g < B; ++g) live[(size_t)g] = g;
  for (;;) {
    long min_prog = std::numeric_limits<long>::max();
    int keep_n = 0;
    for (int i = 0; i < n_live; ++i) {
      const int g = live[(size_t)i];
      const int prog = __atomic_load_n(w.pin_progress + (size_t)g * BatchWs::kProgressStride, __ATOMIC_ACQUIRE);
      if (prog & kProgressDone) {
        result[(size_t)g] = w.pin_final[g];  // (stored before the flag: lm_solve_body)
        continue;
      }
      live[(size_t)keep_n++] = g;
      min_prog = std::min(min_prog, (long)(prog & kProgressMask));
    }
    n_live = keep_n;
    if (n_live == 0) break;
    if (launched >= max_passes || launched - min_prog >= depth) {  // enough in flight (or nothing left to launch: the last possible pass sets done)
      relax();
      continue;
    }
    idle_seen = false;
    for (int i = 0; i < n_live; ++i) bl.lane[i] = live[(size_t)i];
    launch_pass_batch(bl, n_live);
    hipLaunchKernelGGL(k_lm_solve_batch, dim3((unsigned)n_live), dim3(kSolveThreads), 0, h->stream, bl);
    ++launched;
  }
}

// every lane's final state into the caller's arrays, and the description of the traces ngicp_batch_get_lm_trace serves
void return_batch_results(ngicp* h, const std::vector<LmHot>& result, size_t trace_stride, float* T_out, int* converged, int* nr_iterations, double* hessians) {
  BatchWs& w = h->batch;
  for (size_t g = 0; g < result.size(); ++g) {
    const LmHot& r = result[g];
    pose_to_colmajor_f(r.x0, T_out + g * 16);
    if (converged) converged[g] = r.converged;
    if (nr_iterations) nr_iterations[g] = r.nr_iterations;
    if (hessians)
      for (int rr = 0; rr < 6; ++rr)
        for (int cc = 0; cc < 6; ++cc) hessians[g * 36 + cc * 6 + rr] = r.final_H[rr * 6 + cc];
    if (r.lm_failed) std::fprintf(stderr, "lm not converged!!\n");  // impl/lsq_registration_impl.hpp:106
    w.trace_rows.push_back((size_t)r.n_trace);
  }
  w.lanes = (int)result.size();
  w.trace_stride = trace_stride;
}

// The batch always takes the default route: walks in global memory (k_gicp_pass_batch), a solver launch of its own (k_lm_solve_batch).
// NGICP_PERSIST, NGICP_HEAD, NGICP_FUSED, NGICP_QUEUE, NGICP_PASS_IMPL and NGICP_ORDER do not apply to it.
void do_align_batch(ngicp* h, int B, const float* guesses, float* T_out, int* converged, int* nr_iterations, double* hessians) {
  BatchWs& w = h->batch;
  const int max_rows = std::max(1, h->p.max_iter) * std::max(1, h->p.lm_max_iter) + 1;
  // (slots, lazy covariances, the shared fields - and none of the handle's single-alignment buffers: what the getters of the last
  // ngicp_align read is neither resized nor written)
  LoopCtx c;
  prepare_loop(h, c, false);
  c.pa.mode = (h->p.optimizer == NGICP_OPT_GAUSS_NEWTON) ? 2 : 3;
  if (h->prev_staged_fraction < 0.0 || h->prev_staged_fraction >= 0.12) c.pa.mode |= 32;  // (the decision an align on this handle would take now: do_align)

  const size_t n = h->src.dev->n;
  const int nblocks = c.nblocks, n_batches = c.pa.n_batches;
  const size_t tpt_stride = round_up(n * sizeof(float4), 256), mahal_stride = round_up(n * 6 * sizeof(double), 256);
  const size_t part_stride = (size_t)nblocks * kNumSlots * sizeof(double);
  const size_t ord_stride = round_up((size_t)nblocks * sizeof(int), 256), far_stride = round_up((size_t)n_batches + 16, 256);
  const size_t trace_stride = (size_t)max_rows * kTraceCols;
  const size_t off_pass = (size_t)B * sizeof(LmState), off_solve = off_pass + round_up((size_t)B * sizeof(PassArgs), 16);
  const size_t recs_bytes = off_solve + (size_t)B * sizeof(SolveArgs);
  w.lanes = 0;  // (the traces of the previous call go with the buffers)
  w.trace_rows.clear();
  // (a call that fails half way - an allocation, say - must not leave a description of launch orders that a replaced buffer no longer holds)
  const bool order_described = w.order_src == h->src.dev.get() && w.order_groups == nblocks && w.order_lanes >= B;
  const int lanes_before = w.order_lanes;
  w.order_src = nullptr;
  w.order_lanes = 0;
  ensure_batch_pinned(h);
  w.recs.ensure(recs_bytes);
  w.tpt.ensure((size_t)B * 2 * tpt_stride);
  w.mahal.ensure((size_t)B * 2 * mahal_stride);
  w.partials.ensure((size_t)B * part_stride);
  bool order_kept = order_described;
  if (w.order.ensure_grew((size_t)B * ord_stride)) order_kept = false;
  w.cost.ensure((size_t)B * ord_stride);
  if (w.flags.ensure_grew((size_t)kBatchMaxLanes * 4 * sizeof(int))) order_kept = false;
  if (w.far.ensure_grew((size_t)B * far_stride)) HIP_TRY(hipMemsetAsync(w.far.p, 0, w.far.cap, h->stream));
  w.trace.ensure((size_t)B * trace_stride * sizeof(double));
  // a lane's launch order of the previous call is still a good guess when the source index is the same one (do_align)
  if (!order_kept) HIP_TRY(hipMemsetAsync(w.flags.p, 0, (size_t)kBatchMaxLanes * 4 * sizeof(int), h->stream));

  // ---- the lane records: state image, pass arguments, solver arguments ----
  LmState* const st_host = reinterpret_cast<LmState*>(w.pin_recs);
  PassArgs* const pa_host = reinterpret_cast<PassArgs*>(w.pin_recs + off_pass);
  SolveArgs* const sa_host = reinterpret_cast<SolveArgs*>(w.pin_recs + off_solve);
  unsigned char* const recs_dev = w.recs.as<unsigned char>();
  for (int g = 0; g < B; ++g) {
    init_state_from_pose(st_host[g], pose_from_colmajor_f(guesses + (size_t)g * 16));
    if (h->p.max_iter <= 0) st_host[g].hot.done = 1;
    PassArgs pa = c.pa;
    pa.st = reinterpret_cast<LmState*>(recs_dev) + g;
    for (int i = 0; i < 2; ++i) {
      pa.tpt[i] = reinterpret_cast<float4*>(w.tpt.as<unsigned char>() + ((size_t)g * 2 + i) * tpt_stride);
      pa.mahal[i] = reinterpret_cast<double*>(w.mahal.as<unsigned char>() + ((size_t)g * 2 + i) * mahal_stride);
    }
    pa.partials = reinterpret_cast<double*>(w.partials.as<unsigned char>() + (size_t)g * part_stride);
    pa.grp_order = reinterpret_cast<int*>(w.order.as<unsigned char>() + (size_t)g * ord_stride);
    pa.grp_cost = reinterpret_cast<int*>(w.cost.as<unsigned char>() + (size_t)g * ord_stride);
    pa.batch_far = w.far.as<unsigned char>() + (size_t)g * far_stride;
    pa.order_valid = w.flags.as<int>() + (size_t)g * 4;
    pa.ticket = w.flags.as<int>() + (size_t)g * 4 + 1;
    pa.t_first = nullptr;
    SolveArgs sa = c.sa;
    sa.st = pa.st;
    sa.partials = pa.partials;
    sa.grp_order = const_cast<int*>(pa.grp_order);
    sa.grp_cost = pa.grp_cost;
    sa.trace = w.trace.as<double>() + (size_t)g * trace_stride;
    sa.progress_host = w.pin_progress + (size_t)g * BatchWs::kProgressStride;
    sa.final_host = w.pin_final + g;
    sa.order_valid = const_cast<int*>(pa.order_valid);
    sa.t_first = nullptr;
    pa.sa = sa;
    pa_host[g] = pa;
    sa_host[g] = sa;
    *sa.progress_host = 0;
  }
  const long max_passes = (h->p.optimizer == NGICP_OPT_GAUSS_NEWTON) ? (long)h->p.max_iter : (long)h->p.max_iter * std::max(1, h->p.lm_max_iter) + 1;
  std::vector<LmHot> result((size_t)B);
  if (h->p.max_iter <= 0) {
    for (int g = 0; g < B; ++g) result[(size_t)g] = st_host[g].hot;  // every lane returns its guess, as ngicp_align does; nothing is launched
  } else {
    HIP_TRY(hipMemcpyAsync(recs_dev, w.pin_recs, recs_bytes, hipMemcpyHostToDevice, h->stream));  // ONE upload
    BatchLaunch bl;
    bl.pass = recs_dev + off_pass;
    bl.solve = reinterpret_cast<const SolveArgs*>(recs_dev + off_solve);
    for (int i = 0; i < kBatchMaxLanes; ++i) bl.lane[i] = 0;
    feed_batch(h, B, bl, max_passes, result, [&](const BatchLaunch& l, int n_live) {
      const bool four = (long)nblocks * n_live > 2L * h->pass_slots;  // launch_pass's rule on the whole grid
      if (four)
        hipLaunchKernelGGL((k_gicp_pass_batch<2, 4>), dim3((unsigned)nblocks, (unsigned)n_live), dim3(256), 0, h->stream, l);
      else
        hipLaunchKernelGGL((k_gicp_pass_batch<2, 3>), dim3((unsigned)nblocks, (unsigned)n_live), dim3(256), 0, h->stream, l);
    });
    HIP_TRY(hipGetLastError());
  }
  return_batch_results(h, result, trace_stride, T_out, converged, nr_iterations, hessians);
  w.order_src = h->src.dev.get();
  w.order_groups = nblocks;
  w.order_lanes = std::max(order_kept ? lanes_before : 0, B);
}

// ngicp_voxel_align_batch: do_align_batch's protocol - the lane records in one pinned block and one upload, a progress
// word and a final image per lane in pinned memory, the live lanes in the kernel arguments, feed_batch - with k_vgicp_pass_batch<K> in
// k_gicp_pass_batch's place and the solver's records as prepare_voxel_loop sets them (no launch order).  Every per-lane buffer is the
// batch's own: vox_corr / vox_mahal / mahal / state / partials / trace of the handle, which the getters of the last ngicp_align read,
// are neither resized nor written.  None of the exact path's kernel-variant switches applies.
void do_align_voxel_batch(ngicp* h, int B, const float* guesses, float* T_out, int* converged, int* nr_iterations, double* hessians) {
  static_assert(sizeof(VoxelPassArgs) <= sizeof(PassArgs), "the pinned record block is sized for PassArgs records");
  BatchWs& w = h->batch;
  const int max_rows = std::max(1, h->p.max_iter) * std::max(1, h->p.lm_max_iter) + 1;
  LoopCtx c;
  prepare_loop(h, c, false);  // (slots, lazy covariances, the solver's configuration)
  ensure_voxel_map(h);        // (at most one build, whatever the number of lanes)
  const size_t n = h->src.dev->n, K = (size_t)h->voxel_nbr;
  const int nblocks = std::max(1, (int)((n + kVoxBlock - 1) / kVoxBlock));
  const size_t corr_stride = round_up(K * n * sizeof(int), 256), mahal_stride = round_up(K * n * 6 * sizeof(double), 256);
  const size_t part_stride = (size_t)nblocks * kNumSlots * sizeof(double);
  const size_t trace_stride = (size_t)max_rows * kTraceCols;
  const size_t off_pass = (size_t)B * sizeof(LmState), off_solve = off_pass + round_up((size_t)B * sizeof(VoxelPassArgs), 16);
  const size_t recs_bytes = off_solve + (size_t)B * sizeof(SolveArgs);
  w.lanes = 0;  // (the traces of the previous call go with the buffers)
  w.trace_rows.clear();
  // (every buffer is sized before the first launch: growing one frees it, and freeing waits for the device)
  ensure_batch_pinned(h);
  w.recs.ensure(recs_bytes);
  w.vox_corr.ensure((size_t)B * 2 * corr_stride);
  w.vox_mahal.ensure((size_t)B * 2 * mahal_stride);
  w.partials.ensure((size_t)B * part_stride);
  w.trace.ensure((size_t)B * trace_stride * sizeof(double));

  LmState* const st_host = reinterpret_cast<LmState*>(w.pin_recs);
  VoxelPassArgs* const pa_host = reinterpret_cast<VoxelPassArgs*>(w.pin_recs + off_pass);
  SolveArgs* const sa_host = reinterpret_cast<SolveArgs*>(w.pin_recs + off_solve);
  unsigned char* const recs_dev = w.recs.as<unsigned char>();
  VoxelPassArgs shared;
  shared.src = h->src.dev->pts();
  shared.cov_src = c.pa.cov_src;
  shared.n_src = (int)n;
  shared.table = h->vmap.table.as<ulonglong2>();
  shared.mask = h->vmap.mask;
  shared.rec = h->vmap.rec.as<double>();
  shared.n_vox = (int)h->vmap.n_vox;
  shared.inv_res = 1.0f / (float)h->voxel_res;
  shared.mode = (h->p.optimizer == NGICP_OPT_GAUSS_NEWTON) ? 2 : 3;
  shared.t_first = nullptr;
  shared.nbr = (int)K;
  shared.slot_stride = (int)n;
  for (int g = 0; g < B; ++g) {
    init_state_from_pose(st_host[g], pose_from_colmajor_f(guesses + (size_t)g * 16));
    if (h->p.max_iter <= 0) st_host[g].hot.done = 1;
    VoxelPassArgs pa = shared;
    pa.st = reinterpret_cast<LmState*>(recs_dev) + g;
    for (int i = 0; i < 2; ++i) {
      pa.corr[i] = reinterpret_cast<int*>(w.vox_corr.as<unsigned char>() + ((size_t)g * 2 + i) * corr_stride);
      pa.mahal[i] = reinterpret_cast<double*>(w.vox_mahal.as<unsigned char>() + ((size_t)g * 2 + i) * mahal_stride);
    }
    pa.partials = reinterpret_cast<double*>(w.partials.as<unsigned char>() + (size_t)g * part_stride);
    SolveArgs sa = c.sa;
    sa.st = pa.st;
    sa.partials = pa.partials;
    sa.nblocks = nblocks;
    sa.grp_order = nullptr;  // (the solver sorts nothing: prepare_voxel_loop)
    sa.grp_cost = nullptr;
    sa.order_valid = nullptr;
    sa.trace = w.trace.as<double>() + (size_t)g * trace_stride;
    sa.progress_host = w.pin_progress + (size_t)g * BatchWs::kProgressStride;
    sa.final_host = w.pin_final + g;
    sa.t_first = nullptr;
    pa_host[g] = pa;
    sa_host[g] = sa;
    *sa.progress_host = 0;
  }
  const long max_passes = (h->p.optimizer == NGICP_OPT_GAUSS_NEWTON) ? (long)h->p.max_iter : (long)h->p.max_iter * std::max(1, h->p.lm_max_iter) + 1;
  std::vector<LmHot> result((size_t)B);
  if (h->p.max_iter <= 0) {
    for (int g = 0; g < B; ++g) result[(size_t)g] = st_host[g].hot;  // every lane returns its guess, as ngicp_align does; nothing is launched
  } else {
    HIP_TRY(hipMemcpyAsync(recs_dev, w.pin_recs, recs_bytes, hipMemcpyHostToDevice, h->stream));  // ONE upload
    BatchLaunch bl;
    bl.pass = recs_dev + off_pass;
    bl.solve = reinterpret_cast<const SolveArgs*>(recs_dev + off_solve);
    for (int i = 0; i < kBatchMaxLanes; ++i) bl.lane[i] = 0;
    feed_batch(h, B, bl, max_passes, result, [&](const BatchLaunch& l, int n_live) {
      const dim3 grid((unsigned)nblocks, (unsigned)n_live), block(kVoxBlock);
      switch ((int)K) {
        case NGICP_VOX_DIRECT1: hipLaunchKernelGGL(k_vgicp_pass_batch<1>, grid, block, 0, h->stream, l); break;
        case NGICP_VOX_DIRECT7: hipLaunchKernelGGL(k_vgicp_pass_batch<7>, grid, block, 0, h->stream, l); break;
        case NGICP_VOX_DIRECT27: hipLaunchKernelGGL(k_vgicp_pass_batch<27>, grid, block, 0, h->stream, l); break;
        default: throw ArgError{NGICP_ERR_STATE, "voxelized GICP: unknown neighbourhood"};
      }
    });
    HIP_TRY(hipGetLastError());
  }
  return_batch_results(h, result, trace_stride, T_out, converged, nr_iterations, hessians);
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

int set_cloud(ngicp* h, Slot& slot, const float* xyz, size_t n, size_t stride, uint64_t identity, bool build_now) {
  return guarded(h, [&] {
    if (!xyz && n) throw ArgError{NGICP_ERR_ARG, "null cloud pointer"};
    if (identity != 0 && slot.present && slot.identity == identity) return;  // pointer-identity early-out
    slot.clear();
    slot.present = true;
    slot.host = xyz;
    slot.n = n;
    slot.stride = stride;
    slot.identity = identity;
    if (build_now) {
      try {
        slot.dev = upload_and_index(h, xyz, n, stride);
      } catch (...) {
        slot.clear();  // a rejected cloud leaves the slot empty
        throw;
      }
    }
  });
}

// ---- queries on the indexed clouds (ngicp_query.h) ----
// which: 0 = source, 1 = target (as ngicp_covs_shard_*); the slot's cloud is uploaded and indexed if it was only registered
DeviceCloud& query_cloud(ngicp* h, int which) {
  Slot& s = which ? h->tgt : h->src;
  ensure_slot_ready(h, s, which ? "target" : "source");
  return *s.dev;
}
void check_which(int which) {
  if (which != 0 && which != 1) throw ArgError{NGICP_ERR_ARG, "which must be 0 (source) or 1 (target)"};
}

// strided host points -> h->queries (float4 {x, y, z, 1})
void upload_queries(ngicp* h, const float* q, size_t nq, size_t stride) {
  std::vector<float> packed(nq * 4);
  for (size_t i = 0; i < nq; ++i) {
    const float* p = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(q) + i * stride);
    packed[i * 4 + 0] = p[0];
    packed[i * 4 + 1] = p[1];
    packed[i * 4 + 2] = p[2];
    packed[i * 4 + 3] = 1.f;
  }
  h->queries.ensure(nq * sizeof(float4));
  HIP_TRY(hipMemcpyAsync(h->queries.p, packed.data(), nq * sizeof(float4), hipMemcpyHostToDevice, h->stream));
}

void query_timing_done(ngicp* h) {  // after the stream has been synchronised behind ev_q_b
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->ev_q_a, h->ev_q_b));
  h->stats.query_ms = ms;
}

// KdTreeFLANN::nearestKSearch (include/nano_gicp/nanoflann.hpp:141-152) on either index
void knn_impl(ngicp* h, int which, const float* q, size_t nq, size_t stride, int k, int* idx, float* d2) {
  check_which(which);
  if (!q || !idx || !d2) throw ArgError{NGICP_ERR_ARG, "null pointer"};
  if (nq == 0) return;
  if (stride < 12 || stride % 4) throw ArgError{NGICP_ERR_ARG, "bad stride"};
  DeviceCloud& T = query_cloud(h, which);
  if (k <= 0) throw ArgError{NGICP_ERR_ARG, "k must be positive"};
  if (k > 32 || (size_t)k > T.n) throw ArgError{NGICP_ERR_K_TOO_LARGE, "k exceeds the cloud size or the engine limit of 32"};
  upload_queries(h, q, nq, stride);
  h->knn_idx.ensure(nq * k * sizeof(int));
  h->knn_d2.ensure(nq * k * sizeof(float));
  const dim3 grid((unsigned)((nq + kKnnPairs - 1) / kKnnPairs)), block(kKnnBlock);  // a pair of lanes per query
  HIP_TRY(hipEventRecord(h->ev_q_a, h->stream));
  if (k <= 10)
    hipLaunchKernelGGL(k_knn_queries<10>, grid, block, 0, h->stream, T.pts(), T.cells(), T.grid, h->queries.as<float4>(), (int)nq, k,
                       h->knn_idx.as<int>(), h->knn_d2.as<float>());
  else if (k <= 20)
    hipLaunchKernelGGL(k_knn_queries<20>, grid, block, 0, h->stream, T.pts(), T.cells(), T.grid, h->queries.as<float4>(), (int)nq, k,
                       h->knn_idx.as<int>(), h->knn_d2.as<float>());
  else
    hipLaunchKernelGGL(k_knn_queries<32>, grid, block, 0, h->stream, T.pts(), T.cells(), T.grid, h->queries.as<float4>(), (int)nq, k,
                       h->knn_idx.as<int>(), h->knn_d2.as<float>());
  HIP_TRY(hipEventRecord(h->ev_q_b, h->stream));
  HIP_TRY(hipMemcpyAsync(idx, h->knn_idx.p, nq * k * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(d2, h->knn_d2.p, nq * k * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  query_timing_done(h);
}

// ---- range select (ngicp_range.h) ----
// which: 0 = source, 1 = target, 2 = the preprocessed scan still on the device.  median: rank = n / 2.
void range_select_impl(ngicp* h, int which, size_t rank, bool median, float* value, size_t* n_out) {
  if (!value) throw ArgError{NGICP_ERR_ARG, "null output"};
  if (which < 0 || which > 2) throw ArgError{NGICP_ERR_ARG, "which must be 0 (source), 1 (target) or 2 (preprocessed scan)"};
  const float4* pts = nullptr;
  size_t n = 0;
  if (which == 2) {
    if (!h->filt_out || h->filt_n <= 0) throw ArgError{NGICP_ERR_STATE, "no preprocessed cloud: call ngicp_preprocess_scan first"};
    pts = h->filt_out;
    n = (size_t)h->filt_n;
  } else {
    DeviceCloud& C = query_cloud(h, which);
    pts = C.pts();  // the real points: the sentinel frame lies outside [pts, pts + n)
    n = C.n;
  }
  if (n == 0) throw ArgError{NGICP_ERR_STATE, "the cloud is empty"};
  if (n > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "cloud too large for int counters"};
  if (n_out) *n_out = n;
  if (median) rank = n / 2;
  if (rank >= n) throw ArgError{NGICP_ERR_ARG, "rank must be below the number of points"};
  constexpr size_t kHistBytes = 3 * kRangeBins * sizeof(int);
  h->range_ws.ensure(kHistBytes + sizeof(RangeRec));
  int* hist = h->range_ws.as<int>();
  RangeRec* rec = reinterpret_cast<RangeRec*>(h->range_ws.as<unsigned char>() + kHistBytes);
  const int blocks = pick_blocks(n, 4 * kRangeBlock, kRangeMaxBlocks);
  HIP_TRY(hipEventRecord(h->ev_q_a, h->stream));
  HIP_TRY(hipMemsetAsync(hist, 0, kHistBytes, h->stream));
  for (int round = 0; round < 3; ++round) {
    hipLaunchKernelGGL(k_range_hist, dim3(blocks), dim3(kRangeBlock), 0, h->stream, pts, (int)n, round, (const RangeRec*)rec, hist + round * kRangeBins);
    hipLaunchKernelGGL(k_range_pick, dim3(1), dim3(kRangeBlock), 0, h->stream, (const int*)(hist + round * kRangeBins), round, (int)rank, rec);
  }
  HIP_TRY(hipEventRecord(h->ev_q_b, h->stream));
  unsigned int bits = 0;
  HIP_TRY(hipMemcpyAsync(&bits, &rec->value, sizeof(bits), hipMemcpyDeviceToHost, h->stream));  // the one read-back
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  query_timing_done(h);
  std::memcpy(value, &bits, sizeof(bits));
}

}  // namespace

// =============================================================================================
extern "C" {

const char* ngicp_version(void) { return "ngicp-hip 0.1 (gfx950)"; }

int ngicp_create(int device, ngicp_t** out) {
  if (!out) return NGICP_ERR_ARG;
  *out = nullptr;
  try {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
      g_create_error = std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
      (void)hipGetLastError();
      return NGICP_ERR_HIP;
    }
    if (device < 0 || device >= count) {
      g_create_error = "device index out of range";
      return NGICP_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<ngicp> h(new ngicp);
    h->device = device;
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&h->ev_a));
    HIP_TRY(hipEventCreate(&h->ev_b));
    HIP_TRY(hipEventCreate(&h->ev_cov_a));
    HIP_TRY(hipEventCreate(&h->ev_cov_b));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_fence, hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&h->ev_q_a));
    HIP_TRY(hipEventCreate(&h->ev_q_b));
    HIP_TRY(hipEventCreate(&h->ev_vox_a));
    HIP_TRY(hipEventCreate(&h->ev_vox_b));
    HIP_TRY(hipEventCreate(&h->ev_vox_c));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->pin_state), 2 * sizeof(LmState), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->pin_final), sizeof(LmHot), hipHostMallocDefault));
    h->order_flag.ensure(64);
    h->t_first.ensure(64);
    HIP_TRY(hipMemset(h->order_flag.p, 0, 64));
    HIP_TRY(hipMemset(h->t_first.p, 0, 64));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->h_progress), sizeof(int), hipHostMallocDefault));
    *h->h_progress = 0;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->h_shard_done), kShardSlots * sizeof(int), hipHostMallocDefault));
    for (int i = 0; i < kShardSlots; ++i) {
      h->h_shard_done[i] = 0;
      HIP_TRY(hipEventCreateWithFlags(&h->ev_shard[i], hipEventDisableTiming));
    }
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(h->final_T, I, sizeof(I));
    std::memset(h->final_hessian, 0, sizeof(h->final_hessian));
    for (int i = 0; i < 6; ++i) h->final_hessian[i * 6 + i] = 1.0;  // impl/lsq_registration_impl.hpp:62
    {
      int cus = 0, per_cu = 0;
      HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_gicp_pass<2, 3>, 256, 0));
      h->pass_slots = std::max(1, cus) * std::max(1, per_cu);
      int per_cu_p = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_p, k_gicp_persist<2, 3>, 256, 0) == hipSuccess) h->persist_slots = std::max(0, cus) * std::max(0, per_cu_p);
      int q3 = 0, q4 = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&q3, k_gicp_queue<2, 3>, 256, 0) == hipSuccess && q3 > 0) h->queue_slots[0] = cus * q3;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&q4, k_gicp_queue<2, 4>, 256, 0) == hipSuccess && q4 > 0) h->queue_slots[1] = cus * q4;
      int coop = 0;
      if (hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, device) != hipSuccess || !coop) h->persist_slots = 0;
    }
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->pin_ticks), 2 * kMaxTickPasses * sizeof(unsigned long long), hipHostMallocDefault));
    if (const char* s = std::getenv("NGICP_PERSIST")) h->persist = std::atoi(s);
    if (const char* s = std::getenv("NGICP_HEAD")) h->head = std::atoi(s);
    if (const char* s = std::getenv("NGICP_CELL_BOXES")) h->cell_boxes = std::atoi(s);
    if (const char* s = std::getenv("NGICP_TARGET_OCC")) h->target_occupancy = std::max(1.0, std::atof(s));
    if (const char* s = std::getenv("NGICP_VOXEL")) h->voxel_size = std::atof(s);
    if (const char* s = std::getenv("NGICP_CHUNK")) h->chunk_pairs = std::max(1, std::min(64, std::atoi(s)));
    if (const char* s = std::getenv("NGICP_STAGE_GROW")) h->stage_grow = std::max(0, std::min(kStageMaxGrow, std::atoi(s)));
    {
      HandleRegistry& r = registry();
      std::lock_guard<std::mutex> lock(r.m);
      r.live.push_back(h.get());
    }
    *out = h.release();
    return NGICP_OK;
  } catch (const HipError& e) {
    g_create_error = std::string("HIP error in ") + e.what + ": " + hipGetErrorString(e.code);
    (void)hipGetLastError();
    return NGICP_ERR_HIP;
  } catch (...) {
    g_create_error = "unknown error";
    return NGICP_ERR_ARG;
  }
}

int ngicp_destroy(ngicp_t* h) {
  if (!h) return NGICP_OK;
  {
    HandleRegistry& r = registry();
    std::lock_guard<std::mutex> lock(r.m);
    r.live.erase(std::remove(r.live.begin(), r.live.end(), h), r.live.end());
  }
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->src.clear();
  h->tgt.clear();
  h->src_covs.clear();
  h->tgt_covs.clear();
  for (auto& e : h->prof_events)
    if (e) (void)hipEventDestroy(e);
  if (h->pin_state) (void)hipHostFree(h->pin_state);
  if (h->pin_final) (void)hipHostFree(h->pin_final);
  if (h->pin_ticks) (void)hipHostFree(h->pin_ticks);
  if (h->h_progress) (void)hipHostFree(h->h_progress);
  if (h->h_shard_done) (void)hipHostFree(h->h_shard_done);
  if (h->batch.pin_recs) (void)hipHostFree(h->batch.pin_recs);
  if (h->batch.pin_progress) (void)hipHostFree(h->batch.pin_progress);
  if (h->batch.pin_final) (void)hipHostFree(h->batch.pin_final);
  for (auto& e : h->ev_shard)
    if (e) (void)hipEventDestroy(e);
  if (h->ev_a) (void)hipEventDestroy(h->ev_a);
  if (h->ev_b) (void)hipEventDestroy(h->ev_b);
  if (h->ev_cov_a) (void)hipEventDestroy(h->ev_cov_a);
  if (h->ev_cov_b) (void)hipEventDestroy(h->ev_cov_b);
  if (h->ev_fence) (void)hipEventDestroy(h->ev_fence);
  if (h->ev_q_a) (void)hipEventDestroy(h->ev_q_a);
  if (h->ev_q_b) (void)hipEventDestroy(h->ev_q_b);
  if (h->ev_vox_a) (void)hipEventDestroy(h->ev_vox_a);
  if (h->ev_vox_b) (void)hipEventDestroy(h->ev_vox_b);
  if (h->ev_vox_c) (void)hipEventDestroy(h->ev_vox_c);
  h->vmap.invalidate();
  ngk_filter_free(&h->fws);
  ngk_filter_free(&h->vox_ws);
  hipStream_t s = h->stream;
  delete h;
  if (s) (void)hipStreamDestroy(s);
  return NGICP_OK;
}

const char* ngicp_last_error(const ngicp_t* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ngicp_set_params(ngicp_t* h, int k, double max_corr_dist, int max_iter, double trans_eps, double rot_eps, int optimizer, int lm_max_iter, double lm_init_lambda_factor,
                     int regularization, int num_threads) {
  return guarded(h, [&] {
    if (regularization < 0 || regularization > 4) throw ArgError{NGICP_ERR_ARG, "unknown regularization method"};
    if (optimizer != 0 && optimizer != 1) throw ArgError{NGICP_ERR_ARG, "unknown optimizer"};
    h->p.k = k;
    h->p.max_corr_dist = max_corr_dist;
    h->p.max_iter = max_iter;
    h->p.trans_eps = trans_eps;
    h->p.rot_eps = rot_eps;
    h->p.optimizer = optimizer;
    h->p.lm_max_iter = lm_max_iter;
    h->p.lm_init_lambda_factor = lm_init_lambda_factor;
    h->p.regularization = regularization;
    h->p.num_threads = num_threads;
  });
}

int ngicp_set_tuning(ngicp_t* h, double voxel_size, int lanes_per_query) {
  return guarded(h, [&] {
    if (voxel_size < 0) throw ArgError{NGICP_ERR_ARG, "voxel_size must be >= 0"};
    if (lanes_per_query != 0 && lanes_per_query != 1 && lanes_per_query != 2 && lanes_per_query != 4 && lanes_per_query != 8 && lanes_per_query != 16)
      throw ArgError{NGICP_ERR_ARG, "lanes_per_query must be 0,1,2,4,8 or 16"};
    h->voxel_size = voxel_size;
  });
}

int ngicp_set_source(ngicp_t* h, const float* xyz, size_t n, size_t stride_bytes, uint64_t id) {
  if (!h) return NGICP_ERR_ARG;
  const bool same = (id != 0 && h->src.present && h->src.identity == id);
  int rc = set_cloud(h, h->src, xyz, n, stride_bytes, id, true);
  if (rc == NGICP_OK && !same) h->src_covs.clear();  // impl/nano_gicp_impl.hpp:128
  return rc;
}
int ngicp_register_source(ngicp_t* h, const float* xyz, size_t n, size_t stride_bytes, uint64_t id) {
  if (!h) return NGICP_ERR_ARG;
  return set_cloud(h, h->src, xyz, n, stride_bytes, id, false);  // covariances untouched (impl/nano_gicp_impl.hpp:113-118)
}
int ngicp_set_target(ngicp_t* h, const float* xyz, size_t n, size_t stride_bytes, uint64_t id) {
  if (!h) return NGICP_ERR_ARG;
  const bool same = (id != 0 && h->tgt.present && h->tgt.identity == id);
  int rc = set_cloud(h, h->tgt, xyz, n, stride_bytes, id, true);
  if (rc == NGICP_OK && !same) h->tgt_covs.clear();  // :138
  if (!same) {  // the target is no longer the submap assembled by ngicp_submap_set (a recycled index object may reuse its address)
    h->submap_cloud = nullptr;
    h->submap_ids.clear();
    drop_voxel_map(h);
  }
  return rc;
}
int ngicp_clear_source(ngicp_t* h) {
  return guarded(h, [&] {
    h->src.clear();
    h->src_covs.clear();
  });
}
int ngicp_clear_target(ngicp_t* h) {
  return guarded(h, [&] {
    h->tgt.clear();
    h->tgt_covs.clear();
    h->submap_cloud = nullptr;
    h->submap_ids.clear();
    drop_voxel_map(h);
  });
}

int ngicp_share_source_index(ngicp_t* dst, ngicp_t* src) {
  if (!src) return NGICP_ERR_ARG;
  return guarded(dst, [&] {
    if (dst->device != src->device) return;  // different GPUs: dst uploads its own copy lazily
    if (!src->src.present || !src->src.dev) return;
    if (!dst->src.present) return;
    // adopt only when both refer to the same host cloud (the reference would otherwise rebuild the
    // tree for its own cloud at impl/nano_gicp_impl.hpp:304-306)
    const bool same = (dst->src.identity != 0 && dst->src.identity == src->src.identity) || (dst->src.host == src->src.host && dst->src.n == src->src.n);
    if (same) {
      // dst's stream waits (on the device) for the index build src has enqueued: no host synchronisation per scan
      HIP_TRY(hipEventRecord(dst->ev_fence, src->stream));
      HIP_TRY(hipStreamWaitEvent(dst->stream, dst->ev_fence, 0));
      dst->src.dev = src->src.dev;
    }
  });
}

int ngicp_swap_source_target(ngicp_t* h) {
  return guarded(h, [&] {
    std::swap(h->src, h->tgt);
    std::swap(h->src_covs, h->tgt_covs);
    h->hook_valid = 0;  // correspondences_.clear(); sq_distances_.clear();
    h->submap_cloud = nullptr;
    h->submap_ids.clear();
    drop_voxel_map(h);
  });
}

int ngicp_compute_source_covs(ngicp_t* h) {
  return guarded(h, [&] { compute_covs(h, h->src, h->src_covs, "source"); });
}
int ngicp_compute_target_covs(ngicp_t* h) {
  return guarded(h, [&] {
    drop_voxel_map(h);
    compute_covs(h, h->tgt, h->tgt_covs, "target");
  });
}

int ngicp_copy_source_covs(ngicp_t* dst, ngicp_t* src) {
  if (!src) return NGICP_ERR_ARG;
  return guarded(dst, [&] {
    if (src->src_covs.n == 0) {
      dst->src_covs.clear();
      return;
    }
    if (dst->device == src->device) {
      HIP_TRY(hipEventRecord(dst->ev_fence, src->stream));  // the covariance kernel / reorder src has enqueued
      HIP_TRY(hipStreamWaitEvent(dst->stream, dst->ev_fence, 0));
      dst->src_covs = src->src_covs;  // shares the immutable device buffer
    } else {
      throw ArgError{NGICP_ERR_ARG, "copy_source_covs across devices is not supported; use get/set"};
    }
  });
}
int ngicp_clear_source_covs(ngicp_t* h) {
  return guarded(h, [&] { h->src_covs.clear(); });
}
int ngicp_clear_target_covs(ngicp_t* h) {
  return guarded(h, [&] {
    h->tgt_covs.clear();
    drop_voxel_map(h);
  });
}
int ngicp_source_covs_size(const ngicp_t* h, size_t* n) {
  if (!h || !n) return NGICP_ERR_ARG;
  *n = h->src_covs.n;
  return NGICP_OK;
}
int ngicp_target_covs_size(const ngicp_t* h, size_t* n) {
  if (!h || !n) return NGICP_ERR_ARG;
  *n = h->tgt_covs.n;
  return NGICP_OK;
}
int ngicp_get_source_covs(ngicp_t* h, double* out) {
  return guarded(h, [&] {
    if (!out) throw ArgError{NGICP_ERR_ARG, "null output"};
    get_covs(h, h->src_covs, out);
  });
}
int ngicp_get_target_covs(ngicp_t* h, double* out) {
  return guarded(h, [&] {
    if (!out) throw ArgError{NGICP_ERR_ARG, "null output"};
    get_covs(h, h->tgt_covs, out);
  });
}
int ngicp_set_source_covs(ngicp_t* h, const double* in, size_t n) {
  return guarded(h, [&] { set_covs(h, h->src, h->src_covs, in, n, "source"); });
}
int ngicp_set_target_covs(ngicp_t* h, const double* in, size_t n) {
  return guarded(h, [&] {
    drop_voxel_map(h);
    set_covs(h, h->tgt, h->tgt_covs, in, n, "target");
  });
}

int ngicp_align(ngicp_t* h, const float guess[16], float T_out[16], int* converged, int* nr_iterations, double final_hessian[36], float* aligned, size_t out_stride_bytes) {
  int rc = guarded(h, [&] {
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (aligned && (out_stride_bytes < 12 || out_stride_bytes % 4)) throw ArgError{NGICP_ERR_ARG, "bad out_stride_bytes"};
    if (h->voxel_res > 0.0) do_align_voxel(h, guess ? guess : I, aligned, out_stride_bytes);
    else do_align(h, guess ? guess : I, aligned, out_stride_bytes);
  });
  if (h) {
    if (T_out) std::memcpy(T_out, h->final_T, sizeof(h->final_T));
    if (converged) *converged = h->converged;
    if (nr_iterations) *nr_iterations = h->nr_iterations;
    if (final_hessian) std::memcpy(final_hessian, h->final_hessian, sizeof(h->final_hessian));
  }
  return rc;
}

int ngicp_align_batch(ngicp_t* h, size_t n_guesses, const float* guesses, float* T_out, int* converged, int* nr_iterations, double* final_hessians) {
  return guarded(h, [&] {
    refuse_if_voxelized(h, "ngicp_align_batch");
    if (n_guesses == 0) throw ArgError{NGICP_ERR_ARG, "ngicp_align_batch: n_guesses is 0"};
    if (n_guesses > (size_t)NGICP_BATCH_MAX_LANES) throw ArgError{NGICP_ERR_ARG, "ngicp_align_batch: more than NGICP_BATCH_MAX_LANES (64) guesses in one call"};
    if (!guesses) throw ArgError{NGICP_ERR_ARG, "ngicp_align_batch: null guesses"};
    if (!T_out || !converged || !nr_iterations) throw ArgError{NGICP_ERR_ARG, "ngicp_align_batch: null output"};
    do_align_batch(h, (int)n_guesses, guesses, T_out, converged, nr_iterations, final_hessians);
  });
}

int ngicp_voxel_align_batch(ngicp_t* h, size_t n_guesses, const float* guesses, float* T_out, int* converged, int* nr_iterations, double* final_hessians) {
  return guarded(h, [&] {
    if (!(h->voxel_res > 0.0)) throw ArgError{NGICP_ERR_STATE, "ngicp_voxel_align_batch: the voxelized mode is off (ngicp_set_voxel_resolution)"};
    if (n_guesses == 0) throw ArgError{NGICP_ERR_ARG, "ngicp_voxel_align_batch: n_guesses is 0"};
    if (n_guesses > (size_t)NGICP_BATCH_MAX_LANES) throw ArgError{NGICP_ERR_ARG, "ngicp_voxel_align_batch: more than NGICP_BATCH_MAX_LANES (64) guesses in one call"};
    if (!guesses) throw ArgError{NGICP_ERR_ARG, "ngicp_voxel_align_batch: null guesses"};
    if (!T_out || !converged || !nr_iterations) throw ArgError{NGICP_ERR_ARG, "ngicp_voxel_align_batch: null output"};
    do_align_voxel_batch(h, (int)n_guesses, guesses, T_out, converged, nr_iterations, final_hessians);
  });
}

int ngicp_batch_get_lm_trace(ngicp_t* h, size_t lane, double* rows, size_t max_rows, size_t* n_rows) {
  return guarded(h, [&] {
    BatchWs& w = h->batch;
    if (lane >= (size_t)w.lanes) throw ArgError{NGICP_ERR_ARG, "ngicp_batch_get_lm_trace: no such lane in the last ngicp_align_batch / ngicp_voxel_align_batch"};
    const size_t n = w.trace_rows[lane];
    if (n_rows) *n_rows = n;
    const size_t take = std::min(n, max_rows);
    if (rows && take) {
      HIP_TRY(hipMemcpyAsync(rows, w.trace.as<double>() + lane * w.trace_stride, take * kTraceCols * sizeof(double), hipMemcpyDeviceToHost, h->stream));  // (stream order)
      HIP_TRY(hipStreamSynchronize(h->stream));
    }
  });
}

int ngicp_fitness_score_batch(ngicp_t* h, size_t n, const float* T_colmajor, double max_range, double* scores, size_t* n_inliers) {
  return guarded(h, [&] {
    if (n == 0) throw ArgError{NGICP_ERR_ARG, "ngicp_fitness_score_batch: n is 0"};
    if (!T_colmajor) throw ArgError{NGICP_ERR_ARG, "ngicp_fitness_score_batch: null transforms"};
    if (!scores) throw ArgError{NGICP_ERR_ARG, "null output"};
    DeviceCloud& S = query_cloud(h, 0);
    DeviceCloud& T = query_cloud(h, 1);
    BatchWs& w = h->batch;
    const int np = (int)S.n;
    const int nb = (np + kKnnPairs - 1) / kKnnPairs;
    std::vector<double2> r(n);
    // (any number of transforms: the lane dimension of a launch is cut at the grid's limit)
    constexpr size_t kChunk = 4096;
    const size_t chunk = std::min(n, kChunk);
    w.fit_T.ensure(chunk * 16 * sizeof(float));
    w.fit_part.ensure(chunk * (size_t)nb * sizeof(double2));
    w.fit_out.ensure(chunk * sizeof(double2));
    for (size_t at = 0; at < n; at += chunk) {
      const size_t m = std::min(chunk, n - at);
      HIP_TRY(hipMemcpyAsync(w.fit_T.p, T_colmajor + at * 16, m * 16 * sizeof(float), hipMemcpyHostToDevice, h->stream));
      hipLaunchKernelGGL(k_fitness_batch, dim3((unsigned)nb, (unsigned)m), dim3(kKnnBlock), 0, h->stream, S.pts(), np, w.fit_T.as<float>(), T.pts(), T.cells(), T.grid, max_range,
                         w.fit_part.as<double2>());
      hipLaunchKernelGGL(k_fitness_final_batch, dim3((unsigned)m), dim3(kFitnessFinalBlock), 0, h->stream, w.fit_part.as<double2>(), nb, w.fit_out.as<double2>());
      HIP_TRY(hipMemcpyAsync(r.data() + at, w.fit_out.p, m * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
    }
    HIP_TRY(hipGetLastError());
    for (size_t i = 0; i < n; ++i) {
      const size_t cnt = (size_t)r[i].y;
      scores[i] = cnt ? r[i].x / r[i].y : std::numeric_limits<double>::max();
      if (n_inliers) n_inliers[i] = cnt;
    }
  });
}

int ngicp_linearize(ngicp_t* h, const double T[16], double H[36], double b[6], double* err) {
  return guarded(h, [&] {
    if (!T) throw ArgError{NGICP_ERR_ARG, "null pose"};
    LoopCtx c;
    VoxelCtx vc;
    const bool vox = h->voxel_res > 0.0;
    if (vox) prepare_voxel_loop(h, vc);
    else prepare_loop(h, c);
    LmState st;
    init_state_from_pose(st, pose_from_colmajor_d(T));
    HIP_TRY(hipMemcpyAsync(h->state.p, &st, sizeof(st), hipMemcpyHostToDevice, h->stream));
    if (vox) {
      vc.pa.mode = 2 | 4;
      launch_voxel_pass(h, vc);
      c.sa = vc.sa;
    } else {
      c.pa.mode = 2 | 4;
      launch_pass(h, c.pa, c.nblocks, h->stream);
    }
    c.sa.mode = 1;
    hipLaunchKernelGGL(k_lm_solve, dim3(1), dim3(kSolveThreads), 0, h->stream, c.sa);
    HIP_TRY(hipMemcpyAsync(&st, h->state.p, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    if (H)
      for (int r = 0; r < 6; ++r)
        for (int cc = 0; cc < 6; ++cc) H[cc * 6 + r] = st.hot.H[r * 6 + cc];
    if (b) std::memcpy(b, st.hot.b, sizeof(st.hot.b));
    if (err) *err = st.hot.y0;
    h->hook_valid = 1;
  });
}

int ngicp_compute_error(ngicp_t* h, const double T[16], double* err) {
  return guarded(h, [&] {
    if (!T) throw ArgError{NGICP_ERR_ARG, "null pose"};
    if (h->hook_valid != 1) throw ArgError{NGICP_ERR_STATE, "compute_error needs a preceding linearize"};
    LoopCtx c;
    VoxelCtx vc;
    const bool vox = h->voxel_res > 0.0;
    if (vox) prepare_voxel_loop(h, vc);
    else prepare_loop(h, c);
    // keep cur / have_lin, replace the trial pose (read in stream order: behind everything this handle has enqueued)
    LmState st;
    HIP_TRY(hipMemcpyAsync(&st, h->state.p, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const Pose x = pose_from_colmajor_d(T);
    st.hot.xi = x;
    for (int r = 0; r < 3; ++r) {
      for (int cc = 0; cc < 3; ++cc) st.xi_f[r * 4 + cc] = (float)x.R[r * 3 + cc];
      st.xi_f[r * 4 + 3] = (float)x.t[r];
    }
    HIP_TRY(hipMemcpyAsync(h->state.p, &st, sizeof(st), hipMemcpyHostToDevice, h->stream));
    if (vox) {
      vc.pa.mode = 1 | 4;
      launch_voxel_pass(h, vc);
      c.sa = vc.sa;
    } else {
      c.pa.mode = 1 | 4;
      launch_pass(h, c.pa, c.nblocks, h->stream);
    }
    c.sa.mode = 2;
    hipLaunchKernelGGL(k_lm_solve, dim3(1), dim3(kSolveThreads), 0, h->stream, c.sa);
    LmState st2;
    HIP_TRY(hipMemcpyAsync(&st2, h->state.p, sizeof(st2), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    if (err) *err = st2.hot.y0;
  });
}

int ngicp_get_correspondences(ngicp_t* h, int* corr_out, float* sqd_out) {
  return guarded(h, [&] {
    if (!corr_out) throw ArgError{NGICP_ERR_ARG, "null output"};
    if (!h->hook_valid) throw ArgError{NGICP_ERR_STATE, "no correspondences: call ngicp_linearize or ngicp_align first"};
    // In stream order: align() returns when the solver has published `done`, and the (pass, solve) pairs it had enqueued ahead may
    // still be on h->stream (a non-blocking stream: a null-stream copy would not wait for them).
    LmState st;
    HIP_TRY(hipMemcpyAsync(&st, h->state.p, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t n = h->src.dev->n;
    h->knn_idx.ensure(n * sizeof(int));
    h->knn_d2.ensure(n * sizeof(float));
    LmState* dst = h->state.as<LmState>();
    if (h->voxel_res > 0.0)  // voxel numbers; distances to (float)mean_v
      hipLaunchKernelGGL(k_voxel_corr_to_original, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                         (const int*)h->vox_corr[st.hot.cur].as<int>() + (h->voxel_nbr == NGICP_VOX_DIRECT27 ? (size_t)vox_nbr_centre<27>() * n : 0), h->src.dev->pts(), (int)n,
                         (const double*)h->vmap.rec.as<double>(), h->knn_idx.as<int>(), sqd_out ? h->knn_d2.as<float>() : nullptr, dst->hot.lin_f);
    else
    hipLaunchKernelGGL(k_corr_to_original, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->tpt[st.hot.cur].as<float4>(), h->src.dev->qpts.as<float4>(),
                       h->src.dev->pts(), h->tgt.dev->pts(), (int)n, h->knn_idx.as<int>(), sqd_out ? h->knn_d2.as<float>() : nullptr, dst->hot.lin_f);
    HIP_TRY(hipMemcpyAsync(corr_out, h->knn_idx.p, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (sqd_out) HIP_TRY(hipMemcpyAsync(sqd_out, h->knn_d2.p, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
  });
}

int ngicp_set_voxel_resolution(ngicp_t* h, double res) {
  return guarded(h, [&] {
    if (!std::isfinite(res) || res < 0.0) throw ArgError{NGICP_ERR_ARG, "voxel resolution must be finite and >= 0 (0 selects exact GICP)"};
    if (res > 0.0 && !((float)res > 0.f && std::isfinite((float)res) && std::isfinite(1.0f / (float)res)))
      throw ArgError{NGICP_ERR_ARG, "voxel resolution: neither it nor its inverse may leave the float range"};
    if (res == h->voxel_res) return;
    h->voxel_res = res;
    h->vmap.invalidate();  // (rebuilt at the next use; with res == 0 its memory stays with the handle, its holds on the target are dropped)
    h->hook_valid = 0;     // correspondences of the other mode, or voxel numbers of another lattice
  });
}

int ngicp_set_voxel_neighbors(ngicp_t* h, int mode) {
  return guarded(h, [&] {
    if (mode != NGICP_VOX_DIRECT1 && mode != NGICP_VOX_DIRECT7 && mode != NGICP_VOX_DIRECT27)
      throw ArgError{NGICP_ERR_ARG, "voxel neighbourhood must be NGICP_VOX_DIRECT1 (1), NGICP_VOX_DIRECT7 (7) or NGICP_VOX_DIRECT27 (27)"};
    if (mode == h->voxel_nbr) return;
    h->voxel_nbr = mode;   // (the voxel map does not depend on it and stays)
    h->hook_valid = 0;     // the per-slot state has another shape: compute_error and the correspondences wait for the next linearisation
  });
}

int ngicp_get_voxel_neighbors(const ngicp_t* h, int* mode) {
  if (!h || !mode) return NGICP_ERR_ARG;
  *mode = h->voxel_nbr;
  return NGICP_OK;
}

int ngicp_voxel_correspondences(ngicp_t* h, int* corr_n_by_K, size_t capacity_ints, int* K_out) {
  return guarded(h, [&] {
    if (!(h->voxel_res > 0.0)) throw ArgError{NGICP_ERR_STATE, "no voxel resolution set (ngicp_set_voxel_resolution)"};
    if (!h->hook_valid) throw ArgError{NGICP_ERR_STATE, "no correspondences: call ngicp_linearize or ngicp_align first"};
    const size_t n = h->src.dev->n, K = (size_t)h->voxel_nbr;
    if (K_out) *K_out = (int)K;
    if (!corr_n_by_K) throw ArgError{NGICP_ERR_ARG, "null output"};
    if (capacity_ints < n * K) throw ArgError{NGICP_ERR_ARG, "voxel correspondences: the output holds fewer than n_src * K ints"};
    LmState st;  // (in stream order, as ngicp_get_correspondences)
    HIP_TRY(hipMemcpyAsync(&st, h->state.p, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->vox_corr_out.ensure(n * K * sizeof(int));
    hipLaunchKernelGGL(k_voxel_corr_n_to_original, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const int*)h->vox_corr[st.hot.cur].as<int>(), h->src.dev->pts(), (int)n,
                       (int)K, (int)n, h->vox_corr_out.as<int>());
    HIP_TRY(hipMemcpyAsync(corr_n_by_K, h->vox_corr_out.p, n * K * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
  });
}

int ngicp_voxelmap_builds(const ngicp_t* h, long long* n_builds) {
  if (!h || !n_builds) return NGICP_ERR_ARG;
  *n_builds = h->voxel_builds;
  return NGICP_OK;
}

int ngicp_voxelmap_size(ngicp_t* h, size_t* n_voxels) {
  return guarded(h, [&] {
    if (!n_voxels) throw ArgError{NGICP_ERR_ARG, "null output"};
    if (!(h->voxel_res > 0.0)) throw ArgError{NGICP_ERR_STATE, "no voxel resolution set (ngicp_set_voxel_resolution)"};
    ensure_voxel_map(h);
    *n_voxels = h->vmap.n_vox;
  });
}

int ngicp_voxelmap_get(ngicp_t* h, int* ijk_n3, double* mean_n3, double* cov_n6, int* count_n) {
  return guarded(h, [&] {
    if (!(h->voxel_res > 0.0)) throw ArgError{NGICP_ERR_STATE, "no voxel resolution set (ngicp_set_voxel_resolution)"};
    ensure_voxel_map(h);
    const size_t nv = h->vmap.n_vox;
    std::vector<double> rec(nv * kVoxRec);
    std::vector<unsigned long long> keys(nv);
    HIP_TRY(hipMemcpyAsync(rec.data(), h->vmap.rec.p, rec.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(keys.data(), h->vmap.vkeys.p, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t v = 0; v < nv; ++v) {
      if (ijk_n3) {
        ijk_n3[3 * v + 0] = (int)(keys[v] & 0x1fffffull) - kVoxBias;
        ijk_n3[3 * v + 1] = (int)((keys[v] >> 21) & 0x1fffffull) - kVoxBias;
        ijk_n3[3 * v + 2] = (int)((keys[v] >> 42) & 0x1fffffull) - kVoxBias;
      }
      if (mean_n3) std::memcpy(mean_n3 + 3 * v, &rec[v * kVoxRec], 3 * sizeof(double));
      if (cov_n6) std::memcpy(cov_n6 + 6 * v, &rec[v * kVoxRec + 3], 6 * sizeof(double));
      if (count_n) count_n[v] = (int)rec[v * kVoxRec + 9];
    }
  });
}

int ngicp_set_voxel_submap_merge(ngicp_t* h, int on) {
  return guarded(h, [&] {
    const int v = on ? 1 : 0;
    if (v == h->voxel_merge) return;
    h->voxel_merge = v;
    h->vmap.invalidate();  // (rebuilt at the next use, by whichever route then applies)
    h->hook_valid = 0;     // as a change of resolution: the hooks' state and the correspondences go with the map
  });
}

int ngicp_get_voxel_submap_merge(const ngicp_t* h, int* on) {
  if (!h || !on) return NGICP_ERR_ARG;
  *on = h->voxel_merge;
  return NGICP_OK;
}

int ngicp_voxelmap_merge_stats(const ngicp_t* h, long long* merged_builds, long long* parts_built, double* last_parts_ms, double* last_merge_ms) {
  if (!h) return NGICP_ERR_ARG;
  if (merged_builds) *merged_builds = h->merged_builds;
  if (parts_built) *parts_built = h->parts_built;
  if (last_parts_ms) *last_parts_ms = h->last_parts_ms;
  if (last_merge_ms) *last_merge_ms = h->last_merge_ms;
  return NGICP_OK;
}

int ngicp_keyframe_voxelmap_get(ngicp_t* h, int id, size_t* n_vox, int* ijk_n3, double* sum_n3, double* covsum_n6, int* count_n) {
  return guarded(h, [&] {
    if (!(h->voxel_res > 0.0)) throw ArgError{NGICP_ERR_STATE, "no voxel resolution set (ngicp_set_voxel_resolution)"};
    if (id < 0 || (size_t)id >= h->keyframes.size()) throw ArgError{NGICP_ERR_ARG, "unknown keyframe id"};
    ngicp::Keyframe& kf = h->keyframes[(size_t)id];
    if (!keyframe_part_current(h, kf)) {
      size_voxel_work(h, kf.cloud->n);
      build_keyframe_part(h, id);
    }
    const size_t nv = kf.part->n_vox;
    if (n_vox) *n_vox = nv;
    if (!ijk_n3 && !sum_n3 && !covsum_n6 && !count_n) return;
    std::vector<double> rec(nv * kVoxRec);
    std::vector<unsigned long long> keys(nv);
    HIP_TRY(hipMemcpyAsync(rec.data(), kf.part->rec.p, rec.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(keys.data(), kf.part->keys.p, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    for (size_t v = 0; v < nv; ++v) {
      if (ijk_n3) {
        ijk_n3[3 * v + 0] = (int)(keys[v] & 0x1fffffull) - kVoxBias;
        ijk_n3[3 * v + 1] = (int)((keys[v] >> 21) & 0x1fffffull) - kVoxBias;
        ijk_n3[3 * v + 2] = (int)((keys[v] >> 42) & 0x1fffffull) - kVoxBias;
      }
      if (sum_n3) std::memcpy(sum_n3 + 3 * v, &rec[v * kVoxRec], 3 * sizeof(double));
      if (covsum_n6) std::memcpy(covsum_n6 + 6 * v, &rec[v * kVoxRec + 3], 6 * sizeof(double));
      if (count_n) count_n[v] = (int)rec[v * kVoxRec + 9];
    }
  });
}

int ngicp_target_knn(ngicp_t* h, const float* q, size_t nq, size_t stride, int k, int* idx, float* d2) {
  return guarded(h, [&] { knn_impl(h, 1, q, nq, stride, k, idx, d2); });
}

// ---- queries on the indexed clouds (ngicp_query.h) ----
int ngicp_knn_search(ngicp_t* h, int which, const float* q, size_t nq, size_t stride, int k, int* idx, float* d2) {
  return guarded(h, [&] { knn_impl(h, which, q, nq, stride, k, idx, d2); });
}

int ngicp_radius_search(ngicp_t* h, int which, const float* q, size_t nq, size_t stride, double radius, size_t* offsets, size_t* total) {
  return guarded(h, [&] {
    check_which(which);
    if (!offsets || !total) throw ArgError{NGICP_ERR_ARG, "null output"};
    if (nq && !q) throw ArgError{NGICP_ERR_ARG, "null pointer"};
    if (nq && (stride < 12 || stride % 4)) throw ArgError{NGICP_ERR_ARG, "bad stride"};
    if (nq > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "too many queries for int indices"};
    h->rad_valid = false;
    h->rad_total = 0;
    *total = 0;
    if (nq == 0) {
      offsets[0] = 0;
      h->rad_valid = true;
      return;
    }
    DeviceCloud& C = query_cloud(h, which);
    const float rf = (float)radius;  // RadiusResultSet<float,int> (nanoflann.hpp:161)
    if (!(rf > 0.f)) {  // d2 < radius holds for no d2 >= 0
      std::fill(offsets, offsets + nq + 1, (size_t)0);
      h->rad_valid = true;
      return;
    }
    // the cube the cell ranges must cover: sqrt(radius) rounded up, plus the grid's slack for the float cell assignment
    const float reach = (float)(std::sqrt((double)rf) * (1.0 + 1e-6)) + C.grid.slack;
    const int n = (int)nq;
    upload_queries(h, q, nq, stride);
    h->rad_counts.ensure(nq * sizeof(int));
    h->rad_offsets.ensure((nq + 1) * sizeof(unsigned long long));
    h->rad_long.ensure((nq + 1) * sizeof(int));  // {number of long segments, their queries}
    const int ntiles = (n + kScanTile - 1) / kScanTile;
    h->tile_sums.ensure((size_t)ntiles * sizeof(unsigned long long));
    int* n_long_dev = h->rad_long.as<int>();
    HIP_TRY(hipEventRecord(h->ev_q_a, h->stream));
    HIP_TRY(hipMemsetAsync(n_long_dev, 0, sizeof(int), h->stream));
    const dim3 wgrid((unsigned)((nq * kRadLanes + kRadBlock - 1) / kRadBlock));
    hipLaunchKernelGGL(k_radius_walk<false>, wgrid, dim3(kRadBlock), 0, h->stream, C.pts(), C.cells(), C.grid, h->queries.as<float4>(), n, rf, reach,
                       h->rad_counts.as<int>(), (const unsigned long long*)nullptr, (unsigned long long*)nullptr, n_long_dev + 1, n_long_dev);
    hipLaunchKernelGGL(k_scan64_tiles, dim3(ntiles), dim3(kScanBlock), 0, h->stream, h->rad_counts.as<int>(), n, h->tile_sums.as<unsigned long long>());
    hipLaunchKernelGGL(k_scan2_tile_sums, dim3(1), dim3(kScanBlock), 0, h->stream, h->tile_sums.as<unsigned long long>(), ntiles);
    hipLaunchKernelGGL(k_scan64_apply, dim3(ntiles), dim3(kScanBlock), 0, h->stream, h->rad_counts.as<int>(), n, h->tile_sums.as<unsigned long long>(),
                       h->rad_offsets.as<unsigned long long>());
    // the one read-back inside the search: the offsets (the total sizes the key buffer) and the number of long segments
    static_assert(sizeof(size_t) == sizeof(unsigned long long), "offsets are copied as they are");
    int n_long = 0;
    HIP_TRY(hipMemcpyAsync(offsets, h->rad_offsets.p, (nq + 1) * sizeof(size_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&n_long, n_long_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t tot = offsets[nq];
    if (n_long > 0 && C.n > ((size_t)1 << 30)) throw ArgError{NGICP_ERR_ARG, "segments beyond 2^30 points are not sorted by this engine"};
    if (tot > ((size_t)1 << 40) / sizeof(unsigned long long)) throw HipError{hipErrorOutOfMemory, "radius search result buffer", __FILE__, __LINE__};
    if (tot) {
      h->rad_keys.ensure(tot * sizeof(unsigned long long));
      hipLaunchKernelGGL(k_radius_walk<true>, wgrid, dim3(kRadBlock), 0, h->stream, C.pts(), C.cells(), C.grid, h->queries.as<float4>(), n, rf, reach,
                         (int*)nullptr, h->rad_offsets.as<unsigned long long>(), h->rad_keys.as<unsigned long long>(), (int*)nullptr, (int*)nullptr);
      hipLaunchKernelGGL(k_seg_sort_short, dim3((unsigned)((nq + kSegBlock / 64 - 1) / (kSegBlock / 64))), dim3(kSegBlock), 0, h->stream,
                         h->rad_offsets.as<unsigned long long>(), n, h->rad_keys.as<unsigned long long>());
      if (n_long > 0)
        hipLaunchKernelGGL(k_seg_sort_long, dim3((unsigned)n_long), dim3(kSegLongBlock), 0, h->stream, h->rad_offsets.as<unsigned long long>(), n_long_dev + 1,
                           h->rad_keys.as<unsigned long long>());
    }
    HIP_TRY(hipEventRecord(h->ev_q_b, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    query_timing_done(h);
    h->rad_total = tot;
    h->rad_valid = true;
    *total = tot;
  });
}

int ngicp_radius_fetch(ngicp_t* h, int* idx, float* sqd, size_t capacity) {
  return guarded(h, [&] {
    if (!idx || !sqd) throw ArgError{NGICP_ERR_ARG, "null output"};
    if (!h->rad_valid) throw ArgError{NGICP_ERR_STATE, "no radius search to fetch"};
    const size_t tot = h->rad_total;
    if (capacity < tot) throw ArgError{NGICP_ERR_ARG, "capacity is smaller than the search's total"};
    if (tot == 0) return;
    h->knn_idx.ensure(tot * sizeof(int));
    h->knn_d2.ensure(tot * sizeof(float));
    hipLaunchKernelGGL(k_radius_unpack, dim3((unsigned)std::min<size_t>((tot + 255) / 256, 4096)), dim3(256), 0, h->stream, h->rad_keys.as<unsigned long long>(), tot,
                       h->knn_idx.as<int>(), h->knn_d2.as<float>());
    HIP_TRY(hipMemcpyAsync(idx, h->knn_idx.p, tot * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(sqd, h->knn_d2.p, tot * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
  });
}

int ngicp_fitness_score(ngicp_t* h, const float T_colmajor[16], double max_range, double* score, size_t* n_inliers) {
  return guarded(h, [&] {
    if (!score) throw ArgError{NGICP_ERR_ARG, "null output"};
    DeviceCloud& S = query_cloud(h, 0);
    DeviceCloud& T = query_cloud(h, 1);
    const int n = (int)S.n;
    const int nb = (n + kKnnPairs - 1) / kKnnPairs;
    h->fit_T.ensure(16 * sizeof(float));
    h->fit_part.ensure((size_t)nb * sizeof(double2));
    h->fit_out.ensure(sizeof(double2));
    HIP_TRY(hipMemcpyAsync(h->fit_T.p, T_colmajor ? T_colmajor : h->final_T, 16 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->ev_q_a, h->stream));
    hipLaunchKernelGGL(k_fitness, dim3((unsigned)nb), dim3(kKnnBlock), 0, h->stream, S.pts(), n, h->fit_T.as<float>(), T.pts(), T.cells(), T.grid, max_range,
                       h->fit_part.as<double2>());
    hipLaunchKernelGGL(k_fitness_final, dim3(1), dim3(kFitnessFinalBlock), 0, h->stream, h->fit_part.as<double2>(), nb, h->fit_out.as<double2>());
    HIP_TRY(hipEventRecord(h->ev_q_b, h->stream));
    double2 r;
    HIP_TRY(hipMemcpyAsync(&r, h->fit_out.p, sizeof(r), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    query_timing_done(h);
    const size_t cnt = (size_t)r.y;
    *score = cnt ? r.x / r.y : std::numeric_limits<double>::max();
    if (n_inliers) *n_inliers = cnt;
  });
}

int ngicp_range_select(ngicp_t* h, int which, size_t rank, float* value, size_t* n_points) {
  return guarded(h, [&] { range_select_impl(h, which, rank, false, value, n_points); });
}

int ngicp_range_median(ngicp_t* h, int which, float* value, size_t* n_points) {
  return guarded(h, [&] { range_select_impl(h, which, 0, true, value, n_points); });
}

int ngicp_get_lm_trace(ngicp_t* h, double* rows, size_t max_rows, size_t* n_rows) {
  return guarded(h, [&] {
    if (h->trace_host.empty() && h->trace_rows_dev) {
      h->trace_host.resize(h->trace_rows_dev * kTraceCols);
      HIP_TRY(hipMemcpyAsync(h->trace_host.data(), h->trace.p, h->trace_host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));  // (stream order)
      HIP_TRY(hipStreamSynchronize(h->stream));
    }
    const size_t n = h->trace_host.size() / kTraceCols;
    if (n_rows) *n_rows = n;
    if (rows) std::memcpy(rows, h->trace_host.data(), std::min(n, max_rows) * kTraceCols * sizeof(double));
  });
}

int ngicp_get_stats(ngicp_t* h, ngicp_stats* out) {
  if (!h || !out) return NGICP_ERR_ARG;
  if (h->cov_timing_pending) {
    float ms = 0.f;
    if (hipEventSynchronize(h->ev_cov_b) == hipSuccess && hipEventElapsedTime(&ms, h->ev_cov_a, h->ev_cov_b) == hipSuccess) h->stats.covariance_ms = ms;
    h->cov_timing_pending = false;
  }
  h->stats.device_allocs = g_device_allocs.load(std::memory_order_relaxed);
  *out = h->stats;
  return NGICP_OK;
}
int ngicp_set_host_wait(ngicp_t* h, int mode) {
  if (!h || (mode != 0 && mode != 1)) return NGICP_ERR_ARG;
  h->host_wait = mode;
  return NGICP_OK;
}
int ngicp_set_profiling(ngicp_t* h, int on) {
  return guarded(h, [&] {
    h->profiling = on != 0;
    h->prof_stride = on > 1 ? on : 1;
    if (h->profiling && h->prof_events.empty()) {
      h->prof_events.resize(2 * 1024);
      for (auto& e : h->prof_events) HIP_TRY(hipEventCreate(&e));
    }
  });
}

// ---- point-sharded stepping ----
// One loop context per alignment (ngicp_sharded_begin); per pass two small launches around the caller's all-reduce (the pass +
// a reduce-only solver, then the solver proper on the reduced vector); no host synchronisation per pass: the `done` word of
// step k is copied to pinned memory behind an event and READ AT STEP k + kShardLag.  The lag is a constant, so every rank
// takes the same decision in the same step (a rank that stopped calling the collective earlier than its peers would hang them);
// the extra kShardLag passes after the end are no-ops (both kernels return at once when the state says done).
int ngicp_sharded_begin(ngicp_t* h, const float guess[16]) {
  return guarded(h, [&] {
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    refuse_if_voxelized(h, "ngicp_sharded_begin");
    h->shard_ctx.reset(new LoopCtx);
    LoopCtx& c = *h->shard_ctx;
    prepare_loop(h, c);
    c.pa.mode = (h->p.optimizer == NGICP_OPT_GAUSS_NEWTON) ? 2 : 3;
    if (h->prev_staged_fraction < 0.0 || h->prev_staged_fraction >= 0.12) c.pa.mode |= 32;  // (see do_align)
    LmState st;
    init_state_from_pose(st, pose_from_colmajor_f(guess ? guess : I));
    if (h->p.max_iter <= 0) st.hot.done = 1;
    h->pin_state[0] = st;
    HIP_TRY(hipMemcpyAsync(h->state.p, &h->pin_state[0], sizeof(st), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // once per alignment: the caller may step on a stream of its own
    for (int i = 0; i < kShardSlots; ++i) h->h_shard_done[i] = 0;
    h->shard_steps = 0;
    h->sharded_active = true;
    h->hook_valid = 0;
  });
}

int ngicp_sharded_pass(ngicp_t* h, double* sums32_dev, void* stream_or_null) {
  return guarded(h, [&] {
    refuse_if_voxelized(h, "ngicp_sharded_pass");
    if (!h->sharded_active || !h->shard_ctx) throw ArgError{NGICP_ERR_STATE, "ngicp_sharded_begin not called"};
    if (!sums32_dev) throw ArgError{NGICP_ERR_ARG, "null sums buffer"};
    hipStream_t s = stream_or_null ? (hipStream_t)stream_or_null : h->stream;
    LoopCtx& c = *h->shard_ctx;
    launch_pass(h, c.pa, c.nblocks, s);
    SolveArgs sa = c.sa;
    sa.mode = 3;  // reduce only: this rank's 32 sums, for the caller's all-reduce
    sa.sums_out = sums32_dev;
    sa.grp_order = nullptr;
    hipLaunchKernelGGL(k_lm_solve, dim3(1), dim3(kSolveThreads), 0, s, sa);
    HIP_TRY(hipGetLastError());
  });
}

int ngicp_sharded_step(ngicp_t* h, const double* sums32_dev, void* stream_or_null, int* done) {
  return guarded(h, [&] {
    refuse_if_voxelized(h, "ngicp_sharded_step");
    if (!h->sharded_active || !h->shard_ctx) throw ArgError{NGICP_ERR_STATE, "ngicp_sharded_begin not called"};
    if (!sums32_dev) throw ArgError{NGICP_ERR_ARG, "null sums buffer"};
    hipStream_t s = stream_or_null ? (hipStream_t)stream_or_null : h->stream;
    LoopCtx& c = *h->shard_ctx;
    SolveArgs sa = c.sa;
    sa.mode = 0;
    sa.partials = sums32_dev;  // one pre-reduced row
    sa.nblocks = 1;
    sa.grp_order = nullptr;    // (the launch order of the pass is per rank and is left alone)
    hipLaunchKernelGGL(k_lm_solve, dim3(1), dim3(kSolveThreads), 0, s, sa);
    h->shard_stream = s;
    const long k = h->shard_steps++;
    const int slot = (int)(k % kShardSlots);
    LmState* dst = h->state.as<LmState>();
    HIP_TRY(hipMemcpyAsync(&h->h_shard_done[slot], &dst->hot.done, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(h->ev_shard[slot], s));
    HIP_TRY(hipGetLastError());
    int d = 0;
    if (k >= kShardLag) {  // the flag of step k - kShardLag: its copy finished long ago, the wait does not stall the stream
      const int old = (int)((k - kShardLag) % kShardSlots);
      HIP_TRY(hipEventSynchronize(h->ev_shard[old]));
      d = h->h_shard_done[old];
    }
    if (done) *done = d;
  });
}

int ngicp_sharded_finish(ngicp_t* h, float T_out[16], int* converged, int* nr_iterations, double final_hessian[36]) {
  return guarded(h, [&] {
    refuse_if_voxelized(h, "ngicp_sharded_finish");
    if (!h->sharded_active) throw ArgError{NGICP_ERR_STATE, "ngicp_sharded_begin not called"};
    hipStream_t s = h->shard_stream ? h->shard_stream : h->stream;  // the steps were enqueued there
    HIP_TRY(hipMemcpyAsync(&h->pin_state[1], h->state.p, sizeof(LmState), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const LmState& st = h->pin_state[1];
    pose_to_colmajor_f(st.hot.x0, h->final_T);
    h->converged = st.hot.converged;
    h->nr_iterations = st.hot.nr_iterations;
    for (int r = 0; r < 6; ++r)
      for (int cc = 0; cc < 6; ++cc) h->final_hessian[cc * 6 + r] = st.hot.final_H[r * 6 + cc];
    if (st.hot.lm_failed) std::fprintf(stderr, "lm not converged!!\n");  // impl/lsq_registration_impl.hpp:106
    if (T_out) std::memcpy(T_out, h->final_T, sizeof(h->final_T));
    if (converged) *converged = h->converged;
    if (nr_iterations) *nr_iterations = h->nr_iterations;
    if (final_hessian) std::memcpy(final_hessian, h->final_hessian, sizeof(h->final_hessian));
    h->sharded_active = false;
    h->shard_ctx.reset();
    h->shard_stream = nullptr;
  });
}

// ---- K1 sharded over ranks: every rank computes a block of the packed covariance array, the caller all-gathers ----
int ngicp_covs_shard_begin(ngicp_t* h, int which, double** covs6_dev, size_t* n_points) {
  return guarded(h, [&] {
    refuse_if_voxelized(h, "ngicp_covs_shard_begin");
    if ((which != 0 && which != 1) || !covs6_dev || !n_points) throw ArgError{NGICP_ERR_ARG, "bad argument"};
    Slot& slot = which ? h->tgt : h->src;
    ensure_slot_ready(h, slot, which ? "target" : "source");
    CovSet& cs = h->shard_covs[which];
    cs.data = acquire_buf(h, h->device, slot.dev->n * 6 * sizeof(double));
    cs.n = slot.dev->n;
    cs.order = slot.dev;
    HIP_TRY(hipStreamSynchronize(h->stream));  // (the index build; the caller may use a stream of its own from here on)
    *covs6_dev = cs.data->as<double>();
    *n_points = cs.n;
  });
}
int ngicp_covs_shard_compute(ngicp_t* h, int which, size_t lo, size_t hi, void* stream_or_null) {
  return guarded(h, [&] {
    refuse_if_voxelized(h, "ngicp_covs_shard_compute");
    if (which != 0 && which != 1) throw ArgError{NGICP_ERR_ARG, "bad argument"};
    CovSet& cs = h->shard_covs[which];
    Slot& slot = which ? h->tgt : h->src;
    if (!cs.data || cs.order.get() != slot.dev.get()) throw ArgError{NGICP_ERR_STATE, "ngicp_covs_shard_begin not called for this cloud"};
    if (lo > hi || hi > cs.n) throw ArgError{NGICP_ERR_ARG, "block outside the cloud"};
    launch_cov_range(h, *slot.dev, cs.data->as<double>(), lo, hi, stream_or_null ? (hipStream_t)stream_or_null : h->stream);
    HIP_TRY(hipGetLastError());
  });
}
int ngicp_covs_shard_commit(ngicp_t* h, int which) {
  return guarded(h, [&] {
    refuse_if_voxelized(h, "ngicp_covs_shard_commit");
    if (which != 0 && which != 1) throw ArgError{NGICP_ERR_ARG, "bad argument"};
    CovSet& cs = h->shard_covs[which];
    Slot& slot = which ? h->tgt : h->src;
    if (!cs.data || cs.order.get() != slot.dev.get()) throw ArgError{NGICP_ERR_STATE, "ngicp_covs_shard_begin not called for this cloud"};
    (which ? h->tgt_covs : h->src_covs) = cs;
    cs.clear();
  });
}

// ---- device-resident keyframe store + submap assembly ----
int ngicp_keyframe_add(ngicp_t* h, ngicp_t* from, int* id_out) {
  if (!from) return NGICP_ERR_ARG;
  return guarded(h, [&] {
    if (h->device != from->device) throw ArgError{NGICP_ERR_ARG, "keyframe_add across devices is not supported"};
    ensure_slot_ready(from, from->src, "source");
    // `keyframe_normals.push_back(gicp_s2s.getSourceCovariances())` (odom.cc:1174): the covariances the producer holds for its
    // source; computed now if absent, with the producer's k / regularisation (calculateSourceCovariances, odom.cc:1173)
    if (from->src_covs.n != from->src.dev->n) compute_covs(from, from->src, from->src_covs, "source");
    (void)covs_for(from, from->src_covs, from->src.dev);  // in the cloud's own sorted order
    HIP_TRY(hipStreamSynchronize(from->stream));          // the store is read on other streams later (keyframes are rare)
    h->keyframes.push_back({from->src.dev, from->src_covs.data});
    if (id_out) *id_out = (int)h->keyframes.size() - 1;
  });
}

int ngicp_keyframe_add_transformed(ngicp_t* h, ngicp_t* from, const float T_colmajor[16], int* id_out) {
  if (!from) return NGICP_ERR_ARG;
  return guarded(h, [&] {
    if (!T_colmajor) throw ArgError{NGICP_ERR_ARG, "null transform"};
    if (h->device != from->device) throw ArgError{NGICP_ERR_ARG, "keyframe_add across devices is not supported"};
    ensure_slot_ready(from, from->src, "source");
    // transformCurrentScan (odom.cc:971-974) + setInputSource(keyframe_cloud) + calculateSourceCovariances (odom.cc:1172-1173),
    // all on the device: the scan is already there as the producer's source
    DeviceCloud& S = *from->src.dev;
    const size_t n = S.n;
    from->tfinal.ensure(16 * sizeof(float));
    HIP_TRY(hipMemcpyAsync(from->tfinal.p, T_colmajor, 16 * sizeof(float), hipMemcpyHostToDevice, from->stream));
    from->unsorted.ensure(n * sizeof(float4));
    const int bbox_blocks = pick_blocks(n, 1024, 512);
    from->bbox.ensure((size_t)bbox_blocks * 8 * sizeof(float));
    hipLaunchKernelGGL(k_transform_to_unsorted, dim3(bbox_blocks), dim3(256), 0, from->stream, S.pts(), (int)n, from->tfinal.as<float>(), from->unsorted.as<float4>(),
                       from->bbox.as<float>());
    std::vector<float> bb((size_t)bbox_blocks * 8);
    HIP_TRY(hipMemcpyAsync(bb.data(), from->bbox.p, bb.size() * sizeof(float), hipMemcpyDeviceToHost, from->stream));
    HIP_TRY(hipStreamSynchronize(from->stream));
    float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (int b = 0; b < bbox_blocks; ++b)
      for (int d = 0; d < 3; ++d) {
        mn[d] = std::min(mn[d], bb[(size_t)b * 8 + d]);
        mx[d] = std::max(mx[d], bb[(size_t)b * 8 + 3 + d]);
      }
    for (int d = 0; d < 3; ++d)
      if (!std::isfinite(mn[d]) || !std::isfinite(mx[d]) || mn[d] > mx[d]) throw ArgError{NGICP_ERR_ARG, "transform produced non-finite coordinates"};
    Slot tmp;
    tmp.present = true;
    tmp.n = n;
    tmp.dev = index_unsorted(from, n, mn, mx);
    CovSet cs;
    compute_covs(from, tmp, cs, "keyframe");
    HIP_TRY(hipStreamSynchronize(from->stream));
    h->keyframes.push_back({tmp.dev, cs.data});
    if (id_out) *id_out = (int)h->keyframes.size() - 1;
  });
}

int ngicp_keyframe_add_transformed_filtered(ngicp_t* h, ngicp_t* from, const float T_colmajor[16], float leaf, int* id_out) {
  if (!from) return NGICP_ERR_ARG;
  if (!(leaf > 0.f)) return ngicp_keyframe_add_transformed(h, from, T_colmajor, id_out);  // vf_submap_use_ == false
  return guarded(h, [&] {
    if (!T_colmajor) throw ArgError{NGICP_ERR_ARG, "null transform"};
    if (h->device != from->device) throw ArgError{NGICP_ERR_ARG, "keyframe_add across devices is not supported"};
    ensure_slot_ready(from, from->src, "source");
    // DLO's shipped configuration (cfg/params.yaml:33-35: voxelFilter.submap.use = true, res = 0.5): transformCurrentScan
    // (odom.cc:971-974), vf_submap.filter(*current_scan_t) (odom.cc:1160-1163), setInputSource(keyframe_cloud) +
    // calculateSourceCovariances (odom.cc:1172-1173) - the scan is already on the device as the producer's source, and nothing of
    // this visits the host: transform into the scan's ORIGINAL point order (the order VoxelGrid adds the points of a voxel in),
    // VoxelGrid centroids, index build, covariances with the producer's k.
    DeviceCloud& S = *from->src.dev;
    const size_t n = S.n;
    from->tfinal.ensure(16 * sizeof(float));
    HIP_TRY(hipMemcpyAsync(from->tfinal.p, T_colmajor, 16 * sizeof(float), hipMemcpyHostToDevice, from->stream));
    from->xyzi.ensure(n * sizeof(float4));
    hipLaunchKernelGGL(k_transform_sorted_to_original4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, from->stream, S.pts(), (int)n, from->tfinal.as<float>(),
                       from->xyzi.as<float4>());
    from->filt_out = nullptr;  // (the producer's filter workspace is reused: a preprocessed scan waiting there is gone)
    from->filt_n = 0;
    char err[256] = {0};
    const float4* out = nullptr;
    int m = 0;
    if (ngk_filter_cloud(from->stream, &from->fws, from->xyzi.as<float4>(), (int)n, 0, 0.f, leaf, &out, &m, err, sizeof(err))) throw ArgError{NGICP_ERR_HIP, err};
    if (m <= 0) throw ArgError{NGICP_ERR_ARG, "the voxel filter left no points"};
    from->unsorted.ensure((size_t)m * sizeof(float4));
    const int bbox_blocks = pick_blocks((size_t)m, 1024, 512);
    from->bbox.ensure((size_t)bbox_blocks * 8 * sizeof(float));
    hipLaunchKernelGGL(k_xyzi_to_unsorted, dim3(bbox_blocks), dim3(256), 0, from->stream, out, m, from->unsorted.as<float4>(), from->bbox.as<float>());
    std::vector<float> bb((size_t)bbox_blocks * 8);
    HIP_TRY(hipMemcpyAsync(bb.data(), from->bbox.p, bb.size() * sizeof(float), hipMemcpyDeviceToHost, from->stream));
    HIP_TRY(hipStreamSynchronize(from->stream));
    float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (int b = 0; b < bbox_blocks; ++b)
      for (int d = 0; d < 3; ++d) {
        mn[d] = std::min(mn[d], bb[(size_t)b * 8 + d]);
        mx[d] = std::max(mx[d], bb[(size_t)b * 8 + 3 + d]);
      }
    for (int d = 0; d < 3; ++d)
      if (!std::isfinite(mn[d]) || !std::isfinite(mx[d]) || mn[d] > mx[d]) throw ArgError{NGICP_ERR_ARG, "transform produced non-finite coordinates"};
    Slot tmp;
    tmp.present = true;
    tmp.n = (size_t)m;
    tmp.dev = index_unsorted(from, (size_t)m, mn, mx);
    CovSet cs;
    compute_covs(from, tmp, cs, "keyframe");
    HIP_TRY(hipStreamSynchronize(from->stream));
    h->keyframes.push_back({tmp.dev, cs.data});
    if (id_out) *id_out = (int)h->keyframes.size() - 1;
  });
}

int ngicp_keyframe_count(const ngicp_t* h, size_t* n) {
  if (!h || !n) return NGICP_ERR_ARG;
  *n = h->keyframes.size();
  return NGICP_OK;
}

int ngicp_keyframe_size(const ngicp_t* h, int id, size_t* n_points) {
  if (!h || !n_points || id < 0 || (size_t)id >= h->keyframes.size()) return NGICP_ERR_ARG;
  *n_points = h->keyframes[(size_t)id].cloud->n;
  return NGICP_OK;
}

int ngicp_keyframe_clear(ngicp_t* h) {
  return guarded(h, [&] {
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->keyframes.clear();
    h->submap_ids.clear();
    h->submap_cloud = nullptr;
  });
}

int ngicp_submap_set(ngicp_t* h, const int* ids, size_t n_ids, int* changed_out) {
  return guarded(h, [&] {
    if (changed_out) *changed_out = 0;
    if (!ids || n_ids == 0) throw ArgError{NGICP_ERR_ARG, "empty keyframe list"};
    size_t total = 0;
    for (size_t i = 0; i < n_ids; ++i) {
      if (ids[i] < 0 || (size_t)ids[i] >= h->keyframes.size()) throw ArgError{NGICP_ERR_ARG, "unknown keyframe id"};
      total += h->keyframes[(size_t)ids[i]].cloud->n;
    }
    if (total > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "submap too large for int indices"};
    // `if (submap_kf_idx_curr == submap_kf_idx_prev) submap_hasChanged = false` (odom.cc:1308-1310, 827): same keyframes, and the
    // submap built from them is still the target -> nothing to do
    if (h->tgt.present && h->tgt.dev && h->tgt.dev.get() == h->submap_cloud && h->submap_ids.size() == n_ids &&
        std::equal(h->submap_ids.begin(), h->submap_ids.end(), ids) && h->tgt_covs.n == total)
      return;
    const double t0 = now_ms();
    // concatenation in keyframe order (odom.cc:1318-1325): point g = offset_k + (original index inside keyframe k)
    h->unsorted.ensure(total * sizeof(float4));
    float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    size_t off = 0;
    for (size_t i = 0; i < n_ids; ++i) {
      const ngicp::Keyframe& kf = h->keyframes[(size_t)ids[i]];
      const int nk = (int)kf.cloud->n;
      hipLaunchKernelGGL(k_keyframe_gather, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, h->stream, kf.cloud->pts(), nk, (int)off, h->unsorted.as<float4>());
      for (int d = 0; d < 3; ++d) {
        mn[d] = std::min(mn[d], kf.cloud->bb_min[d]);
        mx[d] = std::max(mx[d], kf.cloud->bb_max[d]);
      }
      off += (size_t)nk;
    }
    auto dc = index_unsorted(h, total, mn, mx);
    ensure_inv_perm(h, *dc);
    auto buf = acquire_buf(h, h->device, total * 6 * sizeof(double));
    off = 0;
    for (size_t i = 0; i < n_ids; ++i) {
      const ngicp::Keyframe& kf = h->keyframes[(size_t)ids[i]];
      const int nk = (int)kf.cloud->n;
      hipLaunchKernelGGL(k_keyframe_covs_scatter, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, h->stream, kf.cloud->pts(), kf.covs->as<double>(), nk, (int)off,
                         dc->inv_perm.as<int>(), buf->as<double>());
      off += (size_t)nk;
    }
    HIP_TRY(hipGetLastError());
    // setInputTarget(submap_cloud) + setTargetCovariances(submap_normals) (odom.cc:830-833)
    h->tgt.clear();
    h->tgt.present = true;
    h->tgt.n = total;
    h->tgt.dev = dc;
    h->tgt_covs.data = buf;
    h->tgt_covs.n = total;
    h->tgt_covs.order = dc;
    h->submap_ids.assign(ids, ids + n_ids);
    h->submap_cloud = dc.get();
    h->submap_covs = buf;
    drop_voxel_map(h);
    h->hook_valid = 0;
    h->stats.submap_ms = now_ms() - t0;
    if (changed_out) *changed_out = 1;
  });
}

int ngicp_get_target_points(ngicp_t* h, float* xyz_out, size_t out_stride_bytes, size_t* n_out) {
  return guarded(h, [&] {
    ensure_slot_ready(h, h->tgt, "target");
    const size_t n = h->tgt.dev->n;
    if (n_out) *n_out = n;
    if (!xyz_out) return;
    if (out_stride_bytes < 12 || out_stride_bytes % 4) throw ArgError{NGICP_ERR_ARG, "bad out_stride_bytes"};
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    download_transformed(h, *h->tgt.dev, I, xyz_out, out_stride_bytes);
  });
}

// ---- rigid transform of clouds ----
int ngicp_transform_source(ngicp_t* h, const float T_colmajor[16], float* xyz_out, size_t out_stride_bytes) {
  return guarded(h, [&] {
    if (!T_colmajor || !xyz_out) throw ArgError{NGICP_ERR_ARG, "null pointer"};
    if (out_stride_bytes < 12 || out_stride_bytes % 4) throw ArgError{NGICP_ERR_ARG, "bad out_stride_bytes"};
    ensure_slot_ready(h, h->src, "source");
    download_transformed(h, *h->src.dev, T_colmajor, xyz_out, out_stride_bytes);
  });
}

int ngicp_transform_cloud(ngicp_t* h, const float* xyz, size_t n, size_t stride_bytes, const float T_colmajor[16], float* xyz_out, size_t out_stride_bytes) {
  return guarded(h, [&] {
    if (n == 0) return;
    if (!xyz || !T_colmajor || !xyz_out) throw ArgError{NGICP_ERR_ARG, "null pointer"};
    if (stride_bytes < 12 || stride_bytes % 4 || out_stride_bytes < 12 || out_stride_bytes % 4) throw ArgError{NGICP_ERR_ARG, "bad stride"};
    if (n > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "cloud too large for int indices"};
    const size_t raw_bytes = (n - 1) * stride_bytes + 12;
    h->raw.ensure(raw_bytes);
    h->tfinal.ensure(16 * sizeof(float));
    h->out_xyz.ensure(n * 3 * sizeof(float));
    HIP_TRY(hipMemcpyAsync(h->raw.p, xyz, raw_bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->tfinal.p, T_colmajor, 16 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_transform_raw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->raw.as<unsigned char>(), stride_bytes, (int)n, h->tfinal.as<float>(),
                       h->out_xyz.as<float>());
    download_xyz(h, n, xyz_out, out_stride_bytes);
  });
}

// ---- test hook: ngicp_math.h on the device ----
int ngicp_math_selftest(ngicp_t* h, int which, const double* in, size_t n_problems, double* out) {
  return guarded(h, [&] {
    static const int kIn[4] = {3, 42, 6, 6}, kOut[4] = {9, 6, 12, 6};
    if (which < 0 || which > 3 || !in || !out) throw ArgError{NGICP_ERR_ARG, "bad arguments"};
    if (n_problems == 0) return;
    DevBuf di, dout;
    di.ensure(n_problems * kIn[which] * sizeof(double));
    dout.ensure(n_problems * kOut[which] * sizeof(double));
    HIP_TRY(hipMemcpyAsync(di.p, in, n_problems * kIn[which] * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_math_selftest, dim3((unsigned)((n_problems + 63) / 64)), dim3(64), 0, h->stream, which, di.as<double>(), (int)n_problems, dout.as<double>());
    HIP_TRY(hipMemcpyAsync(out, dout.p, n_problems * kOut[which] * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
  });
}

// ---- measurement: device stream copy ----
int ngicp_measure_copy_bandwidth(ngicp_t* h, size_t bytes, int reps, double* gbps_out) {
  return guarded(h, [&] {
    if (!gbps_out || bytes < 4096 || reps <= 0) throw ArgError{NGICP_ERR_ARG, "bad arguments"};
    const size_t n16 = bytes / 16;
    DevBuf a, b;
    a.ensure(n16 * 16);
    b.ensure(n16 * 16);
    HIP_TRY(hipMemsetAsync(a.p, 1, n16 * 16, h->stream));
    const unsigned blocks = (unsigned)((n16 + 1023) / 1024);
    for (int i = 0; i < 2; ++i) hipLaunchKernelGGL(k_stream_copy, dim3(blocks), dim3(256), 0, h->stream, a.as<float4>(), b.as<float4>(), n16);
    HIP_TRY(hipEventRecord(h->ev_a, h->stream));
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_stream_copy, dim3(blocks), dim3(256), 0, h->stream, a.as<float4>(), b.as<float4>(), n16);
    HIP_TRY(hipEventRecord(h->ev_b, h->stream));
    HIP_TRY(hipEventSynchronize(h->ev_b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev_a, h->ev_b));
    HIP_TRY(hipGetLastError());
    *gbps_out = 2.0 * (double)(n16 * 16) * reps / ((double)ms * 1e-3) / 1e9;  // read + write
  });
}

}  // extern "C"

// ---- scan preprocessing and map accumulation + voxel filter ----
namespace {
// host cloud (strided xyz [+ intensity]) -> device float4 {x, y, z, intensity} at dst[0..n)
void upload_xyzi(ngicp* h, const float* pts, size_t n, size_t stride, long intensity_off, float4* dst) {
  if (stride < 12 || stride % 4) throw ArgError{NGICP_ERR_ARG, "stride_bytes must be a multiple of 4 and >= 12"};
  if (intensity_off >= 0 && ((size_t)intensity_off + 4 > stride || intensity_off % 4)) throw ArgError{NGICP_ERR_ARG, "intensity offset outside the point stride"};
  if (n > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "cloud too large for int indices"};
  const size_t raw_bytes = (n - 1) * stride + (intensity_off >= 0 ? std::max((size_t)12, (size_t)intensity_off + 4) : 12);
  h->raw.ensure(raw_bytes);
  HIP_TRY(hipMemcpyAsync(h->raw.p, pts, raw_bytes, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_unpack_xyzi, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->raw.as<unsigned char>(), stride, intensity_off, (int)n, dst);
}
void download_xyzi(ngicp* h, const float4* src, size_t n, float* out) {
  if (n == 0) return;
  HIP_TRY(hipMemcpyAsync(out, src, n * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
}
}  // namespace

extern "C" {

int ngicp_preprocess_scan(ngicp_t* h, const float* pts, size_t n, size_t stride_bytes, long intensity_offset_bytes, int remove_nan, float crop_half_extent,
                          float voxel_leaf, float* out_xyzi, size_t out_capacity, size_t* n_out) {
  return guarded(h, [&] {
    if (n_out) *n_out = 0;
    h->filt_out = nullptr;
    h->filt_n = 0;
    if (n == 0) return;
    if (!pts) throw ArgError{NGICP_ERR_ARG, "null cloud pointer"};
    h->xyzi.ensure(n * sizeof(float4));
    upload_xyzi(h, pts, n, stride_bytes, intensity_offset_bytes, h->xyzi.as<float4>());
    char err[256] = {0};
    const float4* out = nullptr;
    int m = 0;
    if (ngk_filter_cloud(h->stream, &h->fws, h->xyzi.as<float4>(), (int)n, remove_nan, crop_half_extent, voxel_leaf, &out, &m, err, sizeof(err)))
      throw ArgError{NGICP_ERR_HIP, err};
    h->filt_out = out;
    h->filt_n = m;
    if (n_out) *n_out = (size_t)m;
    if (out_xyzi) {
      if ((size_t)m > out_capacity) throw ArgError{NGICP_ERR_ARG, "output buffer too small for the filtered cloud"};
      download_xyzi(h, out, (size_t)m, out_xyzi);
    }
  });
}

int ngicp_set_source_preprocessed(ngicp_t* h, uint64_t host_identity) {
  int rc = guarded(h, [&] {
    if (!h->filt_out || h->filt_n <= 0) throw ArgError{NGICP_ERR_STATE, "no preprocessed cloud: call ngicp_preprocess_scan first"};
    const size_t n = (size_t)h->filt_n;
    h->unsorted.ensure(n * sizeof(float4));
    const int bbox_blocks = pick_blocks(n, 1024, 512);
    h->bbox.ensure((size_t)bbox_blocks * 8 * sizeof(float));
    hipLaunchKernelGGL(k_xyzi_to_unsorted, dim3(bbox_blocks), dim3(256), 0, h->stream, h->filt_out, (int)n, h->unsorted.as<float4>(), h->bbox.as<float>());
    std::vector<float> bb((size_t)bbox_blocks * 8);
    HIP_TRY(hipMemcpyAsync(bb.data(), h->bbox.p, bb.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (int b = 0; b < bbox_blocks; ++b)
      for (int d = 0; d < 3; ++d) {
        mn[d] = std::min(mn[d], bb[(size_t)b * 8 + d]);
        mx[d] = std::max(mx[d], bb[(size_t)b * 8 + 3 + d]);
      }
    for (int d = 0; d < 3; ++d)
      if (!std::isfinite(mn[d]) || !std::isfinite(mx[d]) || mn[d] > mx[d]) throw ArgError{NGICP_ERR_ARG, "preprocessed cloud contains non-finite coordinates (filter it with remove_nan)"};
    auto dc = index_unsorted(h, n, mn, mx);
    h->src.clear();  // setInputSource (impl/nano_gicp_impl.hpp:121-129) with a cloud that is already on the device
    h->src.present = true;
    h->src.n = n;
    h->src.identity = host_identity;
    h->src.dev = dc;
    h->src_covs.clear();
  });
  return rc;
}

int ngicp_map_add(ngicp_t* h, const float* pts, size_t n, size_t stride_bytes, long intensity_offset_bytes) {
  return guarded(h, [&] {
    if (n == 0) return;
    if (!pts) throw ArgError{NGICP_ERR_ARG, "null cloud pointer"};
    if (h->map_n + n > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "map too large for int indices"};
    if ((h->map_n + n) * sizeof(float4) > h->map_pts.cap) {  // grow, keeping what is there (`*dlo_map += *keyframe`, map.cc:129)
      DevBuf bigger;
      bigger.ensure((h->map_n + n) * 2 * sizeof(float4));
      if (h->map_n) HIP_TRY(hipMemcpyAsync(bigger.p, h->map_pts.p, h->map_n * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
      std::swap(bigger.p, h->map_pts.p);
      std::swap(bigger.cap, h->map_pts.cap);
    }
    upload_xyzi(h, pts, n, stride_bytes, intensity_offset_bytes, h->map_pts.as<float4>() + h->map_n);
    h->map_n += n;
    HIP_TRY(hipGetLastError());
  });
}

int ngicp_map_voxel_filter(ngicp_t* h, float leaf, size_t* n_out) {
  return guarded(h, [&] {
    if (n_out) *n_out = h->map_n;
    if (h->map_n == 0 || !(leaf > 0.f)) return;
    char err[256] = {0};
    const float4* out = nullptr;
    int m = 0;
    // The filter workspace is shared with ngicp_preprocess_scan: whatever that call left there (h->filt_out points into it) is
    // overwritten or reallocated now, so a later ngicp_set_source_preprocessed must find nothing rather than stale memory.
    h->filt_out = nullptr;
    h->filt_n = 0;
    // voxelgrid.setInputCloud(dlo_map); voxelgrid.filter(*dlo_map)  (map.cc:102-104): the map is replaced by its centroids
    if (ngk_filter_cloud(h->stream, &h->fws, h->map_pts.as<float4>(), (int)h->map_n, 0, 0.f, leaf, &out, &m, err, sizeof(err))) throw ArgError{NGICP_ERR_HIP, err};
    if (out != h->map_pts.as<float4>()) {
      HIP_TRY(hipMemcpyAsync(h->map_pts.p, out, (size_t)m * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
    }
    h->map_n = (size_t)m;
    if (n_out) *n_out = h->map_n;
  });
}

int ngicp_map_size(const ngicp_t* h, size_t* n) {
  if (!h || !n) return NGICP_ERR_ARG;
  *n = h->map_n;
  return NGICP_OK;
}

int ngicp_map_get(ngicp_t* h, float* out_xyzi, size_t out_capacity) {
  return guarded(h, [&] {
    if (!out_xyzi) throw ArgError{NGICP_ERR_ARG, "null output"};
    if (h->map_n > out_capacity) throw ArgError{NGICP_ERR_ARG, "output buffer too small for the map"};
    download_xyzi(h, h->map_pts.as<float4>(), h->map_n, out_xyzi);
  });
}

int ngicp_map_clear(ngicp_t* h) {
  return guarded(h, [&] { h->map_n = 0; });
}

}  // extern "C"
