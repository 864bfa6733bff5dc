// C-ABI implementation (include/ngicp.h) — host driver for the HIP kernels.
// One handle == one nano_gicp::NanoGICP instance (/root/reference/include/nano_gicp/nano_gicp.hpp:58-137).
// One translation unit: the handle is in ngicp_handle.h, the voxel-map builds in ngicp_voxelmap.h, the rolling voxel map in ngicp_rollmap.h, the registration loops in ngicp_align.h; here
// are the index build, the covariances, the queries' host helpers and the extern "C" surface.
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

#include "ngicp_route.h"
#include "ngicp_pass.h"
#include "ngicp_cloudops.h"
#include "ngicp_filters.h"
#include "ngicp_query.h"
#include "ngicp_range.h"
#include "ngicp_batch.h"
#include "ngicp_voxel.h"
#include "ngicp_voxel_batch.h"
#include "ngicp_voxel_roll.h"
#include "ngicp_voxel_ray.h"
#include "ngicp_robust.h"

using namespace ngk;

#include "ngicp_handle.h"

namespace {

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
// (read at ngicp_create: ngicp::sw.cell_boxes; an index carries boxes when the handle that built it had the switch on)

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
      const double ratio = h->sw.target_occ / std::max(lam, 1.0);
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
  dc->has_boxes = h->sw.cell_boxes != 0;
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
      const double lam = (double)occ / (double)n, ratio = h->sw.target_occ / std::max(lam, 1.0);
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
  refuse_storage_only(dc, "inverse permutation");
  if (dc.has_inv) return;
  dc.inv_perm.ensure(dc.n * sizeof(int));
  hipLaunchKernelGGL(k_invert_perm, dim3((unsigned)((dc.n + 255) / 256)), dim3(256), 0, h->stream, dc.perm.as<int>(), (int)dc.n, dc.inv_perm.as<int>());
  dc.has_inv = true;
}

void ensure_slot_ready(ngicp* h, Slot& s, const char* what) {
  if (!s.present) throw ArgError{NGICP_ERR_STATE, std::string("no ") + what + " cloud set"};
  if (s.dev) {
    refuse_storage_only(*s.dev, what);  // (every search starts from a slot; no slot can hold such a cloud today)
    return;
  }
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
  refuse_storage_only(dc, "covariances");
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

// ------------------------------------------------------------------------------------------
// Voxelized GICP (ngicp_voxel.h): a mode the caller selects with ngicp_set_voxel_resolution
// ------------------------------------------------------------------------------------------
// The target, or its covariances, changed: the voxel map goes, and while the mode is on so do the correspondences, which are its voxel
// numbers (ngicp_get_correspondences would read the next map's records with them).  Exact GICP's correspondences are left as they were.
void drop_voxel_map(ngicp* h) {
  h->vmap.invalidate();
  if (h->voxel_res > 0.0) h->hook_valid = 0;
}

}  // namespace

#include "ngicp_voxelmap.h"
#include "ngicp_rollmap.h"
#include "ngicp_align.h"

namespace {

void check_batch_args(const char* entry, size_t n_guesses, const float* guesses, const float* T_out, const int* converged, const int* nr_iterations) {
  const std::string e(entry);
  if (n_guesses == 0) throw ArgError{NGICP_ERR_ARG, e + ": n_guesses is 0"};
  if (n_guesses > (size_t)NGICP_BATCH_MAX_LANES) throw ArgError{NGICP_ERR_ARG, e + ": more than NGICP_BATCH_MAX_LANES (64) guesses in one call"};
  if (!guesses) throw ArgError{NGICP_ERR_ARG, e + ": null guesses"};
  if (!T_out || !converged || !nr_iterations) throw ArgError{NGICP_ERR_ARG, e + ": null output"};
}

// the handle's results of the last alignment into the caller's arguments (any may be null)
void copy_results_out(const ngicp* h, float T_out[16], int* converged, int* nr_iterations, double final_hessian[36]) {
  if (T_out) std::memcpy(T_out, h->final_T, sizeof(h->final_T));
  if (converged) *converged = h->converged;
  if (nr_iterations) *nr_iterations = h->nr_iterations;
  if (final_hessian) std::memcpy(final_hessian, h->final_hessian, sizeof(h->final_hessian));
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
    HIP_TRY(hipEventCreate(&h->ev_rec_a));
    HIP_TRY(hipEventCreate(&h->ev_rec_b));
    HIP_TRY(hipEventCreate(&h->ev_vfit_a));
    HIP_TRY(hipEventCreate(&h->ev_vfit_b));
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
    std::memcpy(h->final_T, kIdentity16, sizeof(kIdentity16));
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
    h->sw = route::read_handle_switches(route::from_environment, kStageMaxGrow);
    h->persist = h->sw.persist;
    h->voxel_size = h->sw.voxel;
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
  if (h->ev_rec_a) (void)hipEventDestroy(h->ev_rec_a);
  if (h->ev_rec_b) (void)hipEventDestroy(h->ev_rec_b);
  if (h->ev_vfit_a) (void)hipEventDestroy(h->ev_vfit_a);
  if (h->ev_vfit_b) (void)hipEventDestroy(h->ev_vfit_b);
  if (h->sc.ev_a) (void)hipEventDestroy(h->sc.ev_a);
  if (h->sc.ev_b) (void)hipEventDestroy(h->sc.ev_b);
  for (hipEvent_t e : h->ps.ev)
    if (e) (void)hipEventDestroy(e);
  if (h->ev_kfm_a) (void)hipEventDestroy(h->ev_kfm_a);
  if (h->ev_kfm_b) (void)hipEventDestroy(h->ev_kfm_b);
  if (h->pg.ev_a) (void)hipEventDestroy(h->pg.ev_a);
  if (h->pg.ev_b) (void)hipEventDestroy(h->pg.ev_b);
  if (h->pg.pin) (void)hipHostFree(h->pg.pin);
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
      stream_wait_for(dst, src);
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
      stream_wait_for(dst, src);  // the covariance kernel / reorder src has enqueued
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
    if (aligned && (out_stride_bytes < 12 || out_stride_bytes % 4)) throw ArgError{NGICP_ERR_ARG, "bad out_stride_bytes"};
    if (h->voxel_res > 0.0) do_align_voxel(h, guess ? guess : kIdentity16, aligned, out_stride_bytes);
    else do_align(h, guess ? guess : kIdentity16, aligned, out_stride_bytes);
  });
  if (h) copy_results_out(h, T_out, converged, nr_iterations, final_hessian);
  return rc;
}

int ngicp_align_batch(ngicp_t* h, size_t n_guesses, const float* guesses, float* T_out, int* converged, int* nr_iterations, double* final_hessians) {
  return guarded(h, [&] {
    refuse_for(h, route::Entry::AlignBatch);
    check_batch_args("ngicp_align_batch", n_guesses, guesses, T_out, converged, nr_iterations);
    do_align_batch(h, (int)n_guesses, guesses, T_out, converged, nr_iterations, final_hessians);
  });
}

int ngicp_voxel_align_batch(ngicp_t* h, size_t n_guesses, const float* guesses, float* T_out, int* converged, int* nr_iterations, double* final_hessians) {
  return guarded(h, [&] {
    if (!(h->voxel_res > 0.0)) throw ArgError{NGICP_ERR_STATE, "ngicp_voxel_align_batch: the voxelized mode is off (ngicp_set_voxel_resolution)"};
    refuse_for(h, route::Entry::VoxelAlignBatch);
    check_batch_args("ngicp_voxel_align_batch", n_guesses, guesses, T_out, converged, nr_iterations);
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
      hipLaunchKernelGGL(k_fitness, dim3((unsigned)nb, (unsigned)m), dim3(kKnnBlock), 0, h->stream, S.pts(), np, w.fit_T.as<float>(), T.pts(), T.cells(), T.grid, max_range,
                         w.fit_part.as<double2>());
      hipLaunchKernelGGL(k_fitness_final, dim3((unsigned)m), dim3(kFitnessFinalBlock), 0, h->stream, w.fit_part.as<double2>(), nb, w.fit_out.as<double2>());
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
    HookCtx k;
    prepare_hook(h, k);
    LmState st;
    init_state_from_pose(st, pose_from_colmajor(T));
    HIP_TRY(hipMemcpyAsync(h->state.p, &st, sizeof(st), hipMemcpyHostToDevice, h->stream));
    launch_hook(h, k, 2 | 4, 1);
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
    HookCtx k;
    prepare_hook(h, k);
    // keep cur / have_lin, replace the trial pose (read in stream order: behind everything this handle has enqueued)
    LmState st;
    HIP_TRY(hipMemcpyAsync(&st, h->state.p, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const Pose x = pose_from_colmajor(T);
    st.hot.xi = x;
    for (int r = 0; r < 3; ++r) {
      for (int cc = 0; cc < 3; ++cc) st.xi_f[r * 4 + cc] = (float)x.R[r * 3 + cc];
      st.xi_f[r * 4 + 3] = (float)x.t[r];
    }
    HIP_TRY(hipMemcpyAsync(h->state.p, &st, sizeof(st), hipMemcpyHostToDevice, h->stream));
    launch_hook(h, k, 1 | 4, 2);
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
                         voxel_map_view(h).rec, h->knn_idx.as<int>(), sqd_out ? h->knn_d2.as<float>() : nullptr, dst->hot.lin_f);
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
    roll_clear(h);         // the rolling map's sums belong to one resolution (whether or not that setting is on)
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

int ngicp_set_robust_kernel(ngicp_t* h, int kind, double width) {
  return guarded(h, [&] {
    if (kind != NGICP_ROBUST_NONE && kind != NGICP_ROBUST_HUBER && kind != NGICP_ROBUST_CAUCHY && kind != NGICP_ROBUST_GEMAN_MCCLURE)
      throw ArgError{NGICP_ERR_ARG, "robust kernel: kind must be NGICP_ROBUST_NONE (0), _HUBER (1), _CAUCHY (2) or _GEMAN_MCCLURE (3)"};
    if (kind != NGICP_ROBUST_NONE && !(std::isfinite(width) && width > 0.0)) throw ArgError{NGICP_ERR_ARG, "robust kernel: the width must be finite and > 0"};
    h->robust_kind = kind;
    if (kind != NGICP_ROBUST_NONE) h->robust_width = width;  // (NONE has no width: the last one stays for ngicp_get_robust_kernel)
    // (the stored correspondences and matrices do not depend on the kernel: the hooks' state stays valid)
  });
}

int ngicp_get_robust_kernel(const ngicp_t* h, int* kind, double* width) {
  if (!h) return NGICP_ERR_ARG;
  if (kind) *kind = h->robust_kind;
  if (width) *width = h->robust_width;
  return NGICP_OK;
}

int ngicp_robust_terms(ngicp_t* h, const double T_colmajor[16], double* s_out, double* w_out, size_t capacity_doubles, int* K_out) {
  return guarded(h, [&] {
    if (!T_colmajor) throw ArgError{NGICP_ERR_ARG, "null pose"};
    if (!h->hook_valid) throw ArgError{NGICP_ERR_STATE, "no correspondences: call ngicp_linearize or ngicp_align first"};
    const bool vox = h->voxel_res > 0.0;
    const size_t n = h->src.dev->n, K = vox ? (size_t)h->voxel_nbr : 1;
    if (K_out) *K_out = (int)K;
    if (!s_out || !w_out) throw ArgError{NGICP_ERR_ARG, "null output"};
    if (capacity_doubles < n * K) throw ArgError{NGICP_ERR_ARG, "robust terms: an output holds fewer than n_src * K doubles"};
    LmState st;  // (in stream order, as ngicp_get_correspondences)
    HIP_TRY(hipMemcpyAsync(&st, h->state.p, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int cur = st.hot.cur & 1;
    h->robust_s.ensure(n * K * sizeof(double));
    h->robust_w.ensure(n * K * sizeof(double));
    RobustTermsArgs a{};
    if (vox) {
      const VoxelMapView vm = voxel_map_view(h);
      a.pts = h->src.dev->pts();
      a.corr = h->vox_corr[cur].as<int>();
      a.rec = vm.rec;
      a.n_vox = (int)vm.n_vox;
      a.mahal = K > 1 ? h->vox_mahal[cur].as<double>() : h->mahal[cur].as<double>();
    } else {
      a.pts = h->src.dev->qpts.as<float4>();
      a.src_sorted = h->src.dev->pts();
      a.tpt = h->tpt[cur].as<float4>();
      a.mahal = h->mahal[cur].as<double>();
    }
    a.n = (int)n;
    a.K = (int)K;
    a.slot_stride = (int)n;
    a.T = pose_from_colmajor(T_colmajor);
    fill_robust(h, a.kind, a.c, a.c2);
    a.out_s = h->robust_s.as<double>();
    a.out_w = h->robust_w.as<double>();
    if (n) hipLaunchKernelGGL(k_robust_terms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, a);
    if (n) HIP_TRY(hipMemcpyAsync(s_out, h->robust_s.p, n * K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (n) HIP_TRY(hipMemcpyAsync(w_out, h->robust_w.p, n * K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
  });
}

int ngicp_set_pose_prior(ngicp_t* h, const double T_prior_colmajor[16], const double info_colmajor[36]) {
  return guarded(h, [&] {
    if (!T_prior_colmajor) {  // clear
      h->prior_set = false;
      return;
    }
    if (!info_colmajor) throw ArgError{NGICP_ERR_ARG, "pose prior: null information matrix"};
    const double* T = T_prior_colmajor;
    const double* I = info_colmajor;
    for (int i = 0; i < 16; ++i)
      if (!std::isfinite(T[i])) throw ArgError{NGICP_ERR_ARG, "pose prior: the pose has a non-finite entry"};
    for (int i = 0; i < 36; ++i)
      if (!std::isfinite(I[i])) throw ArgError{NGICP_ERR_ARG, "pose prior: the information matrix has a non-finite entry"};
    if (T[3] != 0.0 || T[7] != 0.0 || T[11] != 0.0 || T[15] != 1.0) throw ArgError{NGICP_ERR_ARG, "pose prior: the pose's last row must be (0, 0, 0, 1)"};
    for (int r = 0; r < 6; ++r) {
      if (I[r * 6 + r] < 0.0) throw ArgError{NGICP_ERR_ARG, "pose prior: the information matrix has a negative diagonal entry"};
      for (int c = r + 1; c < 6; ++c)
        if (I[c * 6 + r] != I[r * 6 + c]) throw ArgError{NGICP_ERR_ARG, "pose prior: the information matrix must be exactly symmetric"};
    }
    double rec[kPriorDoubles];
    const Pose p = pose_from_colmajor(T);
    for (int i = 0; i < 9; ++i) rec[i] = p.R[i];
    for (int i = 0; i < 3; ++i) rec[9 + i] = p.t[i];
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) rec[12 + r * 6 + c] = I[c * 6 + r];
    // (in stream order behind everything this handle has enqueued; the copy has left `rec` when the call returns)
    h->prior_dev.ensure(sizeof(rec));
    HIP_TRY(hipMemcpyAsync(h->prior_dev.p, rec, sizeof(rec), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::memcpy(h->prior_T, T, sizeof(h->prior_T));
    std::memcpy(h->prior_info, I, sizeof(h->prior_info));
    h->prior_set = true;
    // (the stored correspondences and matrices do not depend on the prior: the hooks' state stays valid)
  });
}

int ngicp_get_pose_prior(const ngicp_t* h, int* set, double T_prior_colmajor[16], double info_colmajor[36]) {
  if (!h) return NGICP_ERR_ARG;
  if (set) *set = h->prior_set ? 1 : 0;
  if (h->prior_set && T_prior_colmajor) std::memcpy(T_prior_colmajor, h->prior_T, sizeof(h->prior_T));
  if (h->prior_set && info_colmajor) std::memcpy(info_colmajor, h->prior_info, sizeof(h->prior_info));
  return NGICP_OK;
}

int ngicp_pose_prior_terms(ngicp_t* h, const double T_colmajor[16], double r[6], double* cost, double H[36], double b[6]) {
  return guarded(h, [&] {
    if (!T_colmajor) throw ArgError{NGICP_ERR_ARG, "null pose"};
    if (!h->prior_set) throw ArgError{NGICP_ERR_STATE, "no pose prior set (ngicp_set_pose_prior)"};
    double out[kPriorRowSums + 6];
    h->prior_out.ensure(sizeof(out));
    hipLaunchKernelGGL(k_prior_terms, dim3(1), dim3(64), 0, h->stream, pose_from_colmajor(T_colmajor), h->prior_dev.as<double>(), h->prior_out.as<double>());
    HIP_TRY(hipMemcpyAsync(out, h->prior_out.p, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    if (H)
      for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) H[i * 6 + j] = H[j * 6 + i] = out[tri21(i, j)];
    if (b) std::memcpy(b, out + 21, 6 * sizeof(double));
    if (cost) *cost = out[27];
    if (r) std::memcpy(r, out + kPriorRowSums, 6 * sizeof(double));
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
    *n_voxels = ensure_voxel_map(h).n_vox;
  });
}

int ngicp_voxelmap_get(ngicp_t* h, int* ijk_n3, double* mean_n3, double* cov_n6, int* count_n) {
  return guarded(h, [&] {
    if (!(h->voxel_res > 0.0)) throw ArgError{NGICP_ERR_STATE, "no voxel resolution set (ngicp_set_voxel_resolution)"};
    const VoxelMapView vm = ensure_voxel_map(h);
    const size_t nv = vm.n_vox;
    std::vector<double> rec(nv * kVoxRec);
    std::vector<unsigned long long> keys(nv);
    HIP_TRY(hipMemcpyAsync(rec.data(), vm.rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(keys.data(), vm.vkeys, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
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

// ---- the rolling voxel map (include/ngicp.h "rolling voxel map"; ngicp_rollmap.h) ----
int ngicp_set_voxel_rolling(ngicp_t* h, int on) {
  return guarded(h, [&] {
    const int v = on ? 1 : 0;
    if (v == h->voxel_roll) return;
    h->voxel_roll = v;  // (both maps stay as they are: the entries read the other one from now on)
    h->hook_valid = 0;  // the correspondences number the other map's voxels
  });
}

int ngicp_get_voxel_rolling(const ngicp_t* h, int* on) {
  if (!h || !on) return NGICP_ERR_ARG;
  *on = h->voxel_roll;
  return NGICP_OK;
}

int ngicp_voxel_rolling_insert(ngicp_t* h, ngicp_t* from, const float T_colmajor[16], size_t* n_new, size_t* n_touched) {
  if (!from) return NGICP_ERR_ARG;
  return guarded(h, [&] {
    if (!T_colmajor) throw ArgError{NGICP_ERR_ARG, "null transform"};
    roll_insert(h, from, T_colmajor, n_new, n_touched);
  });
}

int ngicp_voxel_rolling_evict(ngicp_t* h, const float centre[3], double max_dist, long long min_stamp, size_t* n_removed) {
  return guarded(h, [&] { roll_evict(h, centre, max_dist, min_stamp, n_removed); });
}

int ngicp_voxel_rolling_clear(ngicp_t* h) {
  return guarded(h, [&] { roll_clear(h); });
}

int ngicp_voxel_rolling_get(ngicp_t* h, size_t* n_vox, int* ijk_n3, double* sum_n3, double* covsum_n6, int* count_n, long long* stamp_n) {
  return guarded(h, [&] {
    const ngicp::RollMap& r = h->roll;
    const size_t nv = r.n_vox;
    if (n_vox) *n_vox = nv;
    if ((!ijk_n3 && !sum_n3 && !covsum_n6 && !count_n && !stamp_n) || nv == 0) return;
    std::vector<double> sums(nv * kVoxRec);
    std::vector<unsigned long long> keys(nv);
    std::vector<long long> stamps(nv);
    HIP_TRY(hipMemcpyAsync(sums.data(), r.sums.p, sums.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(keys.data(), r.vkeys.p, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(stamps.data(), r.stamps.p, stamps.size() * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    for (size_t v = 0; v < nv; ++v) {
      if (ijk_n3) {
        ijk_n3[3 * v + 0] = (int)(keys[v] & 0x1fffffull) - kVoxBias;
        ijk_n3[3 * v + 1] = (int)((keys[v] >> 21) & 0x1fffffull) - kVoxBias;
        ijk_n3[3 * v + 2] = (int)((keys[v] >> 42) & 0x1fffffull) - kVoxBias;
      }
      if (sum_n3) std::memcpy(sum_n3 + 3 * v, &sums[v * kVoxRec], 3 * sizeof(double));
      if (covsum_n6) std::memcpy(covsum_n6 + 6 * v, &sums[v * kVoxRec + 3], 6 * sizeof(double));
      if (count_n) count_n[v] = (int)sums[v * kVoxRec + 9];
      if (stamp_n) stamp_n[v] = stamps[v];
    }
  });
}

int ngicp_voxel_rolling_stats(const ngicp_t* h, long long* inserts, size_t* n_vox, size_t* capacity_vox, size_t* table_slots, double* last_insert_ms, double* last_evict_ms) {
  if (!h) return NGICP_ERR_ARG;
  if (last_insert_ms) roll_resolve_time(const_cast<ngicp_t*>(h), true);  // (a record insert's commit is left in the stream: its time is read here)
  if (inserts) *inserts = h->roll.inserts;
  if (n_vox) *n_vox = h->roll.n_vox;
  if (capacity_vox) *capacity_vox = h->roll.cap;
  if (table_slots) *table_slots = h->roll.slots;
  if (last_insert_ms) *last_insert_ms = h->roll.last_insert_ms;
  if (last_evict_ms) *last_evict_ms = h->roll.last_evict_ms;
  return NGICP_OK;
}

// ---- the rolling map from voxel records (include/ngicp.h "rolling voxel map: records"; ngicp_voxel_roll.h) ----
int ngicp_voxel_rolling_set(ngicp_t* h, size_t n_vox, const int* ijk_n3, const double* sum_n3, const double* covsum_n6, const int* count_n, const long long* stamp_n, long long inserts) {
  return guarded(h, [&] { roll_set(h, n_vox, ijk_n3, sum_n3, covsum_n6, count_n, stamp_n, inserts); });
}

int ngicp_voxel_rolling_insert_voxels(ngicp_t* h, size_t n_rec, const double* sum_n3, const double* covsum_n6, const int* count_n, const float T_colmajor[16], size_t* n_new,
                                      size_t* n_touched) {
  return guarded(h, [&] { roll_insert_voxels(h, n_rec, sum_n3, covsum_n6, count_n, T_colmajor, n_new, n_touched); });
}

int ngicp_voxel_rolling_insert_map(ngicp_t* h, ngicp_t* from, const float T_colmajor[16], size_t* n_new, size_t* n_touched) {
  if (!from) return NGICP_ERR_ARG;
  return guarded(h, [&] { roll_insert_map(h, from, T_colmajor, n_new, n_touched); });
}

int ngicp_voxel_rolling_transform(ngicp_t* h, const float T_colmajor[16], size_t* n_vox_after) {
  return guarded(h, [&] { roll_transform(h, T_colmajor, n_vox_after); });
}

// ---- clearing the rolling map along a scan's rays (include/ngicp.h "rolling voxel map: clearing along rays"; ngicp_voxel_ray.h) ----
int ngicp_voxel_rolling_ray_clear(ngicp_t* h, ngicp_t* from, const float T_colmajor[16], const float* origin_or_null, const ngicp_ray_clear_options* options_or_null,
                                  ngicp_ray_clear_result* result_out) {
  if (!from) return NGICP_ERR_ARG;
  return guarded(h, [&] { roll_ray_clear(h, from, T_colmajor, origin_or_null, options_or_null, result_out); });
}

int ngicp_voxel_rolling_ray_counts(ngicp_t* h, uint32_t* miss_n, uint32_t* hit_n, size_t capacity, size_t* n_out) {
  return guarded(h, [&] { roll_ray_counts(h, miss_n, hit_n, capacity, n_out); });
}

// ---- the gated insert into the rolling map (include/ngicp.h "rolling voxel map: gated insert"; ngicp_voxel_gate.h) ----
int ngicp_voxel_rolling_insert_gated(ngicp_t* h, ngicp_t* from, const float T_colmajor[16], const ngicp_gate_options* options_or_null, ngicp_gate_result* result_out) {
  if (!from) return NGICP_ERR_ARG;
  return guarded(h, [&] { roll_insert_gated(h, from, T_colmajor, options_or_null, result_out); });
}

int ngicp_voxel_rolling_insert_classes(ngicp_t* h, uint8_t* cls_n, size_t capacity, size_t* n_out) {
  return guarded(h, [&] { roll_gate_classes(h, cls_n, capacity, n_out); });
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
    hipLaunchKernelGGL(k_fitness, dim3((unsigned)nb, 1u), dim3(kKnnBlock), 0, h->stream, S.pts(), n, h->fit_T.as<float>(), T.pts(), T.cells(), T.grid, max_range,
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
    refuse_for(h, route::Entry::ShardedBegin);
    h->shard_ctx.reset(new LoopCtx);
    LoopCtx& c = *h->shard_ctx;
    prepare_loop(h, c);
    set_pass_mode(h, c.pa);
    allow_k4_only_passes(h, c, route_facts(h, route::Caller::Sharded));  // (every rank steps the same lm_step on the same reduced sums: the word is the same on all of them)
    upload_initial_state(h, guess ? guess : kIdentity16);
    HIP_TRY(hipStreamSynchronize(h->stream));  // once per alignment: the caller may step on a stream of its own
    for (int i = 0; i < kShardSlots; ++i) h->h_shard_done[i] = 0;
    h->shard_steps = 0;
    h->sharded_active = true;
    h->hook_valid = 0;
  });
}

int ngicp_sharded_pass(ngicp_t* h, double* sums32_dev, void* stream_or_null) {
  return guarded(h, [&] {
    refuse_for(h, route::Entry::ShardedPass);
    if (!h->sharded_active || !h->shard_ctx) throw ArgError{NGICP_ERR_STATE, "ngicp_sharded_begin not called"};
    if (!sums32_dev) throw ArgError{NGICP_ERR_ARG, "null sums buffer"};
    hipStream_t s = stream_or_null ? (hipStream_t)stream_or_null : h->stream;
    LoopCtx& c = *h->shard_ctx;
    launch_pass(h, c.pa, pass_variant(h, route::Caller::Sharded, c.nblocks), c.nblocks, s);
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
    refuse_for(h, route::Entry::ShardedStep);
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
    refuse_for(h, route::Entry::ShardedFinish);
    if (!h->sharded_active) throw ArgError{NGICP_ERR_STATE, "ngicp_sharded_begin not called"};
    hipStream_t s = h->shard_stream ? h->shard_stream : h->stream;  // the steps were enqueued there
    HIP_TRY(hipMemcpyAsync(&h->pin_state[1], h->state.p, sizeof(LmState), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    store_result(h->pin_state[1].hot, h->final_T, &h->converged, &h->nr_iterations, h->final_hessian);
    copy_results_out(h, T_out, converged, nr_iterations, final_hessian);
    h->stats.passes = h->pin_state[1].hot.passes;  // (the stepped alignment's counts; the other fields stay the last ngicp_align's)
    h->stats.search_passes = h->pin_state[1].hot.search_passes;
    h->stats.lm_trials = h->pin_state[1].hot.n_trace;
    h->sharded_active = false;
    h->shard_ctx.reset();
    h->shard_stream = nullptr;
  });
}

// ---- K1 sharded over ranks: every rank computes a block of the packed covariance array, the caller all-gathers ----
int ngicp_covs_shard_begin(ngicp_t* h, int which, double** covs6_dev, size_t* n_points) {
  return guarded(h, [&] {
    refuse_for(h, route::Entry::CovsShardBegin);
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
    refuse_for(h, route::Entry::CovsShardCompute);
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
    refuse_for(h, route::Entry::CovsShardCommit);
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
    h->submap_moved = false;
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
        std::equal(h->submap_ids.begin(), h->submap_ids.end(), ids) && h->tgt_covs.n == total && !h->submap_moved)
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
    h->submap_moved = false;
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
    download_transformed(h, *h->tgt.dev, kIdentity16, xyz_out, out_stride_bytes);
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
    static const int kIn[6] = {3, 42, 6, 6, 9, 12 + kPriorDoubles}, kOut[6] = {9, 6, 12, 6, 3, kPriorRowSums};
    if (which < 0 || which > 5 || !in || !out) throw ArgError{NGICP_ERR_ARG, "bad arguments"};
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

// ---- test hook: one optimiser step, serial and wave form (k_step_selftest) ----
int ngicp_step_selftest(ngicp_t* h, const double* in, size_t n_problems, unsigned char* out_or_null, size_t* record_bytes) {
  return guarded(h, [&] {
    if (record_bytes) *record_bytes = kStepSelftestRecord;
    if (!out_or_null) return;
    if (!in || n_problems > (size_t)1 << 20) throw ArgError{NGICP_ERR_ARG, "bad arguments"};
    if (n_problems == 0) return;
    DevBuf di, dout;
    const size_t in_bytes = n_problems * kStepSelftestIn * sizeof(double), out_bytes = n_problems * 2 * kStepSelftestRecord;
    di.ensure(in_bytes);
    dout.ensure(out_bytes);
    HIP_TRY(hipMemcpyAsync(di.p, in, in_bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(dout.p, 0, out_bytes, h->stream));
    hipLaunchKernelGGL(k_step_selftest, dim3((unsigned)n_problems), dim3(64), 0, h->stream, di.as<double>(), (int)n_problems, dout.as<unsigned char>());
    HIP_TRY(hipMemcpyAsync(out_or_null, dout.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
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
#include "ngicp_deskew.h"  // (here, after every other kernel: the code object up to this point is laid out as it was without it)
#include "ngicp_voxel_fitness.h"  // (and this one behind it, for the same reason)

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

// ---- motion deskew (csrc/ngicp_deskew.h) ----
void deskew_check_pose(const double* T, const char* field) {
  for (int e = 0; e < 16; ++e)
    if (!std::isfinite(T[e])) throw ArgError{NGICP_ERR_ARG, std::string(field) + ": non-finite entry"};
  if (T[3] != 0.0 || T[7] != 0.0 || T[11] != 0.0 || T[15] != 1.0) throw ArgError{NGICP_ERR_ARG, std::string(field) + ": the last row must be (0, 0, 0, 1)"};
}

// Validates *d and the layout, uploads the cloud, its times and the trajectory, builds the table and runs k_deskew_unpack into `out`
// (device memory: n float4, or n x 3 floats when packed).  Nothing is enqueued before every argument has been accepted.
void deskew_upload_unpack(ngicp* h, const float* pts, size_t n, size_t stride, long intensity_off, const ngicp_deskew_t* d, bool packed, float* out) {
  if (!d) throw ArgError{NGICP_ERR_ARG, "d: null deskew description"};
  if (d->n_poses < 2 || d->n_poses > (size_t)NGICP_DESKEW_MAX_POSES) throw ArgError{NGICP_ERR_ARG, "n_poses must be between 2 and NGICP_DESKEW_MAX_POSES (256)"};
  if (!d->pose_times) throw ArgError{NGICP_ERR_ARG, "pose_times: null pointer"};
  if (!d->poses_colmajor) throw ArgError{NGICP_ERR_ARG, "poses_colmajor: null pointer"};
  const int M = (int)d->n_poses;
  for (int k = 0; k < M; ++k)
    if (!std::isfinite(d->pose_times[k]) || (k > 0 && !(d->pose_times[k] > d->pose_times[k - 1])))
      throw ArgError{NGICP_ERR_ARG, "pose_times must be finite and strictly ascending"};
  for (int k = 0; k < M; ++k) deskew_check_pose(d->poses_colmajor + (size_t)k * 16, "poses_colmajor");
  if (d->T_ref_colmajor) deskew_check_pose(d->T_ref_colmajor, "T_ref_colmajor");
  if (d->time_format != NGICP_TIME_F32_S && d->time_format != NGICP_TIME_F64_S && d->time_format != NGICP_TIME_U32_NS)
    throw ArgError{NGICP_ERR_ARG, "time_format: unknown format"};
  if (stride < 12 || stride % 4) throw ArgError{NGICP_ERR_ARG, "stride_bytes must be a multiple of 4 and >= 12"};
  if (intensity_off >= 0 && ((size_t)intensity_off + 4 > stride || intensity_off % 4)) throw ArgError{NGICP_ERR_ARG, "intensity offset outside the point stride"};
  if (n > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "cloud too large for int indices"};
  const size_t tsize = d->time_format == NGICP_TIME_F64_S ? 8 : 4;  // a time is read with one aligned load of its own size
  size_t record_end = intensity_off >= 0 ? std::max((size_t)12, (size_t)intensity_off + 4) : 12;
  DeskewTimes tm{};
  tm.format = d->time_format;
  tm.unit = d->time_format == NGICP_TIME_U32_NS ? 1e-9 : 1.0;
  tm.offset = d->time_offset;
  if (!d->times) {
    const long off = d->time_offset_bytes;
    if (off < 0 || (size_t)off % tsize || (size_t)off + tsize > stride || stride % tsize)
      throw ArgError{NGICP_ERR_ARG, "time_offset_bytes does not fit the point stride or the time format's size and alignment"};
    record_end = std::max(record_end, (size_t)off + tsize);
    tm.stride = stride;
    tm.first = (size_t)off;
  } else {
    if (d->time_stride_bytes < tsize || d->time_stride_bytes % tsize)
      throw ArgError{NGICP_ERR_ARG, "time_stride_bytes does not fit the time format's size and alignment"};
    tm.stride = d->time_stride_bytes;
    tm.first = 0;
  }
  const size_t raw_bytes = (n - 1) * stride + record_end;
  h->raw.ensure(raw_bytes);
  HIP_TRY(hipMemcpyAsync(h->raw.p, pts, raw_bytes, hipMemcpyHostToDevice, h->stream));
  tm.base = h->raw.as<unsigned char>();
  if (d->times) {
    const size_t time_bytes = (n - 1) * tm.stride + tsize;
    h->dsk_times.ensure(time_bytes);
    HIP_TRY(hipMemcpyAsync(h->dsk_times.p, d->times, time_bytes, hipMemcpyHostToDevice, h->stream));
    tm.base = h->dsk_times.as<unsigned char>();
  }
  std::vector<double>& in = h->dsk_host;
  in.resize((size_t)M * 17 + 16);
  std::copy(d->pose_times, d->pose_times + M, in.begin());
  std::copy(d->poses_colmajor, d->poses_colmajor + (size_t)M * 16, in.begin() + M);
  for (int e = 0; e < 16; ++e) in[(size_t)M * 17 + e] = d->T_ref_colmajor ? d->T_ref_colmajor[e] : (e % 5 == 0 ? 1.0 : 0.0);
  h->dsk_in.ensure(in.size() * sizeof(double));
  h->dsk_table.ensure(deskew_table_doubles(M) * sizeof(double));
  HIP_TRY(hipMemcpyAsync(h->dsk_in.p, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_deskew_prepare, dim3(1), dim3(kDeskewMaxPoses), 0, h->stream, h->dsk_in.as<double>(), M, h->dsk_table.as<double>());
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  const size_t lds = deskew_table_doubles(M) * sizeof(double);
  if (packed)
    hipLaunchKernelGGL((k_deskew_unpack<true>), grid, block, lds, h->stream, h->raw.as<unsigned char>(), stride, intensity_off, tm, h->dsk_table.as<double>(), M, (int)n, out);
  else
    hipLaunchKernelGGL((k_deskew_unpack<false>), grid, block, lds, h->stream, h->raw.as<unsigned char>(), stride, intensity_off, tm, h->dsk_table.as<double>(), M, (int)n, out);
  HIP_TRY(hipGetLastError());
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

// ---- motion deskew: the per-point pose of a trajectory applied where the scan is unpacked (csrc/ngicp_deskew.h) ----
int ngicp_deskew_cloud(ngicp_t* h, const float* pts, size_t n, size_t stride_bytes, const ngicp_deskew_t* d, float* xyz_out, size_t out_stride_bytes) {
  return guarded(h, [&] {
    if (n == 0) return;
    if (!pts || !xyz_out) throw ArgError{NGICP_ERR_ARG, "null pointer"};
    if (out_stride_bytes < 12 || out_stride_bytes % 4) throw ArgError{NGICP_ERR_ARG, "bad out_stride_bytes"};
    if (n > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "cloud too large for int indices"};
    h->out_xyz.ensure(n * 3 * sizeof(float));
    deskew_upload_unpack(h, pts, n, stride_bytes, -1, d, true, h->out_xyz.as<float>());
    download_xyz(h, n, xyz_out, out_stride_bytes);
  });
}

int ngicp_preprocess_scan_deskewed(ngicp_t* h, const float* pts, size_t n, size_t stride_bytes, long intensity_offset_bytes, const ngicp_deskew_t* d, int remove_nan,
                                   float crop_half_extent, float voxel_leaf, float* out_xyzi, size_t out_capacity, size_t* n_out) {
  return guarded(h, [&] {
    if (n_out) *n_out = 0;
    h->filt_out = nullptr;
    h->filt_n = 0;
    if (n == 0) return;
    if (!pts) throw ArgError{NGICP_ERR_ARG, "null cloud pointer"};
    if (n > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "cloud too large for int indices"};
    h->xyzi.ensure(n * sizeof(float4));
    deskew_upload_unpack(h, pts, n, stride_bytes, intensity_offset_bytes, d, false, h->xyzi.as<float>());
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

// ---- voxel fitness: poses scored against the voxel map the handle aligns against (csrc/ngicp_voxel_fitness.h) ----
namespace {

template <bool POINTS>
void launch_voxel_fitness(ngicp* h, const VoxelFitnessArgs& a, int nb, size_t poses) {
  const dim3 grid((unsigned)nb, (unsigned)poses), block(kVoxFitBlock);
  switch (h->voxel_nbr) {
    case NGICP_VOX_DIRECT1: hipLaunchKernelGGL((k_voxel_fitness<1, POINTS>), grid, block, 0, h->stream, a); break;
    case NGICP_VOX_DIRECT7: hipLaunchKernelGGL((k_voxel_fitness<7, POINTS>), grid, block, 0, h->stream, a); break;
    default: hipLaunchKernelGGL((k_voxel_fitness<27, POINTS>), grid, block, 0, h->stream, a); break;
  }
}

// n poses -> out[n]; with per-point outputs (n == 1) also m, d, v of every source point.  Everything the caller passed is checked before
// anything is enqueued; then the source, the map (at most one build) and the source's covariances are readied in align's order.  Reads
// and writes nothing of the hooks' state, of the last align's results and stats or of the batch workspace.
void voxel_fitness_impl(ngicp* h, const std::string& e, size_t n, const float* T_colmajor, double max_m, ngicp_voxel_fitness_t* out, double* pt_m, double* pt_d, int* pt_v,
                        size_t capacity) {
  const bool points = pt_m || pt_d || pt_v;
  if (!(h->voxel_res > 0.0)) throw ArgError{NGICP_ERR_STATE, e + ": the voxelized mode is off (ngicp_set_voxel_resolution)"};
  if (n == 0) throw ArgError{NGICP_ERR_ARG, e + ": n is 0"};
  if (!T_colmajor) throw ArgError{NGICP_ERR_ARG, e + ": null transforms"};
  if (!(max_m >= 0.0)) throw ArgError{NGICP_ERR_ARG, e + ": max_mahalanobis must be >= 0 and not NaN"};
  if (points ? !(pt_m && pt_d && pt_v) : !out) throw ArgError{NGICP_ERR_ARG, e + ": null output"};
  if (points && capacity < h->src.n) throw ArgError{NGICP_ERR_ARG, e + ": the outputs hold fewer than n_src entries"};
  ensure_slot_ready(h, h->src, "source");
  const VoxelMapView vm = ensure_voxel_map(h);
  if (h->src_covs.n != h->src.dev->n) compute_covs(h, h->src, h->src_covs, "source");
  DeviceCloud& S = *h->src.dev;
  const int np = (int)S.n;
  const int nb = std::max(1, (np + kVoxFitBlock - 1) / kVoxFitBlock);
  const size_t chunk = std::min(n, (size_t)kVoxelFitnessChunk);
  h->vfit_T.ensure(chunk * 16 * sizeof(float));
  h->vfit_part.ensure(chunk * (size_t)nb * kVoxFitSums * sizeof(double));
  h->vfit_out.ensure(chunk * kVoxFitSums * sizeof(double));
  VoxelFitnessArgs a{};
  a.src = S.pts();
  a.cov_src = covs_for(h, h->src_covs, h->src.dev);
  a.n_src = np;
  a.table = vm.table;
  a.mask = vm.mask;
  a.rec = vm.rec;
  a.inv_res = 1.0f / (float)h->voxel_res;
  a.T_colmajor = h->vfit_T.as<float>();
  a.max_m = max_m;
  a.partials = h->vfit_part.as<double>();
  if (points) {
    h->vfit_pts.ensure((size_t)np * (2 * sizeof(double) + sizeof(int)));
    a.pt_m = h->vfit_pts.as<double>();
    a.pt_d = a.pt_m + np;
    a.pt_v = reinterpret_cast<int*>(a.pt_d + np);
  }
  std::vector<double> r(n * kVoxFitSums);
  double kernel_ms = 0.0;
  for (size_t at = 0; at < n; at += chunk) {
    const size_t m = std::min(chunk, n - at);
    HIP_TRY(hipMemcpyAsync(h->vfit_T.p, T_colmajor + at * 16, m * 16 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->ev_vfit_a, h->stream));
    if (points) launch_voxel_fitness<true>(h, a, nb, m);
    else launch_voxel_fitness<false>(h, a, nb, m);
    hipLaunchKernelGGL((k_voxel_fitness_final<kVoxFitSums>), dim3((unsigned)m), dim3(kVoxFitFinalBlock), 0, h->stream, (const double*)h->vfit_part.as<double>(), nb, h->vfit_out.as<double>());
    HIP_TRY(hipEventRecord(h->ev_vfit_b, h->stream));
    HIP_TRY(hipMemcpyAsync(r.data() + at * kVoxFitSums, h->vfit_out.p, m * kVoxFitSums * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev_vfit_a, h->ev_vfit_b));
    kernel_ms += ms;
  }
  if (points && np) {
    HIP_TRY(hipMemcpyAsync(pt_m, a.pt_m, (size_t)np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(pt_d, a.pt_d, (size_t)np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(pt_v, a.pt_v, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  HIP_TRY(hipGetLastError());
  h->vfit_kernel_ms = kernel_ms;
  for (size_t i = 0; out && i < n; ++i) {
    const double* s = r.data() + i * kVoxFitSums;
    const bool any = s[2] > 0.0;
    out[i].mahalanobis = any ? s[0] / s[2] : std::numeric_limits<double>::max();
    out[i].sqdist = any ? s[1] / s[2] : std::numeric_limits<double>::max();
    out[i].n_inliers = (size_t)s[2];
    out[i].n_matched = (size_t)s[3];
  }
}

}  // namespace

extern "C" {

int ngicp_voxel_fitness(ngicp_t* h, const float T_colmajor[16], double max_mahalanobis, ngicp_voxel_fitness_t* out) {
  return guarded(h, [&] { voxel_fitness_impl(h, "ngicp_voxel_fitness", 1, T_colmajor ? T_colmajor : h->final_T, max_mahalanobis, out, nullptr, nullptr, nullptr, 0); });
}

int ngicp_voxel_fitness_batch(ngicp_t* h, size_t n, const float* T_colmajor, double max_mahalanobis, ngicp_voxel_fitness_t* out) {
  return guarded(h, [&] { voxel_fitness_impl(h, "ngicp_voxel_fitness_batch", n, T_colmajor, max_mahalanobis, out, nullptr, nullptr, nullptr, 0); });
}

int ngicp_voxel_fitness_points(ngicp_t* h, const float T_colmajor[16], double* m_out, double* sqd_out, int* voxel_out, size_t capacity) {
  return guarded(h, [&] {
    if (!m_out || !sqd_out || !voxel_out) throw ArgError{NGICP_ERR_ARG, "ngicp_voxel_fitness_points: null output"};
    voxel_fitness_impl(h, "ngicp_voxel_fitness_points", 1, T_colmajor ? T_colmajor : h->final_T, std::numeric_limits<double>::max(), nullptr, m_out, sqd_out, voxel_out, capacity);
  });
}

int ngicp_voxel_fitness_kernel_ms(const ngicp_t* h, double* ms) {
  if (!h || !ms) return NGICP_ERR_ARG;
  *ms = h->vfit_kernel_ms;
  return NGICP_OK;
}

}  // extern "C"

// ---- scan context place recognition: descriptors, their database, matching (csrc/ngicp_scan_context.h) ----
#include "ngicp_scan_context.h"  // (kernels and entries; behind everything else, so that the code object up to here is laid out as it was)

// ---- voxel pose search: a lattice of poses scored by occupied-voxel hits, the best few returned (csrc/ngicp_pose_search.h) ----
#include "ngicp_pose_search.h"  // (kernels and entries; behind everything else, for the same reason)

// ---- moving keyframes after a loop closure, and reading one back (csrc/ngicp_keyframe_move.h) ----
#include "ngicp_keyframe_move.h"  // (kernels and entries; behind everything else, for the same reason)

#include "ngicp_pose_graph.h"  // (kernels and entries; behind everything else, for the same reason)

// ---- the gated insert's kernels (csrc/ngicp_voxel_gate.h) and their launches, which roll_insert_gated (ngicp_rollmap.h) calls ----
#include "ngicp_voxel_gate.h"  // (behind everything else, for the same reason)

namespace {

void launch_roll_gate(ngicp* h, const RollGateArgs& a, const RollPose& P) {
  const dim3 grid((unsigned)((a.n + kGateBlock - 1) / kGateBlock)), block(kGateBlock);
  switch (h->voxel_nbr) {
    case NGICP_VOX_DIRECT1: hipLaunchKernelGGL((k_roll_gate<1>), grid, block, 0, h->stream, a, P); break;
    case NGICP_VOX_DIRECT7: hipLaunchKernelGGL((k_roll_gate<7>), grid, block, 0, h->stream, a, P); break;
    default: hipLaunchKernelGGL((k_roll_gate<27>), grid, block, 0, h->stream, a, P); break;
  }
}

void launch_roll_gate_scatter(ngicp* h, const int* keep, const int* rank, int n, const unsigned long long* keys_in, const int* vals_in, unsigned long long* keys, int* vals) {
  hipLaunchKernelGGL((k_roll_gate_scatter<1>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, keep, rank, n, keys_in, vals_in, keys, vals);
}

}  // namespace
