// The rolling voxel map's host code (ngicp_voxel_roll.h; include/ngicp.h "rolling voxel map"): insert, evict, clear and
// the growth of its arrays and table.  Part of ngicp_api.hip's translation unit (included there, after ngicp_voxelmap.h, whose
// size_voxel_work / voxel_segments number a scan's voxels).
#pragma once

namespace {

constexpr size_t kRollMinCap = 1024;  // voxels the per-voxel arrays start with
constexpr size_t kRollMinSlots = 64;  // (the target map's smallest table)

// A buffer of the rolling map to `bytes`, its first `live` bytes kept: DevBuf::ensure frees, so a new allocation, a device-to-device copy
// and only then the old one's release.  The caller's stream is idle or holds only work that the copy is ordered behind.
void roll_grow_keep(ngicp* h, DevBuf& b, size_t bytes, size_t live) {
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, bytes));
  g_device_allocs.fetch_add(1, std::memory_order_relaxed);
  if (b.p && live) {
    const hipError_t e = hipMemcpyAsync(p, b.p, live, hipMemcpyDeviceToDevice, h->stream);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
    if (e2 != hipSuccess) {
      (void)hipFree(p);
      throw HipError{e2, "rolling voxel map: growth copy", __FILE__, __LINE__};
    }
  }
  if (b.p) HIP_TRY(hipFree(b.p));
  b.p = p;
  b.cap = bytes;
}

// the per-voxel arrays for at least `need` voxels: capacity doubles, the live part moves
void roll_reserve(ngicp* h, size_t need) {
  ngicp::RollMap& r = h->roll;
  if (need <= r.cap) return;
  size_t cap = std::max(r.cap, kRollMinCap);
  while (cap < need) cap <<= 1;
  roll_grow_keep(h, r.sums, cap * kVoxRec * sizeof(double), r.n_vox * kVoxRec * sizeof(double));
  roll_grow_keep(h, r.rec, cap * kVoxRec * sizeof(double), r.n_vox * kVoxRec * sizeof(double));
  roll_grow_keep(h, r.vkeys, cap * sizeof(unsigned long long), r.n_vox * sizeof(unsigned long long));
  roll_grow_keep(h, r.stamps, cap * sizeof(long long), r.n_vox * sizeof(long long));
  r.cap = cap;
}

// the table cleared and filled again from the key array (nothing is synchronised)
void roll_refill_table(ngicp* h) {
  ngicp::RollMap& r = h->roll;
  HIP_TRY(hipMemsetAsync(r.table.p, 0xff, r.slots * sizeof(ulonglong2), h->stream));
  if (r.n_vox)
    hipLaunchKernelGGL(k_roll_table_fill, dim3((unsigned)((r.n_vox + 255) / 256)), dim3(256), 0, h->stream, (const unsigned long long*)r.vkeys.as<unsigned long long>(), (int)r.n_vox,
                       r.table.as<ulonglong2>(), (unsigned int)(r.slots - 1));
}

// A table that stays at most half full with `need` voxels: when it is too small (or not there yet) it is rebuilt at twice the size,
// as often as needed, from the key array.  true: it was rebuilt.
bool roll_reserve_table(ngicp* h, size_t need) {
  ngicp::RollMap& r = h->roll;
  if (r.slots && r.slots >= 2 * need) return false;
  size_t slots = std::max(r.slots, kRollMinSlots);
  while (slots < 2 * need) slots <<= 1;
  r.table.ensure(slots * sizeof(ulonglong2));  // (its contents are rebuilt, not kept)
  r.slots = slots;
  roll_refill_table(h);
  return true;
}

void roll_clear(ngicp* h) {
  h->roll.n_vox = 0;
  h->roll.inserts = 0;
  if (h->roll.slots) roll_refill_table(h);  // (memory stays with the handle)
  h->hook_valid = 0;
}

void roll_require_on(const ngicp* h, const char* entry) {
  if (!(h->voxel_res > 0.0)) throw ArgError{NGICP_ERR_STATE, std::string(entry) + ": no voxel resolution set (ngicp_set_voxel_resolution)"};
  if (!h->voxel_roll) throw ArgError{NGICP_ERR_STATE, std::string(entry) + ": the rolling setting is off (ngicp_set_voxel_rolling)"};
}

// Insert `from`'s source cloud at the float pose T.  Two host synchronisations: the scan's voxel count with the `bad` flag (the refusal,
// and what sizes the arrays and the table), and the number of new voxels behind the commit.  An insert that grows an array waits for
// that array's copy as well.
void roll_insert(ngicp* h, ngicp* from, const float T[16], size_t* n_new_out, size_t* n_touched_out) {
  roll_require_on(h, "ngicp_voxel_rolling_insert");
  if (h->device != from->device) throw ArgError{NGICP_ERR_ARG, "ngicp_voxel_rolling_insert across devices is not supported"};
  ensure_slot_ready(from, from->src, "source");
  // the covariances the producer holds for its source; computed now if absent, with the producer's k / regularisation (ngicp_keyframe_add)
  if (from->src_covs.n != from->src.dev->n) compute_covs(from, from->src, from->src_covs, "source");
  const double* covs = covs_for(from, from->src_covs, from->src.dev);  // in the cloud's own sorted order
  if (from != h) {  // the producer's stream may still be writing them: this handle's stream waits, on the device
    HIP_TRY(hipEventRecord(h->ev_fence, from->stream));
    HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_fence, 0));
  }
  const std::shared_ptr<DeviceCloud> cloud = from->src.dev;  // held until the last kernel that reads it has been waited for
  const std::shared_ptr<DevBuf> cov_hold = from->src_covs.data;
  ngicp::RollMap& r = h->roll;
  const int n = (int)cloud->n;
  if (n <= 0) throw ArgError{NGICP_ERR_ARG, "ngicp_voxel_rolling_insert: empty source cloud"};
  RollPose P;
  std::memcpy(P.m, T, sizeof(P.m));
  for (int row = 0; row < 3; ++row)
    for (int col = 0; col < 3; ++col) P.R[row * 3 + col] = (double)T[col * 4 + row];
  const float inv_res = 1.0f / (float)h->voxel_res;
  size_voxel_work(h, (size_t)n);
  h->roll_q.ensure((size_t)n * sizeof(float4));
  h->roll_sums.ensure((size_t)n * kVoxRec * sizeof(double));
  h->roll_hit.ensure((size_t)n * sizeof(int));
  HIP_TRY(hipEventRecord(h->ev_vox_a, h->stream));
  HIP_TRY(hipMemsetAsync(h->vox_flag.p, 0, sizeof(int), h->stream));
  hipLaunchKernelGGL(k_roll_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, cloud->pts(), n, P, inv_res, h->roll_q.as<float4>(),
                     h->vox_keys.as<unsigned long long>(), h->vox_vals.as<int>(), h->vox_flag.as<int>());
  const VoxelSegments sg = voxel_segments(h, n);
  int n_seg = 0, bad = 0;
  HIP_TRY(hipMemcpyAsync(&n_seg, sg.n_seg_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(&bad, h->vox_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  // the refusal comes before anything of the map is written: map, counter and stamps stay as they were
  if (bad)
    throw ArgError{NGICP_ERR_ARG, "rolling voxel map: a transformed point lies 2^20 voxels or more from the origin on some axis (or is not finite); nothing was inserted"};
  if (n_seg <= 0 || n_seg > n) throw ArgError{NGICP_ERR_HIP, "rolling voxel map insert: inconsistent voxel count"};
  // room for every scan voxel being new (an upper bound read back with the flag): the commit can then neither overrun an array nor fill
  // the table beyond half
  if (r.n_vox + (size_t)n_seg > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "rolling voxel map: too many voxels for int indices"};
  roll_reserve(h, r.n_vox + (size_t)n_seg);
  roll_reserve_table(h, r.n_vox + (size_t)n_seg);
  const unsigned blocks = (unsigned)((n_seg + 255) / 256);
  const int ntiles = (n_seg + kScanTile - 1) / kScanTile;
  int* is_new = h->vox_scan.as<int>();  // (voxel_segments' head and prefix arrays are free again; keys, order and seg_start are not)
  int* rank = is_new + n;               // n_seg + 1 + kCellPad <= n + 1 + kCellPad entries
  hipLaunchKernelGGL(k_roll_lookup, dim3(blocks), dim3(256), 0, h->stream, sg.keys, sg.order, sg.seg_start, n_seg, (const float4*)h->roll_q.as<float4>(), covs, P,
                     (const ulonglong2*)r.table.as<ulonglong2>(), (unsigned int)(r.slots - 1), h->roll_sums.as<double>(), h->roll_hit.as<int>(), is_new);
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(kScanBlock), 0, h->stream, (const int*)is_new, n_seg, h->tile_sums.as<int>(), (unsigned long long*)nullptr);
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(kScanBlock), 0, h->stream, h->tile_sums.as<int>(), ntiles, (const unsigned long long*)nullptr, (unsigned long long*)nullptr);
  hipLaunchKernelGGL(k_scan_apply, dim3(ntiles), dim3(kScanBlock), 0, h->stream, (const int*)is_new, n_seg, (const int*)h->tile_sums.as<int>(), rank);
  hipLaunchKernelGGL(k_roll_commit, dim3(blocks), dim3(256), 0, h->stream, sg.keys, sg.seg_start, n_seg, (const double*)h->roll_sums.as<double>(), (const int*)h->roll_hit.as<int>(),
                     (const int*)rank, (int)r.n_vox, r.inserts + 1, r.sums.as<double>(), r.rec.as<double>(), r.vkeys.as<unsigned long long>(), r.stamps.as<long long>(),
                     r.table.as<ulonglong2>(), (unsigned int)(r.slots - 1));
  HIP_TRY(hipEventRecord(h->ev_vox_b, h->stream));
  int n_new = 0;
  HIP_TRY(hipMemcpyAsync(&n_new, rank + n_seg, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  h->hook_valid = 0;  // (from here on the map is being written)
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  if (n_new < 0 || n_new > n_seg) throw ArgError{NGICP_ERR_HIP, "rolling voxel map insert: inconsistent count of new voxels"};
  r.n_vox += (size_t)n_new;
  ++r.inserts;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, h->ev_vox_a, h->ev_vox_b) == hipSuccess) r.last_insert_ms = ms;
  if (n_new_out) *n_new_out = (size_t)n_new;
  if (n_touched_out) *n_touched_out = (size_t)n_seg;
}

// Evict: flags, the scan, a stable compaction into the workspace, copies back, the table rebuilt.  One host synchronisation (the
// survivors' count).
void roll_evict(ngicp* h, const float centre[3], double max_dist, long long min_stamp, size_t* n_removed_out) {
  roll_require_on(h, "ngicp_voxel_rolling_evict");
  if (!centre) throw ArgError{NGICP_ERR_ARG, "ngicp_voxel_rolling_evict: null centre"};
  if (std::isnan(max_dist)) throw ArgError{NGICP_ERR_ARG, "ngicp_voxel_rolling_evict: max_dist is not a number"};
  ngicp::RollMap& r = h->roll;
  h->hook_valid = 0;
  if (n_removed_out) *n_removed_out = 0;
  const int n = (int)r.n_vox;
  if (n == 0) return;
  size_voxel_work(h, (size_t)n);
  const size_t rec_bytes = (size_t)n * kVoxRec * sizeof(double);
  h->roll_tmp.ensure(2 * rec_bytes + (size_t)n * 16);
  const unsigned blocks = (unsigned)((n + 255) / 256);
  const int ntiles = (n + kScanTile - 1) / kScanTile;
  int* keep = h->vox_scan.as<int>();
  int* rank = keep + n;  // n + 1 + kCellPad entries
  double* sums_o = h->roll_tmp.as<double>();
  double* rec_o = sums_o + (size_t)n * kVoxRec;
  unsigned long long* vkeys_o = reinterpret_cast<unsigned long long*>(rec_o + (size_t)n * kVoxRec);
  long long* stamps_o = reinterpret_cast<long long*>(vkeys_o + n);
  HIP_TRY(hipEventRecord(h->ev_vox_a, h->stream));
  hipLaunchKernelGGL(k_roll_evict_flags, dim3(blocks), dim3(256), 0, h->stream, (const unsigned long long*)r.vkeys.as<unsigned long long>(), (const long long*)r.stamps.as<long long>(), n,
                     h->voxel_res, (double)centre[0], (double)centre[1], (double)centre[2], max_dist, min_stamp, keep);
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(kScanBlock), 0, h->stream, (const int*)keep, n, h->tile_sums.as<int>(), (unsigned long long*)nullptr);
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(kScanBlock), 0, h->stream, h->tile_sums.as<int>(), ntiles, (const unsigned long long*)nullptr, (unsigned long long*)nullptr);
  hipLaunchKernelGGL(k_scan_apply, dim3(ntiles), dim3(kScanBlock), 0, h->stream, (const int*)keep, n, (const int*)h->tile_sums.as<int>(), rank);
  hipLaunchKernelGGL(k_roll_compact, dim3(blocks), dim3(256), 0, h->stream, (const int*)keep, (const int*)rank, n, (const double*)r.sums.as<double>(), (const double*)r.rec.as<double>(),
                     (const unsigned long long*)r.vkeys.as<unsigned long long>(), (const long long*)r.stamps.as<long long>(), sums_o, rec_o, vkeys_o, stamps_o);
  int n_keep = 0;
  HIP_TRY(hipMemcpyAsync(&n_keep, rank + n, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  if (n_keep < 0 || n_keep > n) throw ArgError{NGICP_ERR_HIP, "rolling voxel map evict: inconsistent count of survivors"};
  if (n_keep < n) {
    const size_t k = (size_t)n_keep;
    if (k) {
      HIP_TRY(hipMemcpyAsync(r.sums.p, sums_o, k * kVoxRec * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
      HIP_TRY(hipMemcpyAsync(r.rec.p, rec_o, k * kVoxRec * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
      HIP_TRY(hipMemcpyAsync(r.vkeys.p, vkeys_o, k * sizeof(unsigned long long), hipMemcpyDeviceToDevice, h->stream));
      HIP_TRY(hipMemcpyAsync(r.stamps.p, stamps_o, k * sizeof(long long), hipMemcpyDeviceToDevice, h->stream));
    }
    r.n_vox = k;
    roll_refill_table(h);
  }
  HIP_TRY(hipEventRecord(h->ev_vox_b, h->stream));
  HIP_TRY(hipEventSynchronize(h->ev_vox_b));  // (the time; the next alignment would wait for this work anyway)
  HIP_TRY(hipGetLastError());
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, h->ev_vox_a, h->ev_vox_b) == hipSuccess) r.last_evict_ms = ms;
  if (n_removed_out) *n_removed_out = (size_t)(n - n_keep);
}

}  // namespace
