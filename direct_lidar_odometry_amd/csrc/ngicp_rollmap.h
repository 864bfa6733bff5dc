// The rolling voxel map's host code (ngicp_voxel_roll.h; include/ngicp.h "rolling voxel map"): insert, evict, clear and the growth of its
// arrays and table; behind them the record routes: restore, insert of records, handle-to-handle insert,
// move in place; the clearing along a scan's rays (ngicp_voxel_ray.h), which shares the eviction's tail
// (roll_remove_unkept); and the gated insert (ngicp_voxel_gate.h), next to the plain one.
// Part of ngicp_api.hip's translation unit (included there, after ngicp_voxelmap.h, whose size_voxel_work / voxel_segments / read_count / exclusive_scan_flags number a scan's voxels).
#pragma once

namespace {

constexpr size_t kRollMinCap = 1024;  // voxels the per-voxel arrays start with

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
  const size_t slots = voxel_table_slots(need, r.slots);
  r.table.ensure(slots * sizeof(ulonglong2));  // (its contents are rebuilt, not kept)
  r.slots = slots;
  roll_refill_table(h);
  return true;
}

void roll_clear(ngicp* h) {
  h->roll.n_vox = 0;
  h->roll.inserts = 0;
  h->gate_valid = false;  // (the classes of the last gated insert are read up to here)
  if (h->roll.slots) roll_refill_table(h);  // (memory stays with the handle)
  h->hook_valid = 0;
  ++h->roll.gen;
}

void roll_require_on(const ngicp* h, const char* entry) {
  if (!(h->voxel_res > 0.0)) throw ArgError{NGICP_ERR_STATE, std::string(entry) + ": no voxel resolution set (ngicp_set_voxel_resolution)"};
  if (!h->voxel_roll) throw ArgError{NGICP_ERR_STATE, std::string(entry) + ": the rolling setting is off (ngicp_set_voxel_rolling)"};
}

RollPose roll_pose(const float T[16]) {
  RollPose P;
  std::memcpy(P.m, T, sizeof(P.m));
  for (int row = 0; row < 3; ++row)
    for (int col = 0; col < 3; ++col) P.R[row * 3 + col] = (double)T[col * 4 + row];
  return P;
}

// The commit of an insert's n_seg scan / destination voxels (sums in roll_sums, lookup results in roll_hit, ranks of the new ones in
// `rank`) onto the map from voxel `base` on; the stamp is the next insert's number, or seg_stamp[u] (the move in place).
void roll_launch_commit(ngicp* h, const VoxelSegments& sg, int n_seg, const int* rank, size_t base, const long long* seg_stamp) {
  ngicp::RollMap& r = h->roll;
  hipLaunchKernelGGL(k_roll_commit, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, h->stream, sg.keys, sg.seg_start, n_seg, (const double*)h->roll_sums.as<double>(),
                     (const int*)h->roll_hit.as<int>(), rank, (int)base, r.inserts + 1, seg_stamp, r.sums.as<double>(), r.rec.as<double>(), r.vkeys.as<unsigned long long>(),
                     r.stamps.as<long long>(), r.table.as<ulonglong2>(), (unsigned int)(r.slots - 1));
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
  if (from != h) stream_wait_for(h, from);  // the producer's stream may still be writing them
  const std::shared_ptr<DeviceCloud> cloud = from->src.dev;  // held until the last kernel that reads it has been waited for
  const std::shared_ptr<DevBuf> cov_hold = from->src_covs.data;
  ngicp::RollMap& r = h->roll;
  const int n = (int)cloud->n;
  if (n <= 0) throw ArgError{NGICP_ERR_ARG, "ngicp_voxel_rolling_insert: empty source cloud"};
  const RollPose P = roll_pose(T);
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
  const auto [n_seg, bad] = read_count(h, sg.n_seg_dev, true);
  // the refusal comes before anything of the map is written: map, counter and stamps stay as they were
  if (bad)
    throw ArgError{NGICP_ERR_ARG, "rolling voxel map: a transformed point lies 2^20 voxels or more from the origin on some axis (or is not finite); nothing was inserted"};
  if (n_seg <= 0 || n_seg > n) throw ArgError{NGICP_ERR_HIP, "rolling voxel map insert: inconsistent voxel count"};
  // room for every scan voxel being new (an upper bound read back with the flag): the commit can then neither overrun an array nor fill
  // the table beyond half
  if (r.n_vox + (size_t)n_seg > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "rolling voxel map: too many voxels for int indices"};
  roll_reserve(h, r.n_vox + (size_t)n_seg);
  roll_reserve_table(h, r.n_vox + (size_t)n_seg);
  int* is_new = h->vox_scan.as<int>();  // (voxel_segments' head and prefix arrays are free again; keys, order and seg_start are not)
  int* rank = is_new + n;               // n_seg + 1 + kCellPad <= n + 1 + kCellPad entries
  hipLaunchKernelGGL(k_roll_lookup, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, h->stream, sg.keys, sg.order, sg.seg_start, n_seg, (const float4*)h->roll_q.as<float4>(), covs,
                     P, (const ulonglong2*)r.table.as<ulonglong2>(), (unsigned int)(r.slots - 1), h->roll_sums.as<double>(), h->roll_hit.as<int>(), is_new);
  exclusive_scan_flags(h, is_new, n_seg, rank);
  roll_launch_commit(h, sg, n_seg, rank, r.n_vox, nullptr);
  HIP_TRY(hipEventRecord(h->ev_vox_b, h->stream));
  h->hook_valid = 0;
  ++h->roll.gen;  // (from here on the map is being written)
  const int n_new = read_count(h, rank + n_seg).count;
  if (n_new < 0 || n_new > n_seg) throw ArgError{NGICP_ERR_HIP, "rolling voxel map insert: inconsistent count of new voxels"};
  r.n_vox += (size_t)n_new;
  ++r.inserts;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, h->ev_vox_a, h->ev_vox_b) == hipSuccess) r.last_insert_ms = ms;
  h->rec_time_pending = false;  // (a record insert's time that nobody asked for is superseded)
  if (n_new_out) *n_new_out = (size_t)n_new;
  if (n_touched_out) *n_touched_out = (size_t)n_seg;
}

// ---- the gated insert (ngicp_voxel_gate.h; include/ngicp.h "rolling voxel map: gated insert") ----
// the two launches of its own; defined behind the kernels, at the end of ngicp_api.hip
void launch_roll_gate(ngicp* h, const RollGateArgs& a, const RollPose& P);
void launch_roll_gate_scatter(ngicp* h, const int* keep, const int* rank, int n, const unsigned long long* keys_in, const int* vals_in, unsigned long long* keys, int* vals);

// NULL options: no gate (max_mahalanobis has no default of its own; DBL_MAX keeps every judged point) and the defaults of include/ngicp.h
ngicp_gate_options roll_gate_defaults() {
  ngicp_gate_options o;
  o.max_mahalanobis = std::numeric_limits<double>::max();
  o.min_voxel_count = 1;
  o.insert_new = 1;
  o.insert_unjudged = 1;
  o.dry_run = 0;
  return o;
}

// Classify `from`'s source cloud against the map at the float pose T and insert the kept points as roll_insert inserts a scan.  Three
// host synchronisations, one more than roll_insert: FIRST the refusal flag (judged on every point), the class counts and the kept
// points' count in one read-back, behind the classification, the scan over the keep flags and the scatter, all of which write workspace
// only; then roll_insert's two - the kept points' voxel count, and the number of new voxels behind the commit.  Every refusal comes
// before the first write to the map.  The classes go into the array that does not hold the last accepted call's.
void roll_insert_gated(ngicp* h, ngicp* from, const float T[16], const ngicp_gate_options* opt, ngicp_gate_result* out) {
  const char* entry = "ngicp_voxel_rolling_insert_gated";
  roll_require_on(h, entry);
  if (!T) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": null transform"};
  const ngicp_gate_options o = opt ? *opt : roll_gate_defaults();
  if (!(o.max_mahalanobis >= 0.0) || std::isinf(o.max_mahalanobis))
    throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": max_mahalanobis must be >= 0 and finite (DBL_MAX: no gate)"};
  if (o.min_voxel_count < 1) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": min_voxel_count below 1"};
  if (h->device != from->device) throw ArgError{NGICP_ERR_ARG, std::string(entry) + " across devices is not supported"};
  if (!from->src.present) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": empty source cloud"};
  ensure_slot_ready(from, from->src, "source");
  if (from->src_covs.n != from->src.dev->n) compute_covs(from, from->src, from->src_covs, "source");  // (as roll_insert)
  const double* covs = covs_for(from, from->src_covs, from->src.dev);
  if (from != h) stream_wait_for(h, from);
  const std::shared_ptr<DeviceCloud> cloud = from->src.dev;  // held until the last kernel that reads it has been waited for
  const std::shared_ptr<DevBuf> cov_hold = from->src_covs.data;
  ngicp::RollMap& r = h->roll;
  const int n = (int)cloud->n;
  if (n <= 0) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": empty source cloud"};
  const RollPose P = roll_pose(T);
  // every buffer before the first launch: growing one waits for the device
  size_voxel_work(h, (size_t)n);
  h->roll_q.ensure((size_t)n * sizeof(float4));
  h->roll_sums.ensure((size_t)n * kVoxRec * sizeof(double));
  h->roll_hit.ensure((size_t)n * sizeof(int));
  DevBuf& cls = h->roll_gate_cls[1 - h->gate_cur];
  cls.ensure((size_t)n);
  h->roll_gate_cnt.ensure(4 * sizeof(int));
  unsigned long long* keys_a = h->vox_keys.as<unsigned long long>();  // (2 n entries: the uncompacted pairs go into the second half)
  int* vals_a = h->vox_vals.as<int>();
  int* keep = h->vox_scan.as<int>();  // (as roll_remove_unkept: flags, then n + 1 + kCellPad ranks; voxel_segments takes the buffer over behind the scatter)
  int* keep_rank = keep + n;
  const bool probe = r.slots && r.n_vox;
  RollGateArgs a{};
  a.pts = cloud->pts();
  a.covs = covs;
  a.n = n;
  a.inv_res = 1.0f / (float)h->voxel_res;
  a.table = probe ? (const ulonglong2*)r.table.as<ulonglong2>() : (const ulonglong2*)nullptr;
  a.mask = (unsigned int)(r.slots ? r.slots - 1 : 0);
  a.rec = r.rec.as<double>();
  a.max_m = o.max_mahalanobis;
  a.min_count = (double)o.min_voxel_count;
  a.keep_new = o.insert_new ? 1 : 0;
  a.keep_unjudged = o.insert_unjudged ? 1 : 0;
  a.qpts = h->roll_q.as<float4>();
  a.keys = keys_a + n;
  a.vals = vals_a + n;
  a.cls = cls.as<unsigned char>();
  a.keep = keep;
  a.counts = h->roll_gate_cnt.as<int>();
  a.bad = h->vox_flag.as<int>();
  HIP_TRY(hipEventRecord(h->ev_vox_a, h->stream));
  HIP_TRY(hipMemsetAsync(h->vox_flag.p, 0, sizeof(int), h->stream));
  HIP_TRY(hipMemsetAsync(h->roll_gate_cnt.p, 0, 4 * sizeof(int), h->stream));
  launch_roll_gate(h, a, P);
  if (!o.dry_run) {
    exclusive_scan_flags(h, keep, n, keep_rank);
    launch_roll_gate_scatter(h, keep, keep_rank, n, a.keys, a.vals, keys_a, vals_a);
  }
  HIP_TRY(hipEventRecord(h->ev_vox_b, h->stream));
  int counts[4] = {0, 0, 0, 0}, bad = 0, n_scan = -1;
  HIP_TRY(hipMemcpyAsync(counts, h->roll_gate_cnt.p, sizeof(counts), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(&bad, h->vox_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (!o.dry_run) HIP_TRY(hipMemcpyAsync(&n_scan, keep_rank + n, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  // the plain insert's refusal, judged on every point of the scan: map, counter, stamps and the last accepted call's classes stay
  if (bad)
    throw ArgError{NGICP_ERR_ARG, "rolling voxel map: a transformed point lies 2^20 voxels or more from the origin on some axis (or is not finite); nothing was inserted"};
  const int n_kept = counts[kGateExplained] + (a.keep_new ? counts[kGateNew] : 0) + (a.keep_unjudged ? counts[kGateUnjudged] : 0);
  if (counts[0] + counts[1] + counts[2] + counts[3] != n || (!o.dry_run && n_scan != n_kept)) throw ArgError{NGICP_ERR_HIP, std::string(entry) + ": inconsistent class counts"};
  h->gate_cur = 1 - h->gate_cur;
  h->gate_valid = true;
  h->gate_n = (size_t)n;
  float ms = 0.f, ms_tail = 0.f;
  bool timed = hipEventElapsedTime(&ms, h->ev_vox_a, h->ev_vox_b) == hipSuccess;
  size_t n_new_out = 0, n_touched_out = 0;
  if (!o.dry_run && n_kept > 0) {
    // ---- roll_insert from its numbering step on, over the n_kept pairs at the front of vox_keys / vox_vals ----
    HIP_TRY(hipEventRecord(h->ev_vox_a, h->stream));
    const VoxelSegments sg = voxel_segments(h, n_kept);
    const int n_seg = read_count(h, sg.n_seg_dev).count;
    if (n_seg <= 0 || n_seg > n_kept) throw ArgError{NGICP_ERR_HIP, std::string(entry) + ": inconsistent voxel count"};
    if (r.n_vox + (size_t)n_seg > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "rolling voxel map: too many voxels for int indices"};
    roll_reserve(h, r.n_vox + (size_t)n_seg);
    roll_reserve_table(h, r.n_vox + (size_t)n_seg);
    int* is_new = h->vox_scan.as<int>();  // (as roll_insert; the pairs number n_kept, so n_kept is what places the arrays)
    int* rank = is_new + n_kept;
    hipLaunchKernelGGL(k_roll_lookup, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, h->stream, sg.keys, sg.order, sg.seg_start, n_seg, (const float4*)h->roll_q.as<float4>(), covs,
                       P, (const ulonglong2*)r.table.as<ulonglong2>(), (unsigned int)(r.slots - 1), h->roll_sums.as<double>(), h->roll_hit.as<int>(), is_new);
    exclusive_scan_flags(h, is_new, n_seg, rank);
    roll_launch_commit(h, sg, n_seg, rank, r.n_vox, nullptr);
    HIP_TRY(hipEventRecord(h->ev_vox_b, h->stream));
    h->hook_valid = 0;
    ++h->roll.gen;  // (from here on the map is being written)
    const int n_new = read_count(h, rank + n_seg).count;
    if (n_new < 0 || n_new > n_seg) throw ArgError{NGICP_ERR_HIP, std::string(entry) + ": inconsistent count of new voxels"};
    r.n_vox += (size_t)n_new;
    ++r.inserts;
    timed = timed && hipEventElapsedTime(&ms_tail, h->ev_vox_a, h->ev_vox_b) == hipSuccess;
    if (timed) r.last_insert_ms = (double)ms + (double)ms_tail;
    h->rec_time_pending = false;
    n_new_out = (size_t)n_new;
    n_touched_out = (size_t)n_seg;
  }
  if (out) {
    out->n_points = (size_t)n;
    for (int k = 0; k < 4; ++k) out->n_class[k] = (size_t)counts[k];
    out->n_kept = (size_t)n_kept;
    out->n_new = n_new_out;
    out->n_touched = n_touched_out;
    out->kernel_ms = timed ? (double)ms + (double)ms_tail : 0.0;
  }
}

// the classes of the last accepted gated call, in the scan's original order
void roll_gate_classes(ngicp* h, unsigned char* cls_n, size_t capacity, size_t* n_out) {
  const char* entry = "ngicp_voxel_rolling_insert_classes";
  if (!h->gate_valid) throw ArgError{NGICP_ERR_STATE, std::string(entry) + ": no ngicp_voxel_rolling_insert_gated has been accepted since the map was last cleared"};
  const size_t n = h->gate_n;
  if (n_out) *n_out = n;
  if (!cls_n || n == 0) return;
  if (capacity < n) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": the array is shorter than the " + std::to_string(n) + " points of that call"};
  HIP_TRY(hipMemcpyAsync(cls_n, h->roll_gate_cls[h->gate_cur].p, n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
}

// ---- the record routes (include/ngicp.h "rolling voxel map: records") ----
// The device time of the last record insert or move: its commit was left in the stream, so the time is read when somebody asks
// (ngicp_voxel_rolling_stats: wait = true) or, without waiting, before the events are recorded again - a commit still running then
// loses its time, not the host's.
void roll_resolve_time(ngicp* h, bool wait) {
  if (!h->rec_time_pending) return;
  h->rec_time_pending = false;
  float ms = 0.f;
  if ((wait ? hipEventSynchronize(h->ev_rec_b) : hipEventQuery(h->ev_rec_b)) != hipSuccess) {
    (void)hipGetLastError();  // ("not ready" is no error of the insert that follows)
    return;
  }
  if (hipEventElapsedTime(&ms, h->ev_rec_a, h->ev_rec_b) == hipSuccess) h->roll.last_insert_ms = ms;
}

// Insert n records at the float pose T (include/ngicp.h: "insert of records").  in / stamps_in are device arrays that stay valid until
// the second synchronisation (the caller holds them); stamps_in != nullptr is the move in place: the map is rebuilt from its own
// former records, every destination voxel is new and carries the largest stamp of its records, and the counter stays.
// Two host synchronisations, both BEFORE the first write to the map: the destination voxel count with the refusal flag of the keys
// (what sizes nothing yet), then the number of new voxels with the overflow flag of the lookup, which ran on the table as it stood.
// Only then do the arrays and the table grow - by the exact count - and the commit is left in the stream.
void roll_insert_records(ngicp* h, const RollRecs& in, const long long* stamps_in, int n, const float T[16], const char* entry, size_t* n_new_out, size_t* n_touched_out) {
  ngicp::RollMap& r = h->roll;
  const bool move = stamps_in != nullptr;
  const RollPose P = roll_pose(T);
  const float inv_res = 1.0f / (float)h->voxel_res;
  roll_resolve_time(h, false);
  size_voxel_work(h, (size_t)n);
  h->roll_sums.ensure((size_t)n * kVoxRec * sizeof(double));
  h->roll_hit.ensure((size_t)n * sizeof(int));
  if (move) h->roll_seg_stamp.ensure((size_t)n * sizeof(long long));
  HIP_TRY(hipEventRecord(h->ev_rec_a, h->stream));
  HIP_TRY(hipMemsetAsync(h->vox_flag.p, 0, sizeof(int), h->stream));
  hipLaunchKernelGGL(k_rollrec_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, in, n, P, inv_res, h->vox_keys.as<unsigned long long>(), h->vox_vals.as<int>(),
                     h->vox_flag.as<int>());
  const VoxelSegments sg = voxel_segments(h, n);
  const auto [n_seg, flag] = read_count(h, sg.n_seg_dev, true);
  if (flag & kRecBadCount) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": a record's count is below 1; nothing was written"};
  if (flag & kRecNoVoxel)
    throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": a record's moved mean lies 2^20 voxels or more from the origin on some axis (or is not finite); nothing was written"};
  if (n_seg <= 0 || n_seg > n) throw ArgError{NGICP_ERR_HIP, std::string(entry) + ": inconsistent voxel count"};
  int* is_new = h->vox_scan.as<int>();  // (as roll_insert: the head and prefix arrays are free again; keys, order and seg_start are not)
  int* rank = is_new + n;
  const bool probe = !move && r.slots && r.n_vox;  // (an empty map, or the move's empty destination: every voxel is new)
  long long* seg_stamp = move ? h->roll_seg_stamp.as<long long>() : nullptr;
  hipLaunchKernelGGL(k_rollrec_lookup, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, h->stream, sg.keys, sg.order, sg.seg_start, n_seg, in, stamps_in, P,
                     probe ? (const ulonglong2*)r.table.as<ulonglong2>() : (const ulonglong2*)nullptr, (unsigned int)(r.slots ? r.slots - 1 : 0), (const double*)r.sums.as<double>(),
                     h->roll_sums.as<double>(), h->roll_hit.as<int>(), is_new, seg_stamp, h->vox_flag.as<int>());
  exclusive_scan_flags(h, is_new, n_seg, rank);
  const auto [n_new, lookup_flag] = read_count(h, rank + n_seg, true);
  if (lookup_flag & kRecOverflow) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": a voxel's count would pass 2^31 - 1; nothing was written"};
  if (n_new < 0 || n_new > n_seg || (move && n_new != n_seg)) throw ArgError{NGICP_ERR_HIP, std::string(entry) + ": inconsistent count of new voxels"};
  const size_t base = move ? 0 : r.n_vox;
  if (base + (size_t)n_new > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": too many voxels for int indices"};
  // ---- from here on the map is written (the lookup has finished: a move's own records, and another handle's, are not read again) ----
  h->hook_valid = 0;
  ++h->roll.gen;
  if (move) r.n_vox = 0;  // nothing of the former arrays is kept: the destination sums are in the workspace
  roll_reserve(h, base + (size_t)n_new);
  if (!roll_reserve_table(h, base + (size_t)n_new) && move) roll_refill_table(h);  // (n_vox == 0: the table cleared)
  roll_launch_commit(h, sg, n_seg, rank, base, seg_stamp);
  HIP_TRY(hipEventRecord(h->ev_rec_b, h->stream));
  HIP_TRY(hipGetLastError());
  h->rec_time_pending = true;
  r.n_vox = base + (size_t)n_new;
  if (!move) ++r.inserts;
  if (n_new_out) *n_new_out = (size_t)n_new;
  if (n_touched_out) *n_touched_out = (size_t)n_seg;
}

// The three record arrays of the C ABI into roll_up, one behind the other, with `extra_bytes` of room behind them (*extra: where).  The
// copies read pageable host arrays: they are the caller's until the next synchronisation, which the caller of this guarantees.
RollRecs roll_upload_records(ngicp* h, size_t n, const double* sum_n3, const double* covsum_n6, const int* count_n, size_t extra_bytes = 0, unsigned char** extra = nullptr) {
  const size_t off_c = n * 3 * sizeof(double), off_n = off_c + n * 6 * sizeof(double), off_x = off_n + n * sizeof(int);
  h->roll_up.ensure(off_x + extra_bytes);
  unsigned char* up = h->roll_up.as<unsigned char>();
  HIP_TRY(hipMemcpyAsync(up, sum_n3, off_c, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(up + off_c, covsum_n6, off_n - off_c, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(up + off_n, count_n, off_x - off_n, hipMemcpyHostToDevice, h->stream));
  if (extra) *extra = up + off_x;
  return RollRecs{nullptr, reinterpret_cast<const double*>(up), reinterpret_cast<const double*>(up + off_c), reinterpret_cast<const int*>(up + off_n)};
}

void roll_insert_voxels(ngicp* h, size_t n_rec, const double* sum_n3, const double* covsum_n6, const int* count_n, const float T[16], size_t* n_new_out, size_t* n_touched_out) {
  const char* entry = "ngicp_voxel_rolling_insert_voxels";
  roll_require_on(h, entry);
  if (!sum_n3 || !covsum_n6 || !count_n || !T) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": null pointer"};
  if (n_rec == 0) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": no records"};
  if (n_rec > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": too many records for int indices"};
  try {  // (the first synchronisation of the insert comes before this returns)
    const RollRecs in = roll_upload_records(h, n_rec, sum_n3, covsum_n6, count_n);
    roll_insert_records(h, in, nullptr, (int)n_rec, T, entry, n_new_out, n_touched_out);
  } catch (...) {
    (void)hipStreamSynchronize(h->stream);  // an upload may still be pending: it must not outlive the caller's arrays
    throw;
  }
}

void roll_insert_map(ngicp* h, ngicp* from, const float T[16], size_t* n_new_out, size_t* n_touched_out) {
  const char* entry = "ngicp_voxel_rolling_insert_map";
  roll_require_on(h, entry);
  if (!T) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": null transform"};
  if (from == h) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": a map cannot be inserted into itself (ngicp_voxel_rolling_transform moves it)"};
  if (h->device != from->device) throw ArgError{NGICP_ERR_ARG, std::string(entry) + " across devices is not supported"};
  const size_t n = from->roll.n_vox;
  if (n == 0) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": the other handle's rolling map is empty"};
  // the producer's stream may still be writing its map (a commit is left in the stream): this handle's stream waits, on the device.
  // Its arrays are read up to the second synchronisation of the insert, which comes before this returns.
  stream_wait_for(h, from);
  const RollRecs in{(const double*)from->roll.sums.as<double>(), nullptr, nullptr, nullptr};
  roll_insert_records(h, in, nullptr, (int)n, T, entry, n_new_out, n_touched_out);
}

// The move in place.  An empty map stays empty.
void roll_transform(ngicp* h, const float T[16], size_t* n_vox_out) {
  const char* entry = "ngicp_voxel_rolling_transform";
  roll_require_on(h, entry);
  if (!T) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": null transform"};
  ngicp::RollMap& r = h->roll;
  if (r.n_vox) {
    const RollRecs in{(const double*)r.sums.as<double>(), nullptr, nullptr, nullptr};
    roll_insert_records(h, in, (const long long*)r.stamps.as<long long>(), (int)r.n_vox, T, entry, nullptr, nullptr);
  }
  if (n_vox_out) *n_vox_out = r.n_vox;
}

// The restore.  Everything that can refuse is checked on the host before the map is touched.  One host synchronisation (the uploads
// read the caller's arrays).
void roll_set(ngicp* h, size_t n, const int* ijk, const double* sum_n3, const double* covsum_n6, const int* count_n, const long long* stamp_n, long long inserts) {
  const char* entry = "ngicp_voxel_rolling_set";
  roll_require_on(h, entry);
  if (inserts < 0) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": a negative insert counter"};
  if (n && (!ijk || !sum_n3 || !covsum_n6 || !count_n || !stamp_n)) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": null pointer"};
  if (n > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": too many voxels for int indices"};
  std::vector<std::pair<unsigned long long, int>> keyed(n);
  for (size_t v = 0; v < n; ++v) {
    const int ix = ijk[3 * v], iy = ijk[3 * v + 1], iz = ijk[3 * v + 2];
    const auto in_range = [](int i) { return i > -kVoxBias && i < kVoxBias; };
    if (!in_range(ix) || !in_range(iy) || !in_range(iz)) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": row " + std::to_string(v) + ": an index of 2^20 or more in magnitude"};
    if (count_n[v] < 1) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": row " + std::to_string(v) + ": a count below 1"};
    if (stamp_n[v] < 1 || stamp_n[v] > inserts) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": row " + std::to_string(v) + ": a stamp outside 1..inserts"};
    keyed[v] = {((unsigned long long)(iz + kVoxBias) << 42) | ((unsigned long long)(iy + kVoxBias) << 21) | (unsigned long long)(ix + kVoxBias), (int)v};
  }
  std::sort(keyed.begin(), keyed.end());
  for (size_t j = 1; j < n; ++j)
    if (keyed[j].first == keyed[j - 1].first)
      throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": rows " + std::to_string(keyed[j - 1].second) + " and " + std::to_string(keyed[j].second) + " name the same voxel"};
  keyed = {};
  // ---- from here on the map is written ----
  ngicp::RollMap& r = h->roll;
  h->hook_valid = 0;
  ++h->roll.gen;
  r.n_vox = 0;  // (nothing of the former map is kept when an array grows)
  r.inserts = inserts;
  if (n == 0) {
    if (r.slots) roll_refill_table(h);
    return;
  }
  roll_reserve(h, n);
  try {
    unsigned char* ijk_dev = nullptr;
    const RollRecs up = roll_upload_records(h, n, sum_n3, covsum_n6, count_n, n * 3 * sizeof(int), &ijk_dev);
    HIP_TRY(hipMemcpyAsync(ijk_dev, ijk, n * 3 * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(r.stamps.p, stamp_n, n * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_rollrec_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, reinterpret_cast<const int*>(ijk_dev), up.S, up.C, up.cnt, (int)n,
                       r.sums.as<double>(), r.rec.as<double>(), r.vkeys.as<unsigned long long>());
    r.n_vox = n;
    if (!roll_reserve_table(h, n)) roll_refill_table(h);  // the key table, filled as after an eviction
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
  } catch (...) {
    (void)hipStreamSynchronize(h->stream);  // an upload may still be pending: it must not outlive the caller's arrays
    r.n_vox = 0;                            // a device failure half way: an empty map, not a half-written one
    if (r.slots) (void)hipMemsetAsync(r.table.p, 0xff, r.slots * sizeof(ulonglong2), h->stream);
    throw;
  }
}

// The tail every removal shares.  `launch_flags(keep)` has written keep[v] = 0 / 1 for the n (> 0) voxels of the map; then the scan, a
// stable compaction into the workspace, ONE host synchronisation - the survivors' count, with whatever `queue_reads` queues beside it -
// then `before_write()`, which refuses by throwing, and the copies back and the table rebuilt, both left in the stream.  A refused call
// has written only workspace.  Returns the survivors' count.
template <class Flags, class Reads, class BeforeWrite>
int roll_remove_unkept(ngicp* h, const char* what, Flags&& launch_flags, Reads&& queue_reads, BeforeWrite&& before_write) {
  ngicp::RollMap& r = h->roll;
  const int n = (int)r.n_vox;
  size_voxel_work(h, (size_t)n);
  const size_t rec_bytes = (size_t)n * kVoxRec * sizeof(double);
  h->roll_tmp.ensure(2 * rec_bytes + (size_t)n * 16);
  const unsigned blocks = (unsigned)((n + 255) / 256);
  int* keep = h->vox_scan.as<int>();
  int* rank = keep + n;  // n + 1 + kCellPad entries
  double* sums_o = h->roll_tmp.as<double>();
  double* rec_o = sums_o + (size_t)n * kVoxRec;
  unsigned long long* vkeys_o = reinterpret_cast<unsigned long long*>(rec_o + (size_t)n * kVoxRec);
  long long* stamps_o = reinterpret_cast<long long*>(vkeys_o + n);
  launch_flags(keep);
  exclusive_scan_flags(h, keep, n, rank);
  hipLaunchKernelGGL(k_roll_compact, dim3(blocks), dim3(256), 0, h->stream, (const int*)keep, (const int*)rank, n, (const double*)r.sums.as<double>(), (const double*)r.rec.as<double>(),
                     (const unsigned long long*)r.vkeys.as<unsigned long long>(), (const long long*)r.stamps.as<long long>(), sums_o, rec_o, vkeys_o, stamps_o);
  queue_reads();
  const int n_keep = read_count(h, rank + n).count;
  before_write();
  if (n_keep < 0 || n_keep > n) throw ArgError{NGICP_ERR_HIP, std::string(what) + ": inconsistent count of survivors"};
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
  return n_keep;
}

// Evict: flags, then the shared tail.  One host synchronisation (the survivors' count) and the wait for the time.
void roll_evict(ngicp* h, const float centre[3], double max_dist, long long min_stamp, size_t* n_removed_out) {
  roll_require_on(h, "ngicp_voxel_rolling_evict");
  if (!centre) throw ArgError{NGICP_ERR_ARG, "ngicp_voxel_rolling_evict: null centre"};
  if (std::isnan(max_dist)) throw ArgError{NGICP_ERR_ARG, "ngicp_voxel_rolling_evict: max_dist is not a number"};
  ngicp::RollMap& r = h->roll;
  h->hook_valid = 0;
  ++h->roll.gen;
  if (n_removed_out) *n_removed_out = 0;
  const int n = (int)r.n_vox;
  if (n == 0) return;
  size_voxel_work(h, (size_t)n);  // (before the first event: growing a buffer waits for the device)
  h->roll_tmp.ensure(2 * (size_t)n * kVoxRec * sizeof(double) + (size_t)n * 16);
  HIP_TRY(hipEventRecord(h->ev_vox_a, h->stream));
  const int n_keep = roll_remove_unkept(
      h, "rolling voxel map evict",
      [&](int* keep) {
        hipLaunchKernelGGL(k_roll_evict_flags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const unsigned long long*)r.vkeys.as<unsigned long long>(),
                           (const long long*)r.stamps.as<long long>(), n, h->voxel_res, (double)centre[0], (double)centre[1], (double)centre[2], max_dist, min_stamp, keep);
      },
      [] {}, [] {});
  HIP_TRY(hipEventRecord(h->ev_vox_b, h->stream));
  HIP_TRY(hipEventSynchronize(h->ev_vox_b));  // (the time; the next alignment would wait for this work anyway)
  HIP_TRY(hipGetLastError());
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, h->ev_vox_a, h->ev_vox_b) == hipSuccess) r.last_evict_ms = ms;
  if (n_removed_out) *n_removed_out = (size_t)(n - n_keep);
}

// ---- clearing along a scan's rays (ngicp_voxel_ray.h; include/ngicp.h "rolling voxel map: clearing along rays") ----
ngicp_ray_clear_options roll_ray_defaults() {
  ngicp_ray_clear_options o;
  o.near_cells = 1;
  o.back_cells = 2;
  o.max_steps = 4096;
  o.min_miss = 2;
  o.radius_cells = 0.25;
  o.keep_stamp = 0;
  o.dry_run = 0;
  return o;
}

// Count `from`'s source cloud at the float pose T against the map, then remove the voxels seen through (the eviction's tail).  One host
// synchronisation: the refusal flag, the totals and the survivors' count in one read-back, behind the compaction into the workspace and
// before anything is copied back.  The counters go into the pair that does not hold the last accepted call's.
void roll_ray_clear(ngicp* h, ngicp* from, const float T[16], const float* origin, const ngicp_ray_clear_options* opt_or_null, ngicp_ray_clear_result* out) {
  const char* entry = "ngicp_voxel_rolling_ray_clear";
  roll_require_on(h, entry);
  if (!T) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": null transform"};
  const ngicp_ray_clear_options o = opt_or_null ? *opt_or_null : roll_ray_defaults();
  if (o.near_cells < 1) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": near_cells below 1"};
  if (o.back_cells < 0) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": back_cells below 0"};
  if (o.max_steps < 1 || o.max_steps > 65536) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": max_steps outside 1 .. 65536"};
  if (o.min_miss < 1) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": min_miss below 1"};
  if (!(o.radius_cells >= 0.0)) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": radius_cells is negative or not a number"};
  if (h->device != from->device) throw ArgError{NGICP_ERR_ARG, std::string(entry) + " across devices is not supported"};
  if (!from->src.present) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": the producer has no source cloud"};
  ensure_slot_ready(from, from->src, "source");
  if (from != h) stream_wait_for(h, from);  // the producer's stream may still be writing the cloud
  const std::shared_ptr<DeviceCloud> cloud = from->src.dev;  // held until the kernel that reads it has been waited for
  const int n_pts = (int)cloud->n;
  if (n_pts <= 0) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": empty source cloud"};
  ngicp::RollMap& r = h->roll;
  const int n = (int)r.n_vox;
  const bool remove = !o.dry_run && n > 0;
  RollRayArgs a;
  for (int k = 0; k < 3; ++k) a.o[k] = origin ? origin[k] : T[12 + k];
  a.inv_res = 1.0f / (float)h->voxel_res;
  a.res = h->voxel_res;
  a.near_cells = o.near_cells;
  a.back_cells = o.back_cells;
  a.max_steps = o.max_steps;
  a.use_radius = o.radius_cells > 0.0 ? 1 : 0;
  const double rad = o.radius_cells * h->voxel_res;
  a.r2 = rad * rad;
  // every buffer before the first launch: growing one waits for the device
  DevBuf& cnt = h->roll_ray[1 - h->ray_cur];
  cnt.ensure((size_t)std::max(n, 1) * 2 * sizeof(unsigned int));
  h->roll_ray_tot.ensure(3 * sizeof(unsigned long long));
  size_voxel_work(h, (size_t)std::max(n, 1));
  if (remove) h->roll_tmp.ensure(2 * (size_t)n * kVoxRec * sizeof(double) + (size_t)n * 16);
  unsigned int* miss = cnt.as<unsigned int>();
  unsigned int* hit = miss + n;
  if (n) HIP_TRY(hipMemsetAsync(cnt.p, 0, (size_t)n * 2 * sizeof(unsigned int), h->stream));
  HIP_TRY(hipMemsetAsync(h->roll_ray_tot.p, 0, 3 * sizeof(unsigned long long), h->stream));
  HIP_TRY(hipMemsetAsync(h->vox_flag.p, 0, sizeof(int), h->stream));
  HIP_TRY(hipEventRecord(h->ev_vox_a, h->stream));
  const bool probe = r.slots && n;
  hipLaunchKernelGGL(k_roll_ray_count, dim3((unsigned)((n_pts + 255) / 256)), dim3(256), 0, h->stream, cloud->pts(), n_pts, roll_pose(T), a,
                     probe ? (const ulonglong2*)r.table.as<ulonglong2>() : (const ulonglong2*)nullptr, (unsigned int)(r.slots ? r.slots - 1 : 0), (const double*)r.rec.as<double>(), miss,
                     hit, h->roll_ray_tot.as<unsigned long long>(), h->vox_flag.as<int>());
  HIP_TRY(hipEventRecord(h->ev_vox_b, h->stream));
  unsigned long long totals[3] = {0, 0, 0};
  int bad = 0;
  const auto queue_reads = [&] {
    HIP_TRY(hipMemcpyAsync(totals, h->roll_ray_tot.p, sizeof(totals), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&bad, h->vox_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  };
  // called behind the one synchronisation: the refusal, or - from here on the map is written - what an eviction drops
  const auto accept = [&] {
    if (bad)
      throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": the origin or a transformed point lies 2^20 voxels or more from the map's origin on some axis (or is not finite); nothing was changed"};
    if (!o.dry_run) {
      h->hook_valid = 0;
      ++h->roll.gen;
    }
  };
  int n_keep = n;
  if (remove) {
    n_keep = roll_remove_unkept(
        h, entry,
        [&](int* keep) {
          hipLaunchKernelGGL(k_roll_ray_flags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const unsigned int*)miss, (const unsigned int*)hit,
                             (const long long*)r.stamps.as<long long>(), n, (unsigned int)o.min_miss, (long long)o.keep_stamp, keep);
        },
        queue_reads, accept);
  } else {
    queue_reads();
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    accept();
  }
  h->ray_cur = 1 - h->ray_cur;
  h->ray_valid = true;
  h->ray_gen = h->roll.gen;
  h->ray_n = (size_t)n;
  float ms = 0.f;
  const bool timed = hipEventElapsedTime(&ms, h->ev_vox_a, h->ev_vox_b) == hipSuccess;
  if (out) {
    out->n_removed = (size_t)(n - n_keep);
    out->steps = (long long)totals[0];
    out->occupied = (long long)totals[1];
    out->misses = (long long)totals[2];
    out->kernel_ms = timed ? (double)ms : 0.0;
  }
}

// the counters of the last accepted clear, in the numbering from before its removal
void roll_ray_counts(ngicp* h, unsigned int* miss_n, unsigned int* hit_n, size_t capacity, size_t* n_out) {
  const char* entry = "ngicp_voxel_rolling_ray_counts";
  if (!h->ray_valid) throw ArgError{NGICP_ERR_STATE, std::string(entry) + ": no ngicp_voxel_rolling_ray_clear has been accepted"};
  if (h->ray_gen != h->roll.gen) throw ArgError{NGICP_ERR_STATE, std::string(entry) + ": the map has been changed since the last ngicp_voxel_rolling_ray_clear"};
  const size_t n = h->ray_n;
  if (n_out) *n_out = n;
  if ((!miss_n && !hit_n) || n == 0) return;
  if (capacity < n) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": the arrays are shorter than the " + std::to_string(n) + " voxels of that call"};
  const unsigned int* dev = h->roll_ray[h->ray_cur].as<unsigned int>();
  if (miss_n) HIP_TRY(hipMemcpyAsync(miss_n, dev, n * sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
  if (hit_n) HIP_TRY(hipMemcpyAsync(hit_n, dev + n, n * sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
}

}  // namespace
