// The voxel map of a voxelized target (ngicp_voxel.h): built from the target's points, or merged from the voxel parts of
// a submap's keyframes.  Part of ngicp_api.hip's translation unit (included there, after the covariances' host code).
#pragma once

namespace {

// The working buffers of a voxel build over a list of up to n (key, value) pairs.  Every build sizes them for its longest list before
// its first launch: growing a buffer frees it, and freeing waits for the device.
void size_voxel_work(ngicp* h, size_t n) {
  h->vox_keys.ensure(n * 2 * sizeof(unsigned long long));
  h->vox_vals.ensure(n * 2 * sizeof(int));
  h->vox_scan.ensure((n * 3 + 2 + kCellPad) * sizeof(int));
  h->vox_flag.ensure(64);
  h->tile_sums.ensure(((n + kScanTile - 1) / kScanTile) * sizeof(int));
}

// rank[0 .. n] = the exclusive prefix sums of the n int flags (rank[n]: their total), three launches on the handle's stream with tile_sums,
// which size_voxel_work sized for n.  Nothing is synchronised.
void exclusive_scan_flags(ngicp* h, const int* flags, int n, int* rank) {
  const int ntiles = (n + kScanTile - 1) / kScanTile;
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(kScanBlock), 0, h->stream, flags, n, h->tile_sums.as<int>(), (unsigned long long*)nullptr);
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(kScanBlock), 0, h->stream, h->tile_sums.as<int>(), ntiles, (const unsigned long long*)nullptr, (unsigned long long*)nullptr);
  hipLaunchKernelGGL(k_scan_apply, dim3(ntiles), dim3(kScanBlock), 0, h->stream, flags, n, (const int*)h->tile_sums.as<int>(), rank);
}

// A count the stream leaves on the device (a numbering's segments, a scan's total) and, if asked for, the flag word vox_flag, read
// back: one host synchronisation.  What the two values refuse is the caller's business.
struct CountAndFlag {
  int count, flag;
};
CountAndFlag read_count(ngicp* h, const int* count_dev, bool with_flag = false) {
  CountAndFlag r{0, 0};
  HIP_TRY(hipMemcpyAsync(&r.count, count_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (with_flag) HIP_TRY(hipMemcpyAsync(&r.flag, h->vox_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  return r;
}

// the slots of a table that stays at most half full with `need` voxels: a power of two, at least 64 and at least `current`
size_t voxel_table_slots(size_t need, size_t current = 0) {
  size_t slots = std::max(current, (size_t)64);
  while (slots < 2 * need) slots <<= 1;
  return slots;
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
  exclusive_scan_flags(h, head, n, vox_of);
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
  const size_t slots = voxel_table_slots((size_t)n_vox);
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
  const auto [n_vox, bad] = read_count(h, sg.n_seg_dev, true);
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
  const auto [n_vox, bad] = read_count(h, sg.n_seg_dev, true);
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
  const int n_vox = read_count(h, sg.n_seg_dev).count;
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

// Is the rolling map (ngicp_rollmap.h) the map of this handle's voxelized entries?  Then the target slot is not read at all.
bool rolling_active(const ngicp* h) { return h->voxel_roll && h->voxel_res > 0.0; }

// The map the voxelized entries use as it stands now, without building anything: the rolling map while that setting is on, else the
// target's (what the correspondences of the last linearisation number).
VoxelMapView voxel_map_view(const ngicp* h) {
  if (rolling_active(h)) {
    const ngicp::RollMap& r = h->roll;
    return VoxelMapView{r.table.as<ulonglong2>(), (unsigned int)(r.slots - 1), r.rec.as<double>(), r.vkeys.as<unsigned long long>(), r.n_vox};
  }
  const ngicp::VoxelMap& m = h->vmap;
  return VoxelMapView{m.table.as<ulonglong2>(), m.mask, m.rec.as<double>(), m.vkeys.as<unsigned long long>(), m.n_vox};
}

// Would ensure_voxel_map return the target's map as it stands (no upload, no covariances, no build)?  Not meant for the rolling map.
bool voxel_map_current(const ngicp* h) {
  const ngicp::VoxelMap& m = h->vmap;
  if (!h->tgt.dev || h->tgt_covs.n != h->tgt.dev->n) return false;
  // (after ngicp_keyframe_transform moved a keyframe of the submap, the map of the unchanged target stands whichever route built it)
  return m.valid && m.res == h->voxel_res && m.cloud == h->tgt.dev && m.covs == h->tgt_covs.data && (m.merged == (merged_route_applies(h) ? 1 : 0) || h->submap_moved);
}

// The voxel map of the current target, its covariances (computed if missing, as for align) and the resolution: built at the first use
// after any of the three changed, or after the route it would be built by did (ngicp_set_voxel_submap_merge).  With the rolling setting
// on: the rolling map as inserts and evictions left it (nothing is built, the target and the merged setting are not consulted); an
// empty one is NGICP_ERR_STATE, where a missing target would be.
VoxelMapView ensure_voxel_map(ngicp* h) {
  if (rolling_active(h)) {
    if (h->roll.n_vox == 0) throw ArgError{NGICP_ERR_STATE, "the rolling voxel map is empty (ngicp_voxel_rolling_insert)"};
    return voxel_map_view(h);
  }
  ensure_slot_ready(h, h->tgt, "target");
  if (h->tgt_covs.n != h->tgt.dev->n) compute_covs(h, h->tgt, h->tgt_covs, "target");
  const double* covs = covs_for(h, h->tgt_covs, h->tgt.dev);
  ngicp::VoxelMap& m = h->vmap;
  const int merged = merged_route_applies(h) && !h->submap_moved ? 1 : 0;  // (moved keyframes' parts no longer add up to this target)
  if (voxel_map_current(h)) return voxel_map_view(h);
  m.invalidate();
  if (merged) build_voxel_map_merged(h);
  else build_voxel_map_from_points(h, covs);
  m.merged = merged;
  m.res = h->voxel_res;
  m.cloud = h->tgt.dev;
  m.covs = h->tgt_covs.data;
  m.valid = true;
  ++h->voxel_builds;
  return voxel_map_view(h);
}

}  // namespace
