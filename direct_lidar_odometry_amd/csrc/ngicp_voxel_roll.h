// The rolling voxel map (include/ngicp.h "rolling voxel map"): a voxel map that lives across frames.  Scans are added to
// it at a pose, old voxels are dropped from it, and the voxelized passes (ngicp_voxel.h) align against it unchanged: they read
// {table, mask, rec, n_vox} and do not care who filled them.  The project's own definition; no fidelity to an outside library is claimed.
//
//   state per voxel v             sums[v] = {S 3, C 6 (xx, xy, xz, yy, yz, zz), n} in double, stamp[v] = the number of the last insert that
//                                 added a point, vkeys[v] = the voxel's key, and rec[v] = {S / n, C / n, n}: the kVoxRec record the passes
//                                 read.  Voxels are numbered in order of first insertion.
//   insert of a scan at pose T    k_roll_keys       one thread per scan point: q = transform_point_f(T, a) kept in qpts (sorted position), the
//                                                   key of q and the sorted position by ORIGINAL index; *bad when q has no voxel
//                                 voxel_segments    (ngicp_voxelmap.h) stable sort, heads, scan, starts - over the scan's points only
//                                 k_roll_lookup     one thread per scan voxel: voxel_segment_sums over qpts, ONE rotate_sym of the covariance
//                                                   sum, one read-only voxel_lookup: the existing number or -1, and the flag "new"
//                                 (the three-kernel exclusive scan over the flags: a new voxel's rank, in ascending key)
//                                 k_roll_commit     one thread per scan voxel: an existing voxel gets one addition per entry, a new one is
//                                                   appended at n_vox + rank and entered into the table; the stamp; the record by one division
//                                 Lookup and commit are separate launches: no probe races an insertion.  Distinct threads own distinct
//                                 voxels: nothing depends on the order in which threads arrive.  Nothing walks the existing map.
//   table                         ngicp_voxel.h's, at most half full.  k_roll_table_fill enters the keys [0, n) into a cleared table: the
//                                 rebuild at twice the size before a commit that would cross the limit, and after an eviction.
//   evict                         k_roll_evict_flags (keep = 0 / 1 per voxel), the same scan, k_roll_compact into a workspace (stable: the
//                                 survivors keep their order), copies back, table rebuild.
#pragma once
#include "ngicp_cloudops.h"
#include "ngicp_voxel.h"

namespace ngk {

// the pose of an insert as the kernels take it: the float matrix (column-major) and the row-major double image of its 3x3 block
struct RollPose {
  float m[16];
  double R[9];
};

// keys[o] / vals[o] for ORIGINAL index o, as k_voxel_map_keys, of the TRANSFORMED point, which stays in qpts[sorted position]
__global__ void __launch_bounds__(256) k_roll_keys(const float4* __restrict__ pts, int n, RollPose T, float inv_res, float4* __restrict__ qpts,
                                                    unsigned long long* __restrict__ keys, int* __restrict__ vals, int* __restrict__ bad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const float4 p = pts[s];
  const int o = __float_as_int(p.w);
  const float3 q = transform_point_f(T.m, p.x, p.y, p.z);
  qpts[s] = make_float4(q.x, q.y, q.z, p.w);
  unsigned long long key = 0;
  if (!voxel_key(q.x, q.y, q.z, inv_res, key)) atomicOr(bad, 1);
  keys[o] = key;
  vals[o] = s;
}

// One thread per scan voxel u: its sums {s 3, rotate_sym(R, sum C) 6, n} into scan_sums[u], the map's number of its key (or -1) into
// hit[u], is_new[u] = 1 when the map does not have it.  The table is only read.
__global__ void __launch_bounds__(256) k_roll_lookup(const unsigned long long* __restrict__ keys, const int* __restrict__ order, const int* __restrict__ seg_start, int n_seg,
                                                      const float4* __restrict__ qpts, const double* __restrict__ covs, RollPose T, const ulonglong2* __restrict__ table,
                                                      unsigned int mask, double* __restrict__ scan_sums, int* __restrict__ hit, int* __restrict__ is_new) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_seg) return;
  const int s = seg_start[u], e = seg_start[u + 1];
  double m[3], c[6], rc[6];
  voxel_segment_sums(order, s, e, qpts, covs, m, c);
  rotate_sym(T.R, c, rc);
  double* o = scan_sums + (size_t)u * kVoxRec;
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = m[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) o[3 + k] = rc[k];
  o[9] = (double)(e - s);
  unsigned int probes = 0;
  const int v = voxel_lookup(table, mask, keys[s], probes);
  hit[u] = v;
  is_new[u] = v < 0 ? 1 : 0;
}

// the record of a voxel from its sums: one division per entry
__device__ __forceinline__ void roll_write_record(const double (&S)[kVoxRec], double* __restrict__ r) {
  const double cnt = S[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) r[k] = S[k] / cnt;
  r[9] = cnt;
}

// One thread per scan voxel u.  An existing voxel: sums = sums + scan sums (one addition per entry, the count among them: exact).  A new
// one: voxel n_vox + rank[u] starts from the scan's sums, gets its key and its table entry.  Both: the stamp and the record.
__global__ void __launch_bounds__(256) k_roll_commit(const unsigned long long* __restrict__ keys, const int* __restrict__ seg_start, int n_seg,
                                                      const double* __restrict__ scan_sums, const int* __restrict__ hit, const int* __restrict__ rank, int n_vox, long long stamp,
                                                      double* __restrict__ sums, double* __restrict__ rec, unsigned long long* __restrict__ vkeys, long long* __restrict__ stamps,
                                                      ulonglong2* __restrict__ table, unsigned int mask) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_seg) return;
  const double* a = scan_sums + (size_t)u * kVoxRec;
  double S[kVoxRec];
  int v = hit[u];
  if (v >= 0) {
    const double* old = sums + (size_t)v * kVoxRec;
#pragma unroll
    for (int k = 0; k < kVoxRec; ++k) S[k] = old[k] + a[k];
  } else {
    v = n_vox + rank[u];
#pragma unroll
    for (int k = 0; k < kVoxRec; ++k) S[k] = a[k];
    const unsigned long long key = keys[seg_start[u]];
    vkeys[v] = key;
    voxel_table_insert(table, mask, key, v);
  }
  double* d = sums + (size_t)v * kVoxRec;
#pragma unroll
  for (int k = 0; k < kVoxRec; ++k) d[k] = S[k];
  stamps[v] = stamp;
  roll_write_record(S, rec + (size_t)v * kVoxRec);
}

// {vkeys[v], v} for v in [0, n) into a cleared table
__global__ void __launch_bounds__(256) k_roll_table_fill(const unsigned long long* __restrict__ vkeys, int n, ulonglong2* __restrict__ table, unsigned int mask) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  voxel_table_insert(table, mask, vkeys[v], v);
}

// keep[v] = 0 when voxel v goes: its centre lies farther than max_dist from c (max_dist > 0), or its stamp is below min_stamp (min_stamp > 0).
// All in double, nothing fused (the library is built with -ffp-contract=off).
__global__ void __launch_bounds__(256) k_roll_evict_flags(const unsigned long long* __restrict__ vkeys, const long long* __restrict__ stamps, int n, double res, double cx, double cy,
                                                           double cz, double max_dist, long long min_stamp, int* __restrict__ keep) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const unsigned long long key = vkeys[v];
  const int ix = (int)(key & 0x1fffffull) - kVoxBias, iy = (int)((key >> 21) & 0x1fffffull) - kVoxBias, iz = (int)((key >> 42) & 0x1fffffull) - kVoxBias;
  bool gone = false;
  if (max_dist > 0.0) {
    const double dx = ((double)ix + 0.5) * res - cx, dy = ((double)iy + 0.5) * res - cy, dz = ((double)iz + 0.5) * res - cz;
    gone = ((dx * dx + dy * dy) + dz * dz) > max_dist * max_dist;
  }
  if (min_stamp > 0 && stamps[v] < min_stamp) gone = true;
  keep[v] = gone ? 0 : 1;
}

// survivor v -> position rank[v] of the workspace arrays (rank: the exclusive prefix of keep)
__global__ void __launch_bounds__(256) k_roll_compact(const int* __restrict__ keep, const int* __restrict__ rank, int n, const double* __restrict__ sums,
                                                       const double* __restrict__ rec, const unsigned long long* __restrict__ vkeys, const long long* __restrict__ stamps,
                                                       double* __restrict__ sums_o, double* __restrict__ rec_o, unsigned long long* __restrict__ vkeys_o,
                                                       long long* __restrict__ stamps_o) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n || !keep[v]) return;
  const int w = rank[v];
#pragma unroll
  for (int k = 0; k < kVoxRec; ++k) sums_o[(size_t)w * kVoxRec + k] = sums[(size_t)v * kVoxRec + k];
#pragma unroll
  for (int k = 0; k < kVoxRec; ++k) rec_o[(size_t)w * kVoxRec + k] = rec[(size_t)v * kVoxRec + k];
  vkeys_o[w] = vkeys[v];
  stamps_o[w] = stamps[v];
}

}  // namespace ngk
