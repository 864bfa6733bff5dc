// The rolling voxel map (include/ngicp.h "rolling voxel map" and "rolling voxel map: records"): a voxel map that
// lives across frames.  Scans are added to it at a pose, voxel RECORDS (what ngicp_voxel_rolling_get returns per voxel, {S 3, C 6, n},
// plus a stamp) are restored into it, added to it at a pose or moved in place, old voxels are dropped from it, and the voxelized passes
// (ngicp_voxel.h) align against it unchanged: they read {table, mask, rec, n_vox} and do not care who filled them.  The project's own
// definition; no fidelity to an outside library is claimed.
//
//   state per voxel v    sums[v] = {S 3, C 6 (xx, xy, xz, yy, yz, zz), n} in double, stamp[v] = the number of the last insert that added to it,
//                        vkeys[v] = the voxel's key, and rec[v] = {S / n, C / n, n}: the kVoxRec record the passes read
//                        (voxel_record_from_sums).  Voxels are numbered in order of first insertion.
//   step                 insert of a scan at pose T (ngicp_voxel_rolling_insert)     insert of records at pose T (_insert_voxels / _insert_map / _transform)
//   keys                 k_roll_keys: one thread per scan point, q = transform_point_f  k_rollrec_keys: one thread per record, m = S / n (three divisions),
//                        (T, a) kept in qpts (sorted position), the key of q and the     p = (float)m, q = transform_point_f(T, p), the key of q;
//                        sorted position by ORIGINAL index; *bad when q has no voxel     keys[r] / vals[r] = r; flag bits kRecNoVoxel, kRecBadCount
//   numbering            voxel_segments (ngicp_voxelmap.h): stable sort, heads, scan, starts - over the scan's points or the records only
//   lookup               k_roll_lookup: one thread per scan voxel,                      k_rollrec_lookup: one thread per destination voxel, A = sum S_r,
//                        voxel_segment_sums over qpts, ONE rotate_sym of the             Cc = sum C_r from 0.0 in ascending input index, N = sum n_r in
//                        covariance sum                                                  integers, the segment's largest stamp (the move), s = R A + N t,
//                                                                                        ONE rotate_sym; flag bit kRecOverflow past 2^31 - 1
//                        both end in roll_store_lookup: the ten sums stored, one read-only voxel_lookup, the existing number or -1, the flag "new"
//   ranks                exclusive_scan_flags (ngicp_voxelmap.h) over the flags: a new voxel's rank, in ascending key
//   commit               k_roll_commit: one thread per scan / destination voxel: an existing voxel gets one addition per entry, a new one is
//                        appended at n_vox + rank and entered into the table; the stamp (the insert's number, or per destination voxel for the
//                        move); the record by one division
//   restore              k_rollrec_fill: one thread per voxel, the key from ijk, the sums as given, the record (k_roll_table_fill follows)
//   table                ngicp_voxel.h's, at most half full.  k_roll_table_fill enters the keys [0, n) into a cleared table: the rebuild at
//                        twice the size before a commit that would cross the limit, after an eviction and after a restore.
//   evict                k_roll_evict_flags (keep = 0 / 1 per voxel), the same scan, k_roll_compact into a workspace (stable: the survivors
//                        keep their order), copies back, table rebuild.
//   clear along rays     ngicp_voxel_ray.h: k_roll_ray_count walks the map along a scan's rays and counts misses and hits
//                        per voxel, k_roll_ray_flags turns them into keep flags, and the removal is the eviction's from the scan on.
//   gated insert         ngicp_voxel_gate.h: k_roll_gate classifies a scan's points against the map and does k_roll_keys' work
//                        beside it, k_roll_gate_scatter compacts the kept pairs, and the insert is the one above from its numbering step on.
// Lookup and commit are separate launches: no probe races an insertion.  Distinct threads own distinct voxels and nothing is added
// atomically: nothing depends on the order in which threads arrive.  Nothing walks the existing map.
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

// The ending both lookups share: a scan / destination voxel's sums {s 3, rc 6, n} stored, the map's number of its key (or -1; a null
// table holds no voxel) into *hit, *is_new = 1 when the map does not have it.  The table is only read.  Returns the number.
__device__ __forceinline__ int roll_store_lookup(const double (&s)[3], const double (&rc)[6], double n, const ulonglong2* __restrict__ table, unsigned int mask,
                                                 unsigned long long key, double* __restrict__ o, int* __restrict__ hit, int* __restrict__ is_new) {
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = s[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) o[3 + k] = rc[k];
  o[9] = n;
  int v = -1;
  if (table) {
    unsigned int probes = 0;
    v = voxel_lookup(table, mask, key, probes);
  }
  *hit = v;
  *is_new = v < 0 ? 1 : 0;
  return v;
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
  roll_store_lookup(m, rc, (double)(e - s), table, mask, keys[s], scan_sums + (size_t)u * kVoxRec, hit + u, is_new + u);
}

// One thread per scan / destination voxel u.  An existing voxel: sums = sums + scan sums (one addition per entry, the count among them:
// exact).  A new one: voxel n_vox + rank[u] starts from the scan's sums, gets its key and its table entry.  Both: the record, and the
// stamp - seg_stamp[u] when that array is given (the move in place), else `stamp`.
__global__ void __launch_bounds__(256) k_roll_commit(const unsigned long long* __restrict__ keys, const int* __restrict__ seg_start, int n_seg,
                                                      const double* __restrict__ scan_sums, const int* __restrict__ hit, const int* __restrict__ rank, int n_vox, long long stamp,
                                                      const long long* __restrict__ seg_stamp, double* __restrict__ sums, double* __restrict__ rec,
                                                      unsigned long long* __restrict__ vkeys, long long* __restrict__ stamps, ulonglong2* __restrict__ table, unsigned int mask) {
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
  stamps[v] = seg_stamp ? seg_stamp[u] : stamp;
  voxel_record_from_sums(S, rec + (size_t)v * kVoxRec);
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

// ---- the record routes ----
constexpr int kRecNoVoxel = 1, kRecBadCount = 2, kRecOverflow = 4;  // bits of the refusal flag

// Where the records of an insert are: the map's own layout [n][kVoxRec] (another handle's sums, or this map's), or the three arrays
// of the C ABI as uploaded (packed == nullptr).
struct RollRecs {
  const double* packed;
  const double* S;   // [n][3]
  const double* C;   // [n][6]
  const int* cnt;    // [n]
};

__device__ __forceinline__ void rollrec_load(const RollRecs& in, int r, double (&S)[3], double (&Cv)[6], double& cnt) {
  if (in.packed) {
    const double* p = in.packed + (size_t)r * kVoxRec;
#pragma unroll
    for (int k = 0; k < 3; ++k) S[k] = p[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) Cv[k] = p[3 + k];
    cnt = p[9];
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) S[k] = in.S[(size_t)r * 3 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) Cv[k] = in.C[(size_t)r * 6 + k];
    cnt = (double)in.cnt[r];
  }
}

// keys[r] / vals[r] = r for record r: the key of the voxel its moved float mean lies in
__global__ void __launch_bounds__(256) k_rollrec_keys(RollRecs in, int n, RollPose T, float inv_res, unsigned long long* __restrict__ keys, int* __restrict__ vals,
                                                       int* __restrict__ flag) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const double* S = in.packed ? in.packed + (size_t)r * kVoxRec : in.S + (size_t)r * 3;  // (the covariance sum is not read here)
  const double cnt = in.packed ? S[9] : (double)in.cnt[r];
  int f = 0;
  if (!(cnt >= 1.0)) f |= kRecBadCount;
  const float px = (float)(S[0] / cnt), py = (float)(S[1] / cnt), pz = (float)(S[2] / cnt);
  const float3 q = transform_point_f(T.m, px, py, pz);
  unsigned long long key = 0;
  if (!voxel_key(q.x, q.y, q.z, inv_res, key)) f |= kRecNoVoxel;
  if (f) atomicOr(flag, f);
  keys[r] = key;
  vals[r] = r;
}

// One thread per destination voxel u: {s 3, rotate_sym(R, sum C) 6, N} into dst_sums[u], the map's number of its key (or -1) into hit[u],
// is_new[u], and (stamps_in != nullptr) the largest stamp of its records into seg_stamp[u].  `table` may be null (no map yet, or the move
// in place, which inserts into an empty map): every voxel is new.  The map is only read.
__global__ void __launch_bounds__(256) k_rollrec_lookup(const unsigned long long* __restrict__ keys, const int* __restrict__ order, const int* __restrict__ seg_start, int n_seg,
                                                         RollRecs in, const long long* __restrict__ stamps_in, RollPose T, const ulonglong2* __restrict__ table, unsigned int mask,
                                                         const double* __restrict__ map_sums, double* __restrict__ dst_sums, int* __restrict__ hit, int* __restrict__ is_new,
                                                         long long* __restrict__ seg_stamp, int* __restrict__ flag) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_seg) return;
  const int s = seg_start[u], e = seg_start[u + 1];
  double A[3], Cc[6], rc[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) A[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) Cc[k] = 0.0;
  long long N = 0, newest = 0;
  for (int j = s; j < e; ++j) {
    const int r = order[j];
    double S[3], Cv[6], cnt;
    rollrec_load(in, r, S, Cv, cnt);
#pragma unroll
    for (int k = 0; k < 3; ++k) A[k] += S[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) Cc[k] += Cv[k];
    N += (long long)cnt;  // (counts are integers below 2^31; at most 2^31 records: no overflow)
    if (stamps_in) {
      const long long t = stamps_in[r];
      newest = t > newest ? t : newest;
    }
  }
  rotate_sym(T.R, Cc, rc);
  double sv[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) sv[k] = ((T.R[k * 3 + 0] * A[0] + T.R[k * 3 + 1] * A[1]) + T.R[k * 3 + 2] * A[2]) + (double)N * (double)T.m[12 + k];
  const int v = roll_store_lookup(sv, rc, (double)N, table, mask, keys[s], dst_sums + (size_t)u * kVoxRec, hit + u, is_new + u);
  const long long total = N + (v >= 0 ? (long long)map_sums[(size_t)v * kVoxRec + 9] : 0ll);
  if (total > 2147483647ll) atomicOr(flag, kRecOverflow);
  if (seg_stamp) seg_stamp[u] = newest;
}

// The restore: voxel v from row v of the uploaded arrays.  (The stamps are copied straight into the map's array.)
__global__ void __launch_bounds__(256) k_rollrec_fill(const int* __restrict__ ijk, const double* __restrict__ S3, const double* __restrict__ C6, const int* __restrict__ cnt, int n,
                                                       double* __restrict__ sums, double* __restrict__ rec, unsigned long long* __restrict__ vkeys) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  double S[kVoxRec];
#pragma unroll
  for (int k = 0; k < 3; ++k) S[k] = S3[(size_t)v * 3 + k];
#pragma unroll
  for (int k = 0; k < 6; ++k) S[3 + k] = C6[(size_t)v * 6 + k];
  S[9] = (double)cnt[v];
  double* d = sums + (size_t)v * kVoxRec;
#pragma unroll
  for (int k = 0; k < kVoxRec; ++k) d[k] = S[k];
  voxel_record_from_sums(S, rec + (size_t)v * kVoxRec);
  vkeys[v] = voxel_pack(ijk[3 * v + 0], ijk[3 * v + 1], ijk[3 * v + 2]);
}

// ---- the gated insert: what its classification takes.  The kernels are in ngicp_voxel_gate.h, behind every other kernel
// of the library; the host code (ngicp_rollmap.h) fills this in front of them. ----
constexpr int kGateBlock = 256;
constexpr int kGateNew = 0, kGateExplained = 1, kGateConflict = 2, kGateUnjudged = 3;  // ngicp.h NGICP_GATE_*

struct RollGateArgs {
  const float4* pts;        // the producer's source in the index's sorted order, w = original index
  const double* covs;       // [n][6], the same order
  int n;
  float inv_res;
  const ulonglong2* table;  // the rolling map's table (null: a map that never had one - no slot is occupied), mask and records
  unsigned int mask;
  const double* rec;
  double max_m;             // the gate
  double min_count;         // (double)min_voxel_count: counts are stored as doubles, exact
  int keep_new, keep_unjudged;
  float4* qpts;             // [n] by sorted position: the insert's transformed points
  unsigned long long* keys; // [n] by original index: the insert's keys, uncompacted
  int* vals;                // [n] by original index: sorted positions
  unsigned char* cls;       // [n] by original index
  int* keep;                // [n] by original index: 0 / 1
  int* counts;              // [4] class counts, cleared by the caller
  int* bad;
};

}  // namespace ngk
