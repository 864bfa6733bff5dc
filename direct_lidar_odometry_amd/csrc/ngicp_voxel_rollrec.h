// The rolling voxel map filled from voxel RECORDS instead of points (include/ngicp.h "rolling voxel map: records"):
// restore (ngicp_voxel_rolling_set), insert of records at a pose (ngicp_voxel_rolling_insert_voxels / _insert_map) and the move in place
// (ngicp_voxel_rolling_transform).  A record is what ngicp_voxel_rolling_get returns per voxel, {S 3, C 6, n}, plus a stamp.  The scan
// insert's pipeline (ngicp_voxel_roll.h) over records; its kernels are not touched.
//
//   insert of records at pose T   k_rollrec_keys     one thread per record: m = S / n (three divisions), p = (float)m, q = transform_point_f(T, p),
//                                                    the key of q; keys[r] / vals[r] = r as k_roll_keys lays them out.  *flag bit 0 when q
//                                                    has no voxel, bit 1 when the count is below 1
//                                 voxel_segments     (ngicp_voxelmap.h) unchanged: stable sort, heads, scan, starts
//                                 k_rollrec_lookup   one thread per destination voxel: A = sum S_r, Cc = sum C_r from 0.0 in ascending input index,
//                                                    N = sum n_r in integers, the segment's largest stamp (the move), s = R A + N t, ONE
//                                                    rotate_sym, one read-only voxel_lookup; *flag bit 2 when the voxel's count would pass 2^31 - 1
//                                 (the three-kernel exclusive scan over the flags "new")
//                                 k_rollrec_commit   k_roll_commit with the stamp either a scalar or per destination voxel
//   restore                       k_rollrec_fill     one thread per voxel: the key from ijk, the sums as given, the record by roll_write_record
//                                                    (k_roll_table_fill follows)
// Lookup and commit are separate launches, distinct threads own distinct voxels, nothing is added atomically: nothing depends on the
// order in which threads arrive.
#pragma once
#include "ngicp_voxel_roll.h"

namespace ngk {

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
  double* o = dst_sums + (size_t)u * kVoxRec;
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = ((T.R[k * 3 + 0] * A[0] + T.R[k * 3 + 1] * A[1]) + T.R[k * 3 + 2] * A[2]) + (double)N * (double)T.m[12 + k];
#pragma unroll
  for (int k = 0; k < 6; ++k) o[3 + k] = rc[k];
  o[9] = (double)N;
  int v = -1;
  if (table) {
    unsigned int probes = 0;
    v = voxel_lookup(table, mask, keys[s], probes);
  }
  hit[u] = v;
  is_new[u] = v < 0 ? 1 : 0;
  const long long total = N + (v >= 0 ? (long long)map_sums[(size_t)v * kVoxRec + 9] : 0ll);
  if (total > 2147483647ll) atomicOr(flag, kRecOverflow);
  if (seg_stamp) seg_stamp[u] = newest;
}

// k_roll_commit for destination voxels of records: the stamp is seg_stamp[u] when that array is given (the move in place), else `stamp`.
__global__ void __launch_bounds__(256) k_rollrec_commit(const unsigned long long* __restrict__ keys, const int* __restrict__ seg_start, int n_seg,
                                                         const double* __restrict__ dst_sums, const int* __restrict__ hit, const int* __restrict__ rank, int n_vox, long long stamp,
                                                         const long long* __restrict__ seg_stamp, double* __restrict__ sums, double* __restrict__ rec,
                                                         unsigned long long* __restrict__ vkeys, long long* __restrict__ stamps, ulonglong2* __restrict__ table, unsigned int mask) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_seg) return;
  const double* a = dst_sums + (size_t)u * kVoxRec;
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
  roll_write_record(S, rec + (size_t)v * kVoxRec);
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
  roll_write_record(S, rec + (size_t)v * kVoxRec);
  vkeys[v] = voxel_pack(ijk[3 * v + 0], ijk[3 * v + 1], ijk[3 * v + 2]);
}

}  // namespace ngk
