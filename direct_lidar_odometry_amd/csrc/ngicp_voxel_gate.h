// The gated insert of the rolling voxel map (include/ngicp.h "rolling voxel map: gated insert"): a scan's points are
// classified against the map at the pose, and only the points the map explains - or that fall where it holds nothing - enter the
// insert's own pipeline (ngicp_voxel_roll.h).  The project's own definition; no fidelity to an outside library is claimed.
//
//   classify   k_roll_gate<K>: one thread per source point in the index's sorted order.  The point and its covariance are loaded once.
//                q_i   the INSERT's point, transform_point_f(T, a) as k_roll_keys computes it: kept in qpts[sorted position], its key and
//                      the sorted position by ORIGINAL index in the pair arrays, *bad when it has no voxel (whatever the class).
//                q_g   the GATE's point, the float pose times the point in the passes' order (transform_point_rowmajor_f), its cell
//                      from voxel_cell: exactly k_voxel_fitness's q, so that the classes follow from ngicp_voxel_fitness_points.
//                slots vox_fit_best_slot (ngicp_voxel_fitness.h), the rolled slot loop k_voxel_fitness runs, with the count test:
//                      an occupied slot judges only when its voxel's count is at least min_voxel_count.  No LDS column, no scratch.
//                class NEW (no occupied slot), EXPLAINED (a winner, best <= max_m), CONFLICT (a winner, best > max_m), UNJUDGED
//                      (occupied slots, no winner); cls[o] and keep[o] by original index.
//              The block's four class counts: a ballot and a population count per wave and class, the four waves through LDS, one
//              integer atomicAdd per class and block.  No floating-point atomics.
//   compact    exclusive_scan_flags over keep (ascending original index), then k_roll_gate_scatter: the kept pairs to the front of
//              vox_keys / vox_vals in that order.  qpts and the covariances are read by sorted position and are not compacted.
//   the tail   voxel_segments over the kept pairs, k_roll_lookup, the rank scan, k_roll_commit: the plain insert's, unchanged.
// Templates throughout (the scatter too): the compiler then emits them behind every kernel the library had, and the code object up to
// there is laid out as it was without this header (the note at k_voxel_fitness_final).
#pragma once
#include "ngicp_voxel_fitness.h"
#include "ngicp_voxel_roll.h"

namespace ngk {

template <int K>
__global__ void __launch_bounds__(kGateBlock) k_roll_gate(RollGateArgs a, RollPose T) {
  static_assert(K == 1 || K == 7 || K == 27, "DIRECT1, DIRECT7 or DIRECT27");
  __shared__ int wave_cnt[kGateBlock / 64][4];
  const int i = blockIdx.x * kGateBlock + threadIdx.x;
  int cls = -1;
  if (i < a.n) {
    const float4 sp = a.pts[i];
    const int o = __float_as_int(sp.w);
    // the insert's half: k_roll_keys
    const float3 qi = transform_point_f(T.m, sp.x, sp.y, sp.z);
    a.qpts[i] = make_float4(qi.x, qi.y, qi.z, sp.w);
    unsigned long long key = 0;
    if (!voxel_key(qi.x, qi.y, qi.z, a.inv_res, key)) atomicOr(a.bad, 1);
    a.keys[o] = key;
    a.vals[o] = i;
    // the gate's half: k_voxel_fitness's point, cell and slots
    float Tf[12];  // row-major 3x4, the layout of the passes' float pose
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) Tf[r * 4 + c] = T.m[c * 4 + r];
    const float3 q = transform_point_rowmajor_f(Tf, sp.x, sp.y, sp.z);
    bool occupied = false;
    double best = __builtin_inf(), best_d = __builtin_inf();
    int best_v = -1;
    int cx, cy, cz;
    if (a.table && voxel_cell(q.x, q.y, q.z, a.inv_res, cx, cy, cz)) {
      const double ax = (double)sp.x, ay = (double)sp.y, az = (double)sp.z;
      const double tax = T.R[0] * ax + T.R[1] * ay + T.R[2] * az + (double)T.m[12];  // T * a in FP64, as the passes
      const double tay = T.R[3] * ax + T.R[4] * ay + T.R[5] * az + (double)T.m[13];
      const double taz = T.R[6] * ax + T.R[7] * ay + T.R[8] * az + (double)T.m[14];
      const double* CA = a.covs + (size_t)i * 6;
      double ca[6], rcr[6];
#pragma unroll
      for (int e = 0; e < 6; ++e) ca[e] = CA[e];
      rotate_sym(T.R, ca, rcr);
      occupied = vox_fit_best_slot<K, true>(cx, cy, cz, a.table, a.mask, a.rec, tax, tay, taz, rcr, a.min_count, best, best_d, best_v);
    }
    bool kept;
    if (!occupied) {
      cls = kGateNew;
      kept = a.keep_new != 0;
    } else if (best_v < 0) {
      cls = kGateUnjudged;
      kept = a.keep_unjudged != 0;
    } else {
      kept = best <= a.max_m;
      cls = kept ? kGateExplained : kGateConflict;
    }
    a.cls[o] = (unsigned char)cls;
    a.keep[o] = kept ? 1 : 0;
  }
  // the block's class counts: integers, so nothing depends on the order in which blocks arrive
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = __popcll(__ballot(cls == k));
    if (lane == 0) wave_cnt[wave][k] = c;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kGateBlock / 64; ++w) s += wave_cnt[w][threadIdx.x];
    if (s) atomicAdd(a.counts + threadIdx.x, s);
  }
}

// kept point o -> pair rank[o] at the front of the pair arrays (rank: the exclusive prefix of keep, so ascending original index stays).
// A template only for its place in the code object (see the head of this file).
template <int W>
__global__ void __launch_bounds__(256) k_roll_gate_scatter(const int* __restrict__ keep, const int* __restrict__ rank, int n, const unsigned long long* __restrict__ keys_in,
                                                            const int* __restrict__ vals_in, unsigned long long* __restrict__ keys, int* __restrict__ vals) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n || !keep[o]) return;
  const int w = rank[o];
  keys[w] = keys_in[o];
  vals[w] = vals_in[o];
}

}  // namespace ngk
