// Voxel fitness (include/ngicp.h "voxel fitness"): how well a pose explains the source against the voxel map the handle
// aligns against - the target's, the merged one or the rolling one - without a target cloud or an exact index.  The project's own
// definition; a query: nothing an alignment or a hook left on the handle is read or written.
//
//   k_voxel_fitness<K, POINTS>   grid (ceil(n / 256), poses), 256 threads: one thread per source point in the index's sorted order, row
//                                blockIdx.y serves pose blockIdx.y of T_colmajor[poses][16].  The pose is read through the constant
//                                address space (scalar loads: it is uniform per block), as the batch passes read their lane's record.
//                                  q     the float pose times the point in the passes' order, ((c0 x + c1 y) + c2 z) + c3
//                                        (transform_point_rowmajor_f on the transposed entries), its cell from voxel_cell
//                                  slot  s = 0..K-1 is voxel c + off[s] under the passes' rule: the centre and the neighbour in range on
//                                        the integers, the voxel occupied.  No occupied slot: the point is unmatched.
//                                  term  FP64, R and t the float entries widened: e = mean_v - (R a + t) in the order of the passes'
//                                        tax / tay / taz, M = inv3_sym(cov_v + rotate_sym(R, C_a)), m = err_term(e, M) - the pass's term
//                                        WITHOUT the factor n_v - and d = (ex ex + ey ey) + ez ez
//                                  value best = +inf; in ascending slot, slot s wins when m_s < best (ties to the lower slot, a NaN never
//                                        wins).  No winner among the occupied slots: m = d = +inf, v = -1, matched and never an inlier.
//                                  inlier  m <= max_m
//                                Slots are looked up and evaluated one after the other in ONE rolled loop (vox_fit_best_slot, which the
//                                gated insert's k_roll_gate shares, ngicp_voxel_gate.h): no thread holds K voxel numbers, so there is
//                                no LDS column per thread and no scratch.  The block's partial is four doubles
//                                {sum m, sum d over the inliers, inliers, matched} (counts as doubles: exact), reduced in a fixed order:
//                                a lane's value, the wave's butterflies (wave_sum, ngicp_query.h), the four waves in order.
//                                POINTS (single pose): also m, d, v by ORIGINAL index (p.w); unmatched is -1 / -1 / -1 (the convention
//                                of k_robust_terms).
//   k_voxel_fitness_final        one block per pose: its block partials strided per thread, butterflies, waves in order - the shape
//                                of k_fitness_final on four doubles.  A pose's four sums therefore do not depend on the number of poses
//                                in the launch: lane g of a batch is the single call bit for bit.
#pragma once
#include "ngicp_query.h"
#include "ngicp_voxel.h"

namespace ngk {

constexpr int kVoxFitBlock = 256;       // source points per block
constexpr int kVoxFitFinalBlock = 256;
constexpr int kVoxFitSums = 4;          // {sum m, sum d, inliers, matched}
constexpr int kVoxelFitnessChunk = 4096;  // poses per launch (the grid's y limit is 65535; ngicp_fitness_score_batch cuts at the same number)

struct VoxelFitnessArgs {
  const float4* src;        // source points in the index's sorted order, w = original index
  const double* cov_src;    // [n_src][6], the same order
  int n_src;
  const ulonglong2* table;  // the voxel map's hash table, records and resolution (VoxelPassArgs' fields)
  unsigned int mask;
  const double* rec;
  float inv_res;
  const float* T_colmajor;  // [poses][16]
  double max_m;             // the gate: a point is an inlier iff m <= max_m
  double* partials;         // [poses][blocks][kVoxFitSums]
  double* pt_m;             // POINTS: [n_src] each, original source order
  double* pt_d;
  int* pt_v;
};

typedef const float __attribute__((address_space(4))) KernelPoseFloat;

// offset of slot s on `axis`, s a run-time value (vox_nbr_off is defined for K = 7 and 27; DIRECT1 is its centre alone)
template <int K>
__device__ __forceinline__ int vox_fit_off(int s, int axis) {
  if constexpr (K == 1) return 0;
  else return vox_nbr_off<K>(s, axis);
}

// The slots of a point whose cell is c, looked up and evaluated one after the other in ONE rolled loop (the head of this file: slot,
// term, value).  ta = T a in FP64, rcr = R C_a R^T.  COUNT (the gated insert, ngicp_voxel_gate.h): an occupied slot is evaluated only
// when its voxel's count is at least min_count.  Returns whether any slot is occupied; best / best_d / best_v keep the winner's.
template <int K, bool COUNT>
__device__ __forceinline__ bool vox_fit_best_slot(int cx, int cy, int cz, const ulonglong2* __restrict__ table, unsigned int mask, const double* __restrict__ rec, double tax,
                                                  double tay, double taz, const double (&rcr)[6], double min_count, double& best, double& best_d, int& best_v) {
  bool matched = false;
  unsigned int probes = 0;  // (voxel_lookup counts them; nobody asks here)
#pragma unroll 1
  for (int s = 0; s < K; ++s) {
    const int nx = cx + vox_fit_off<K>(s, 0), ny = cy + vox_fit_off<K>(s, 1), nz = cz + vox_fit_off<K>(s, 2);
    if (!(nx > -kVoxBias && nx < kVoxBias && ny > -kVoxBias && ny < kVoxBias && nz > -kVoxBias && nz < kVoxBias)) continue;
    const int v = voxel_lookup(table, mask, voxel_pack(nx, ny, nz), probes);
    if (v < 0) continue;
    matched = true;
    const double* rv = rec + (size_t)v * kVoxRec;
    if constexpr (COUNT) {
      if (!(rv[9] >= min_count)) continue;
    }
    double S[6], M[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) S[e] = rv[3 + e] + rcr[e];
    inv3_sym(S, M);
    const double ex = rv[0] - tax, ey = rv[1] - tay, ez = rv[2] - taz;
    const double m = err_term(ex, ey, ez, M);
    if (m < best) {
      best = m;
      best_d = (ex * ex + ey * ey) + ez * ez;
      best_v = v;
    }
  }
  return matched;
}

template <int K, bool POINTS>
__global__ void __launch_bounds__(kVoxFitBlock) k_voxel_fitness(VoxelFitnessArgs a) {
  static_assert(K == 1 || K == 7 || K == 27, "DIRECT1, DIRECT7 or DIRECT27");
  __shared__ double wave_part[kVoxFitBlock / 64][kVoxFitSums];
  KernelPoseFloat* Tm = (KernelPoseFloat*)(unsigned long long)(a.T_colmajor + (size_t)blockIdx.y * 16);
  float Tf[12];  // row-major 3x4, the layout of the passes' float pose
  double R[9], t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) Tf[r * 4 + c] = Tm[c * 4 + r];
#pragma unroll
    for (int c = 0; c < 3; ++c) R[r * 3 + c] = (double)Tf[r * 4 + c];
    t[r] = (double)Tf[r * 4 + 3];
  }
  const int i = blockIdx.x * kVoxFitBlock + threadIdx.x;
  double sm = 0.0, sd = 0.0, n_in = 0.0, n_match = 0.0;
  if (i < a.n_src) {
    const float4 sp = a.src[i];
    const float3 q = transform_point_rowmajor_f(Tf, sp.x, sp.y, sp.z);
    bool matched = false;
    double best = __builtin_inf(), best_d = __builtin_inf();
    int best_v = -1;
    int cx, cy, cz;
    if (voxel_cell(q.x, q.y, q.z, a.inv_res, cx, cy, cz)) {
      const double ax = (double)sp.x, ay = (double)sp.y, az = (double)sp.z;
      const double tax = R[0] * ax + R[1] * ay + R[2] * az + t[0];  // T * a in FP64, as the passes
      const double tay = R[3] * ax + R[4] * ay + R[5] * az + t[1];
      const double taz = R[6] * ax + R[7] * ay + R[8] * az + t[2];
      const double* CA = a.cov_src + (size_t)i * 6;
      double ca[6], rcr[6];
#pragma unroll
      for (int e = 0; e < 6; ++e) ca[e] = CA[e];
      rotate_sym(R, ca, rcr);
      matched = vox_fit_best_slot<K, false>(cx, cy, cz, a.table, a.mask, a.rec, tax, tay, taz, rcr, 0.0, best, best_d, best_v);
    }
    if (matched) {
      n_match = 1.0;
      if (best <= a.max_m) {
        sm = best;
        sd = best_d;
        n_in = 1.0;
      }
    }
    if constexpr (POINTS) {
      const int o = __float_as_int(sp.w);
      a.pt_m[o] = matched ? best : -1.0;
      a.pt_d[o] = matched ? best_d : -1.0;
      a.pt_v[o] = best_v;
    }
  }
  sm = wave_sum(sm);
  sd = wave_sum(sd);
  n_in = wave_sum(n_in);
  n_match = wave_sum(n_match);
  if ((threadIdx.x & 63) == 0) {
    double* w = wave_part[threadIdx.x >> 6];
    w[0] = sm, w[1] = sd, w[2] = n_in, w[3] = n_match;
  }
  __syncthreads();
  if (threadIdx.x < kVoxFitSums) {
    const int k = threadIdx.x;
    double r = wave_part[0][k];
#pragma unroll
    for (int w = 1; w < kVoxFitBlock / 64; ++w) r += wave_part[w][k];
    a.partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kVoxFitSums + k] = r;
  }
}

// block l: out[l][k] = the sum of partials[l * nb .. l * nb + nb)[k], in a fixed order (strided per thread, then wave butterflies, then
// the waves in order): k_fitness_final's shape on records of W doubles.  A template, although only W = kVoxFitSums is used: the
// compiler then emits it behind every kernel the library had, with k_voxel_fitness's instantiations, and the code object up to there -
// the pass kernels among it - is laid out as it was without this header (as a plain kernel it sat in front of them and moved them all).
template <int W>
__global__ void __launch_bounds__(kVoxFitFinalBlock) k_voxel_fitness_final(const double* __restrict__ partials, int nb, double* __restrict__ out) {
  __shared__ double wave_part[kVoxFitFinalBlock / 64][W];
  const double* __restrict__ mine = partials + (size_t)blockIdx.x * nb * W;
  double s[W];
#pragma unroll
  for (int k = 0; k < W; ++k) s[k] = 0.0;
  for (int b = threadIdx.x; b < nb; b += kVoxFitFinalBlock) {
#pragma unroll
    for (int k = 0; k < W; ++k) s[k] += mine[(size_t)b * W + k];
  }
#pragma unroll
  for (int k = 0; k < W; ++k) s[k] = wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < W; ++k) wave_part[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < W) {
    const int k = threadIdx.x;
    double r = wave_part[0][k];
#pragma unroll
    for (int w = 1; w < kVoxFitFinalBlock / 64; ++w) r += wave_part[w][k];
    out[(size_t)blockIdx.x * W + k] = r;
  }
}

}  // namespace ngk
