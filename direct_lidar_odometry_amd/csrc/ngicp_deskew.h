// Motion deskew of a scan from per-point times and a pose trajectory (include/ngicp.h "motion deskew"; restated
// in numpy float64 by tests/_deskew_model.py).  No counterpart in the reference: DLO treats a sweep as one rigid snapshot.
//   k_deskew_prepare   the caller's trajectory -> the table {tau_k, R'_k, t'_k, phi_k} relative to the reference pose, once per call
//   k_deskew_unpack    k_unpack_xyzi with the pose at each point's own time applied: raw strided bytes -> float4 {x', y', z', intensity}
// Everything is FP64 in the element expressions of ngicp_math.h (pose_mul_r, pose_mul_t, so3_log, so3_exp_matrix), rounded once to
// float32 at the store; the build is -ffp-contract=off, so the operand order below is the arithmetic.
#pragma once
#include "ngicp_math.h"

namespace ngk {

constexpr int kDeskewMaxPoses = 256;  // NGICP_DESKEW_MAX_POSES
constexpr int kDeskewRec = 15;        // per pose: R'_k row-major (9), t'_k (3), phi_k (3; zero for the last pose)
// The table in device memory and in LDS, 16 doubles per pose: tau[0..M) first, so that the bracket search walks a dense array (a
// wave's lanes read one or two addresses of it per step: a broadcast), then the M records.
__host__ __device__ inline size_t deskew_table_doubles(int M) { return (size_t)M * (1 + kDeskewRec); }

// pose k of the uploaded trajectory (column-major 4x4) relative to the reference: R' = R_ref^T R_k, t' = R_ref^T (t_k - t_ref)
__device__ __forceinline__ void deskew_relative(const double* __restrict__ Tref, const double* __restrict__ Tk, double R[9], double t[3]) {
  const double d0 = Tk[12] - Tref[12], d1 = Tk[13] - Tref[13], d2 = Tk[14] - Tref[14];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = pose_mul_r(Tref[i * 4 + 0], Tref[i * 4 + 1], Tref[i * 4 + 2], Tk[j * 4 + 0], Tk[j * 4 + 1], Tk[j * 4 + 2]);
    t[i] = pose_mul_r(Tref[i * 4 + 0], Tref[i * 4 + 1], Tref[i * 4 + 2], d0, d1, d2);
  }
}

// in: pose_times [M], poses column-major [M][16], T_ref column-major [16].  One thread per pose; thread k < M - 1 also owns segment k.
__global__ void __launch_bounds__(kDeskewMaxPoses) k_deskew_prepare(const double* __restrict__ in, int M, double* __restrict__ table) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= M) return;
  const double* poses = in + M;
  const double* Tref = poses + (size_t)M * 16;
  double R[9], t[3], phi[3] = {0.0, 0.0, 0.0};
  deskew_relative(Tref, poses + (size_t)k * 16, R, t);
  if (k < M - 1) {
    double Rn[9], tn[3], D[9];
    deskew_relative(Tref, poses + (size_t)(k + 1) * 16, Rn, tn);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) D[i * 3 + j] = pose_mul_r(R[0 * 3 + i], R[1 * 3 + i], R[2 * 3 + i], Rn[0 * 3 + j], Rn[1 * 3 + j], Rn[2 * 3 + j]);
    so3_log(D, phi);
  }
  table[k] = in[k];
  double* rec = table + M + (size_t)k * kDeskewRec;
#pragma unroll
  for (int e = 0; e < 9; ++e) rec[e] = R[e];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    rec[9 + e] = t[e];
    rec[12 + e] = phi[e];
  }
}

// Where a point's time is read from and how it becomes seconds: s = double(raw) * unit + offset (two roundings, in that order).
struct DeskewTimes {
  const unsigned char* base;  // the separately uploaded array, or the point records themselves
  size_t stride;              // bytes between two points' times
  size_t first;               // byte of point 0's time
  int format;                 // NGICP_TIME_*
  double unit, offset;
};

__device__ __forceinline__ double deskew_time(const DeskewTimes& tm, int i) {
  const unsigned char* b = tm.base + tm.first + (size_t)i * tm.stride;
  double raw;
  if (tm.format == 0) raw = (double)*reinterpret_cast<const float*>(b);
  else if (tm.format == 1) raw = *reinterpret_cast<const double*>(b);
  else raw = (double)*reinterpret_cast<const unsigned int*>(b);
  return raw * tm.unit + tm.offset;
}

// One thread per point.  kPacked: 12 bytes per point out (ngicp_deskew_cloud) instead of float4 {x, y, z, intensity}.
// Dynamic LDS: the table, deskew_table_doubles(M) * 8 bytes (32 KB at M = 256: five blocks per CU by LDS, four by the guideline).
// A result depends on the point's own bytes and the table only: not on n, the grid or a neighbour.
template <bool kPacked>
__global__ void __launch_bounds__(256) k_deskew_unpack(const unsigned char* __restrict__ raw, size_t stride_bytes, long intensity_offset, DeskewTimes tm,
                                                        const double* __restrict__ table, int M, int n, float* __restrict__ out) {
  extern __shared__ double tab[];
  const int n_tab = (int)deskew_table_doubles(M);
  for (int e = threadIdx.x; e < n_tab; e += blockDim.x) tab[e] = table[e];
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned char* b = raw + (size_t)i * stride_bytes;
  const float* p = reinterpret_cast<const float*>(b);
  float x = p[0], y = p[1], z = p[2];
  const float w = (!kPacked && intensity_offset >= 0) ? *reinterpret_cast<const float*>(b + intensity_offset) : 0.f;
  if (isfinite(x) && isfinite(y) && isfinite(z)) {  // a non-finite point is copied as it is
    const double s = deskew_time(tm, i);
    if (!isfinite(s)) {
      x = y = z = __int_as_float(0x7fc00000);  // removeNaN drops it, rather than leaving it skewed unnoticed
    } else {
      int lo = 0, hi = M - 2;  // the largest k in [0, M - 2] with tau_k <= s, 0 when there is none: at most 8 steps
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid] <= s) lo = mid; else hi = mid - 1;
      }
      const double t0 = tab[lo], t1 = tab[lo + 1];
      double alpha = (s - t0) / (t1 - t0);
      if (alpha < 0.0) alpha = 0.0;
      if (alpha > 1.0) alpha = 1.0;
      const double* rec = tab + M + lo * kDeskewRec;
      double Rk[9], tk[3], aphi[3], E[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) Rk[e] = rec[e];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const double a = rec[9 + e], bnext = rec[kDeskewRec + 9 + e];
        tk[e] = a + alpha * (bnext - a);
        aphi[e] = alpha * rec[12 + e];
      }
      so3_exp_matrix(aphi, E);
      const double px = (double)x, py = (double)y, pz = (double)z;
      float o[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double r0 = pose_mul_r(Rk[r * 3 + 0], Rk[r * 3 + 1], Rk[r * 3 + 2], E[0], E[3], E[6]);
        const double r1 = pose_mul_r(Rk[r * 3 + 0], Rk[r * 3 + 1], Rk[r * 3 + 2], E[1], E[4], E[7]);
        const double r2 = pose_mul_r(Rk[r * 3 + 0], Rk[r * 3 + 1], Rk[r * 3 + 2], E[2], E[5], E[8]);
        o[r] = (float)pose_mul_t(r0, r1, r2, px, py, pz, tk[r]);
      }
      x = o[0]; y = o[1]; z = o[2];
    }
  }
  if (kPacked) {
    float* d = out + (size_t)i * 3;
    d[0] = x; d[1] = y; d[2] = z;
  } else {
    reinterpret_cast<float4*>(out)[i] = make_float4(x, y, z, w);
  }
}

}  // namespace ngk
