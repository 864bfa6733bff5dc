// k_robust_terms: what the robust kernel makes of every term at a pose T, under the correspondences and the (unweighted) matrices of the
// last linearisation - ngicp_compute_error's contract, term by term instead of summed (include/ngicp.h, "robust kernel").
//
// A thread serves one source point and its K slots (K = 1: the exact route and DIRECT1).  Per term it writes s = e^T M e (err_term's
// order of operations, as the passes' error leg) and w(s) (robust_term, ngicp_terms.h: the passes' own definition); where the slot has no
// correspondence, s = -1 and w = 0.  Rows are in ORIGINAL source order, (n_src, K) doubles each:
//   exact      points come in the pass's query order (qpts, w = sorted source position); correspondence and target point from tpt,
//              the matrix from mahal[i]; the row is that of ngicp_get_correspondences (k_corr_to_original)
//   voxelized  points come in the index's sorted order (w = original index); voxel numbers and matrices slot-major
//              (slot s of point i at [s * slot_stride + i]), the mean from the voxel's record
#pragma once
#include "ngicp_voxel.h"

namespace ngk {

struct RobustTermsArgs {
  const float4* pts;         // exact: qpts; voxelized: the sorted source
  const float4* src_sorted;  // exact: the sorted source (its w is the original index); voxelized: null
  const float4* tpt;         // exact: [n] {target point, bitcast(sorted target position or -1)}; voxelized: null
  const int* corr;           // voxelized: [K][slot_stride] voxel numbers or -1
  const double* rec;         // voxelized: [n_vox][kVoxRec]
  int n_vox;
  const double* mahal;       // exact: [n][6]; voxelized: [K][slot_stride][6]
  int n, K, slot_stride;
  Pose T;
  int kind;
  double c, c2;
  double* out_s;             // [n][K], original source order
  double* out_w;
};

__global__ void __launch_bounds__(256) k_robust_terms(RobustTermsArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const float4 sp = a.pts[i];
  const double ax = (double)sp.x, ay = (double)sp.y, az = (double)sp.z;
  const double* R = a.T.R;
  const double* t = a.T.t;
  const double tax = R[0] * ax + R[1] * ay + R[2] * az + t[0];  // T * a in FP64, as the passes
  const double tay = R[3] * ax + R[4] * ay + R[5] * az + t[1];
  const double taz = R[6] * ax + R[7] * ay + R[8] * az + t[2];
  const bool exact = a.tpt != nullptr;
  const int o = exact ? __float_as_int(a.src_sorted[__float_as_int(sp.w)].w) : __float_as_int(sp.w);
  for (int s = 0; s < a.K; ++s) {
    double bx = 0.0, by = 0.0, bz = 0.0;
    const double* M = nullptr;
    if (exact) {
      const float4 bp = a.tpt[i];
      if (__float_as_int(bp.w) >= 0) {
        bx = (double)bp.x, by = (double)bp.y, bz = (double)bp.z;
        M = a.mahal + (size_t)i * 6;
      }
    } else {
      const int v = a.corr[(size_t)s * a.slot_stride + i];
      if ((unsigned int)v < (unsigned int)a.n_vox) {
        const double* mv = a.rec + (size_t)v * kVoxRec;
        bx = mv[0], by = mv[1], bz = mv[2];
        M = a.mahal + ((size_t)s * a.slot_stride + i) * 6;
      }
    }
    double sv = -1.0, w = 0.0;
    if (M) {
      double rho;
      sv = err_term(bx - tax, by - tay, bz - taz, M);
      robust_term(a.kind, a.c, a.c2, sv, rho, w);
    }
    a.out_s[(size_t)o * a.K + s] = sv;
    a.out_w[(size_t)o * a.K + s] = w;
  }
}

}  // namespace ngk
