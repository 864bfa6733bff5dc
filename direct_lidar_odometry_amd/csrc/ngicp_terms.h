// The terms of one correspondence, the only definition of each: K3 (lin_terms), K4's error leg (err_term), the robust kernel
// (robust_term) and the two legs under it, with the layout of a row of partial sums they add into.
// Needed by every pass kernel, exact and voxelized, and by the solver for the layout; all of them reach it through ngicp_pass.h
// (ngicp_voxel.h and ngicp_robust.h too: they also need the state and the pose of ngicp_lm.h).  The host reads the constants.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ngicp.h"

namespace ngk {

constexpr int kPartialStride = 32;  // doubles per block partial: 21 H + 6 b + y0 + yi (+3 pad)
constexpr int kNumSums = 29;
constexpr int kNumSlots = 32;      // + candidates tested, valid correspondences, queries served through the LDS row list (exact integers carried as doubles)
constexpr int kTraceCols = 8;

// K3 of one correspondence, the only definition (every pass kernel, exact and voxelized, calls it): residual e = b - T a, Mahalanobis
// matrix M = {m00, m01, m02, m11, m12, m22}, Ta = T a; adds y0 to acc[27], H's upper triangle to acc[0..20] and b to acc[21..26]
// (impl/nano_gicp_impl.hpp:232-257).  Statement order and parentheses are the result's bits: nothing here may be reassociated or fused.
__device__ __forceinline__ void lin_terms(double (&acc)[kNumSums], const double tax, const double tay, const double taz, const double ex, const double ey, const double ez,
                                          const double (&M)[6]) {
  const double m00 = M[0], m01 = M[1], m02 = M[2], m11 = M[3], m12 = M[4], m22 = M[5];
  const double mex = m00 * ex + m01 * ey + m02 * ez;
  const double mey = m01 * ex + m11 * ey + m12 * ez;
  const double mez = m02 * ex + m12 * ey + m22 * ez;
  acc[27] += ex * mex + ey * mey + ez * mez;
  // J = [S | -I], S = skew(Ta).   A = S*M  (column j of A = Ta x M[:,j]) = H_rot,trans block
  const double A00 = tay * m02 - taz * m01, A10 = taz * m00 - tax * m02, A20 = tax * m01 - tay * m00;
  const double A01 = tay * m12 - taz * m11, A11 = taz * m01 - tax * m12, A21 = tax * m11 - tay * m01;
  const double A02 = tay * m22 - taz * m12, A12 = taz * m02 - tax * m22, A22 = tax * m12 - tay * m02;
  // H_rr = S^T M S = -(A S);  S columns: (0,az,-ay) (-az,0,ax) (ay,-ax,0)
  acc[0] += -(A01 * taz - A02 * tay);   // (0,0)
  acc[1] += -(-A00 * taz + A02 * tax);  // (0,1)
  acc[2] += -(A00 * tay - A01 * tax);   // (0,2)
  acc[6] += -(-A10 * taz + A12 * tax);  // (1,1)
  acc[7] += -(A10 * tay - A11 * tax);   // (1,2)
  acc[11] += -(A20 * tay - A21 * tax);  // (2,2)
  // H_rt = -S^T M = S M = A   rows 0..2, cols 3..5
  acc[3] += A00; acc[4] += A01; acc[5] += A02;
  acc[8] += A10; acc[9] += A11; acc[10] += A12;
  acc[12] += A20; acc[13] += A21; acc[14] += A22;
  // H_tt = M
  acc[15] += m00; acc[16] += m01; acc[17] += m02;
  acc[18] += m11; acc[19] += m12;
  acc[20] += m22;
  // b = J^T M e = [ S^T Me ; -Me ],  S^T v = v x Ta
  acc[21] += mey * taz - mez * tay;
  acc[22] += mez * tax - mex * taz;
  acc[23] += mex * tay - mey * tax;
  acc[24] += -mex;
  acc[25] += -mey;
  acc[26] += -mez;
}

// the error leg alone: e^T M e with M read from six doubles in memory, in lin_terms' order of operations
__device__ __forceinline__ double err_term(const double ex, const double ey, const double ez, const double* M) {
  const double m00 = M[0], m01 = M[1], m02 = M[2], m11 = M[3], m12 = M[4], m22 = M[5];
  const double mex = m00 * ex + m01 * ey + m02 * ez;
  const double mey = m01 * ex + m11 * ey + m12 * ez;
  const double mez = m02 * ex + m12 * ey + m22 * ez;
  return ex * mex + ey * mey + ez * mez;
}

// The robust kernel of one term (include/ngicp.h, "robust kernel"), the only definition: s = e^T M e -> rho(s) and w(s) = d rho / d s.
// kind is wave-uniform (an argument of the launch); c2 = c * c.  A term with !(s > 0) passes through as under NONE.  An inlier weight
// is exactly 1.0 and its rho exactly s, so that scaling M by it changes no bit.
__device__ __forceinline__ void robust_term(const int kind, const double c, const double c2, const double s, double& rho, double& w) {
  rho = s;
  w = 1.0;
  if (!(s > 0.0)) return;
  if (kind == NGICP_ROBUST_HUBER) {
    if (!(s <= c2)) {
      const double r = sqrt(s);
      rho = 2.0 * c * r - c2;
      w = c / r;
    }
  } else if (kind == NGICP_ROBUST_CAUCHY) {
    const double u = s / c2;
    rho = c2 * log1p(u);
    w = 1.0 / (1.0 + u);
  } else if (kind == NGICP_ROBUST_GEMAN_MCCLURE) {
    const double q = c2 / (c2 + s);
    rho = s * q;
    w = q * q;
  }
}

// K3 of one term under a robust kernel: s in err_term's order, M scaled by w, lin_terms, and the y0 slot takes rho instead of w s.
// M itself (what the pass stores) stays unweighted.
__device__ __forceinline__ void lin_terms_robust(double (&acc)[kNumSums], const int kind, const double c, const double c2, const double tax, const double tay, const double taz,
                                                 const double ex, const double ey, const double ez, const double (&M)[6]) {
  double rho, w;
  robust_term(kind, c, c2, err_term(ex, ey, ez, M), rho, w);
  double Mw[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) Mw[e] = w * M[e];
  const double y0 = acc[27];
  lin_terms(acc, tax, tay, taz, ex, ey, ez, Mw);
  acc[27] = y0 + rho;
}

// the error leg of one term under a robust kernel: rho(e^T M e)
__device__ __forceinline__ double err_term_robust(const int kind, const double c, const double c2, const double ex, const double ey, const double ez, const double* M) {
  double rho, w;
  robust_term(kind, c, c2, err_term(ex, ey, ez, M), rho, w);
  return rho;
}

}  // namespace ngk
