// The on-device pose-graph optimiser (include/ngicp.h "pose graph").  The project's own definition: the reference has
// no counterpart.  Part of ngicp_api.hip's translation unit (included there behind every other kernel).  FP64 throughout.
//
// The definition in one place (include/ngicp.h restates it, tests/_pose_graph_model.py is its numpy model):
//   edge (i, j, Z, Lambda):  E = Z^-1 T_i^-1 T_j,  r = (so3_log(R_E), t_E),  s = r^T Lambda r,  (rho, w) = robust_term(s) when the edge is
//   flagged and a kernel is chosen, (s, 1) otherwise.  With A = Z^-1 T_i^-1 and the project's perturbation T_k <- (so3_exp(d_w), d_t) T_k:
//       J_j = [[Jl^-1(phi) R_A, 0], [-R_A [t_j]x, R_A]],      J_i = -J_j
//   (a common left perturbation of both ends leaves T_i^-1 T_j alone), so that ONE block per edge carries the whole linearisation:
//       M = J_j^T (w Lambda) J_j = J_i^T wL J_i = -J_i^T wL J_j,      g = J_j^T (w Lambda) r = -J_i^T wL r
//   H's diagonal block of node k is the sum of M over its incident edges, its gradient the sum of +g (k is the edge's j) or -g (its i),
//   and (H x)_k = sum over incident edges of M (x_k - x_other), with x = 0 at fixed nodes.  Every per-node sum runs over the node's
//   incidence list (ngicp_pose_graph_plan.h) in ascending edge id.
//
// Kernels (256 threads; a thread per edge or per node; no floating-point atomics, no inter-block communication inside a launch):
//   k_pg_linearize   per edge: r, s, rho, w, M (upper triangle, 21), g - 36 doubles per edge - and the block's sum of rho
//   k_pg_assemble    per free node: diagonal block and gradient over its list; the block's largest |diagonal entry|
//   k_pg_lin_reduce  one block: chi2 from the blocks' sums of rho; the largest diagonal entry (the initial lambda's rule)
//   k_pg_precond     per free node: (D + lambda I)^-1 column by column with ldlt6_solve; x = 0, r = -b, z = M^-1 r, p = z; block sums r.z, r.r
//   k_pg_cg_start    one block: r.z and |b|^2 into the scalars; the solve is over at once when b = 0
//   k_pg_cg_matvec   q = (H + lambda I) p and the block sums of p.q
//   k_pg_cg_step     every block adds up p.q for itself -> alpha; x += alpha p, r -= alpha q, z = M^-1 r; block sums r.z, r.r
//   k_pg_cg_dir      every block adds up r.z, r.r for itself -> the stop (|r| <= cg_tol |b|) or beta and p = z + beta p; block 0 records it
//   k_pg_update      trial pose = (so3_exp(x_w), x_t) * pose for free nodes; block sums of x.(lambda x - b), block maxima of the step sizes
//   k_pg_try_reduce  one block: the gain ratio's denominator, the two step sizes, the trial's chi2
//   k_pg_multiply    the test hook: y = (H + lambda I) x at the current linearisation
//   k_pg_corrections C_k = T_k T_k_old^-1 in FP64, rounded to the float column-major 4x4 the keyframe and voxel-map moves take
// A dot product is a fixed tree: a thread's six products in order, the block's 256 values through LDS in halving strides, then the blocks'
// sums by ONE block's threads striding over them in ascending order and the same tree.  Two runs on the same input are bit-equal.
// Within a linear solve nothing synchronises the host: `done_at` (the iteration at which the solve ended) lives in device memory and the
// launches of later iterations return at once; the word is mirrored into pinned memory, which the host glances at every 64 iterations
// so as to stop feeding the stream - when it looks has no influence on any result.
#pragma once
#include <hip/hip_runtime.h>

#include "ngicp_lm.h"
#include "ngicp_math.h"
#include "ngicp_pose_graph_plan.h"
#include "ngicp_terms.h"

namespace ngk {

constexpr int kPgBlock = 256;
constexpr int kPgLin = (int)ngpg::kEdgeLinDoubles;  // doubles per linearised edge: M 21, g 6, r 6, s, w, rho
constexpr int kPgG = 21, kPgR = 27, kPgS = 33, kPgW = 34, kPgRho = 35;
constexpr int kPgNotDone = 0x7fffffff;

struct PgScalars {
  double chi2[2];   // of the two linearisation buffers
  double maxdiag;
  double rz[2];     // r.z of CG iteration k in slot k & 1
  double bnorm2;
  double den, rot_max, trans_max;
  int done_at;      // the CG iteration that met the stop (-1: b = 0), kPgNotDone while running
  int iters;        // CG iterations done
  int breakdown;    // p.q <= 0 was met: the solve stopped there
  int pad;
};

struct PgGraphDev {
  int n, m;
  const int2* ij;              // [m]
  const double* Z;             // [m][12] R row-major, t
  const double* info;          // [m][36] row-major
  const unsigned char* eflag;  // [m] robust flags
  const unsigned char* fixed;  // [n]
  const int* off;              // [n + 1]
  const int* ent;              // [2 m] 2 * edge + side
};

// the block's sum in a fixed tree; every thread returns it
__device__ __forceinline__ double pg_block_sum(double v, double* lds) {
  __syncthreads();  // (lds may still be read from a previous call)
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kPgBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  return lds[0];
}
__device__ __forceinline__ double pg_block_max(double v, double* lds) {
  __syncthreads();
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kPgBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] = fmax(lds[threadIdx.x], lds[threadIdx.x + s]);
    __syncthreads();
  }
  return lds[0];
}
// the sum / maximum of nb block results: thread t takes t, t + 256, ... in ascending order, then the tree
__device__ __forceinline__ double pg_sum_partials(const double* part, int nb, double* lds) {
  double v = 0.0;
  for (int b = threadIdx.x; b < nb; b += kPgBlock) v += part[b];
  return pg_block_sum(v, lds);
}
__device__ __forceinline__ double pg_max_partials(const double* part, int nb, double* lds) {
  double v = 0.0;
  for (int b = threadIdx.x; b < nb; b += kPgBlock) v = fmax(v, part[b]);
  return pg_block_max(v, lds);
}

__device__ __forceinline__ double pg_dot6(const double* a, const double* b) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) s += a[i] * b[i];
  return s;
}
// y += M d, M symmetric, upper triangle in tri21's order
__device__ __forceinline__ void pg_sym21_mac(const double* __restrict__ M, const double* d, double* y) {
  double m[21];
#pragma unroll
  for (int e = 0; e < 21; ++e) m[e] = M[e];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) acc += m[tri21(r < c ? r : c, r < c ? c : r)] * d[c];
    y[r] += acc;
  }
}

struct PgLinArgs {
  PgGraphDev g;
  const double* poses;  // [n][12]
  double* lin;          // [m][kPgLin]
  double* part_chi2;    // [blocks]
  int kind;
  double c, c2;
};

template <int>
__global__ void __launch_bounds__(kPgBlock) k_pg_linearize(PgLinArgs a) {
  __shared__ double lds[kPgBlock];
  const int e = blockIdx.x * kPgBlock + threadIdx.x;
  double rho = 0.0;
  if (e < a.g.m) {
    const int2 ij = a.g.ij[e];
    const double* Ti = a.poses + (size_t)ij.x * 12;
    const double* Tj = a.poses + (size_t)ij.y * 12;
    const double* Z = a.g.Z + (size_t)e * 12;
    double Ri[9], Rj[9], Rz[9], tj[3], dij[3], tz[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) Ri[q] = Ti[q], Rj[q] = Tj[q], Rz[q] = Z[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) tj[q] = Tj[9 + q], dij[q] = Tj[9 + q] - Ti[9 + q], tz[q] = Z[9 + q];
    // R_A = R_z^T R_i^T;  R_E = R_A R_j;  t_E = R_z^T (R_i^T (t_j - t_i) - t_z)
    double RA[9], RE[9], u[3], tE[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) RA[r * 3 + c] = pose_mul_r(Rz[0 * 3 + r], Rz[1 * 3 + r], Rz[2 * 3 + r], Ri[c * 3 + 0], Ri[c * 3 + 1], Ri[c * 3 + 2]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) RE[r * 3 + c] = pose_mul_r(RA[r * 3 + 0], RA[r * 3 + 1], RA[r * 3 + 2], Rj[0 * 3 + c], Rj[1 * 3 + c], Rj[2 * 3 + c]);
#pragma unroll
    for (int r = 0; r < 3; ++r) u[r] = pose_mul_r(Ri[0 * 3 + r], Ri[1 * 3 + r], Ri[2 * 3 + r], dij[0], dij[1], dij[2]) - tz[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) tE[r] = pose_mul_r(Rz[0 * 3 + r], Rz[1 * 3 + r], Rz[2 * 3 + r], u[0], u[1], u[2]);
    double res[6];
    so3_log(RE, res);
    res[3] = tE[0], res[4] = tE[1], res[5] = tE[2];
    double Jinv[9];
    so3_left_jacobian_inv(res, Jinv);
    // J = [[P, 0], [Q, R_A]],  P = Jl^-1 R_A,  Q = -R_A [t_j]x
    double J[36];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        J[r * 6 + c] = pose_mul_r(Jinv[r * 3 + 0], Jinv[r * 3 + 1], Jinv[r * 3 + 2], RA[0 * 3 + c], RA[1 * 3 + c], RA[2 * 3 + c]);
        J[r * 6 + 3 + c] = 0.0;
        J[(3 + r) * 6 + 3 + c] = RA[r * 3 + c];
      }
      J[(3 + r) * 6 + 0] = -(RA[r * 3 + 1] * tj[2] - RA[r * 3 + 2] * tj[1]);
      J[(3 + r) * 6 + 1] = -(RA[r * 3 + 2] * tj[0] - RA[r * 3 + 0] * tj[2]);
      J[(3 + r) * 6 + 2] = -(RA[r * 3 + 0] * tj[1] - RA[r * 3 + 1] * tj[0]);
    }
    // s = r^T (Lambda r), k and l ascending; then W = w Lambda
    const double* L = a.g.info + (size_t)e * 36;
    double Lr[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double acc = 0.0;
#pragma unroll
      for (int l = 0; l < 6; ++l) acc += L[k * 6 + l] * res[l];
      Lr[k] = acc;
    }
    const double s = pg_dot6(res, Lr);
    double w = 1.0;
    rho = s;
    if (a.kind != NGICP_ROBUST_NONE && a.g.eflag[e]) robust_term(a.kind, a.c, a.c2, s, rho, w);
    // WJ = (w Lambda) J;  M = J^T WJ (upper triangle);  g = J^T (w Lambda r)
    double WJ[36];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double acc = 0.0;
#pragma unroll
        for (int l = 0; l < 6; ++l) acc += (w * L[k * 6 + l]) * J[l * 6 + c];
        WJ[k * 6 + c] = acc;
      }
    double* out = a.lin + (size_t)e * kPgLin;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) acc += J[k * 6 + r] * WJ[k * 6 + c];
        out[tri21(r, c)] = acc;
      }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) acc += J[k * 6 + r] * (w * Lr[k]);
      out[kPgG + r] = acc;
      out[kPgR + r] = res[r];
    }
    out[kPgS] = s;
    out[kPgW] = w;
    out[kPgRho] = rho;
  }
  const double sum = pg_block_sum(rho, lds);
  if (threadIdx.x == 0) a.part_chi2[blockIdx.x] = sum;
}

// per free node: D (36, row-major, symmetric) and b; fixed nodes get zeros
template <int>
__global__ void __launch_bounds__(kPgBlock) k_pg_assemble(PgGraphDev g, const double* __restrict__ lin, double* __restrict__ diag, double* __restrict__ grad,
                                                          double* __restrict__ part_max) {
  __shared__ double lds[kPgBlock];
  const int k = blockIdx.x * kPgBlock + threadIdx.x;
  double top = 0.0;
  if (k < g.n) {
    double D[21], b[6];
#pragma unroll
    for (int q = 0; q < 21; ++q) D[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) b[q] = 0.0;
    if (!g.fixed[k]) {
      const int hi = g.off[k + 1];
      for (int p = g.off[k]; p < hi; ++p) {
        const int v = g.ent[p];
        const double* le = lin + (size_t)(v >> 1) * kPgLin;
        const double sign = (v & 1) ? 1.0 : -1.0;
#pragma unroll
        for (int q = 0; q < 21; ++q) D[q] += le[q];
#pragma unroll
        for (int q = 0; q < 6; ++q) b[q] += sign * le[kPgG + q];
      }
    }
    double* d = diag + (size_t)k * 36;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) d[r * 6 + c] = D[tri21(r < c ? r : c, r < c ? c : r)];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      grad[(size_t)k * 6 + q] = b[q];
      top = fmax(top, fabs(D[tri21(q, q)]));
    }
  }
  top = pg_block_max(top, lds);
  if (threadIdx.x == 0) part_max[blockIdx.x] = top;
}

template <int>
__global__ void __launch_bounds__(kPgBlock) k_pg_lin_reduce(PgScalars* sc, const double* part_chi2, int nb_e, int which, const double* part_max, int nb_n) {
  __shared__ double lds[kPgBlock];
  const double chi2 = pg_sum_partials(part_chi2, nb_e, lds);
  const double top = part_max ? pg_max_partials(part_max, nb_n, lds) : 0.0;
  if (threadIdx.x == 0) {
    sc->chi2[which] = chi2;
    if (part_max) sc->maxdiag = top;
  }
}

struct PgCgArgs {
  PgGraphDev g;
  const double* lin;
  const double* diag;   // [n][36]
  const double* grad;   // [n][6]
  double* minv;         // [n][36] (D + lambda I)^-1, column by column as solved; applied symmetrised
  double *x, *r, *z, *p, *q;  // [n][6]
  double *part_a, *part_b, *part_c;
  PgScalars* sc;
  int* host_done;       // pinned: set to 1 when the solve has ended
  double lambda, tol2;
  int nb;               // blocks over the nodes
  int k;                // the CG iteration of this launch
};

// z = sym(Minv) r
__device__ __forceinline__ void pg_apply_minv(const double* __restrict__ Mi, const double* r, double* z) {
  double m[36];
#pragma unroll
  for (int e = 0; e < 36; ++e) m[e] = Mi[e];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) acc += (0.5 * (m[i * 6 + j] + m[j * 6 + i])) * r[j];
    z[i] = acc;
  }
}

template <int>
__global__ void __launch_bounds__(kPgBlock) k_pg_precond(PgCgArgs a) {
  __shared__ double lds[kPgBlock];
  const int k = blockIdx.x * kPgBlock + threadIdx.x;
  double rz = 0.0, rr = 0.0;
  if (k < a.g.n) {
    double r[6], z[6];
    double* Mi = a.minv + (size_t)k * 36;
    if (a.g.fixed[k]) {
      for (int e = 0; e < 36; ++e) Mi[e] = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) r[i] = z[i] = 0.0;
    } else {
      const double* D = a.diag + (size_t)k * 36;
#pragma unroll 1
      for (int c = 0; c < 6; ++c) {
        double A[36], rhs[6], col[6];
#pragma unroll
        for (int e = 0; e < 36; ++e) A[e] = D[e];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          A[i * 6 + i] += a.lambda;
          rhs[i] = i == c ? 1.0 : 0.0;
        }
        ldlt6_solve(A, rhs, col);
#pragma unroll
        for (int i = 0; i < 6; ++i) Mi[i * 6 + c] = col[i];
      }
      __threadfence_block();  // (the thread reads its own stores back below)
#pragma unroll
      for (int i = 0; i < 6; ++i) r[i] = -a.grad[(size_t)k * 6 + i];
      pg_apply_minv(Mi, r, z);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const size_t o = (size_t)k * 6 + i;
      a.x[o] = 0.0;
      a.r[o] = r[i];
      a.z[o] = z[i];
      a.p[o] = z[i];
    }
    rz = pg_dot6(r, z);
    rr = pg_dot6(r, r);
  }
  rz = pg_block_sum(rz, lds);
  rr = pg_block_sum(rr, lds);
  if (threadIdx.x == 0) a.part_a[blockIdx.x] = rz, a.part_b[blockIdx.x] = rr;
}

template <int>
__global__ void __launch_bounds__(kPgBlock) k_pg_cg_start(PgCgArgs a) {
  __shared__ double lds[kPgBlock];
  const double rz = pg_sum_partials(a.part_a, a.nb, lds);
  const double rr = pg_sum_partials(a.part_b, a.nb, lds);
  if (threadIdx.x == 0) {
    a.sc->rz[0] = rz;
    a.sc->rz[1] = rz;
    a.sc->bnorm2 = rr;
    a.sc->iters = 0;
    a.sc->breakdown = 0;
    const bool over = !(rr > 0.0);
    a.sc->done_at = over ? -1 : kPgNotDone;
    if (over) __hip_atomic_store(a.host_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// (H + lambda I) x at node k over its incidence list; CHECK_FIXED: x of a fixed node counts as zero whatever the array holds
template <bool CHECK_FIXED>
__device__ __forceinline__ void pg_node_matvec(const PgGraphDev& g, const double* __restrict__ lin, const double* __restrict__ x, double lambda, int k, double* y) {
  double xi[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    xi[i] = x[(size_t)k * 6 + i];
    y[i] = lambda * xi[i];
  }
  const int hi = g.off[k + 1];
  for (int p = g.off[k]; p < hi; ++p) {
    const int v = g.ent[p];
    const int2 ij = g.ij[v >> 1];
    const int other = (v & 1) ? ij.x : ij.y;
    const bool zero = CHECK_FIXED && g.fixed[other];
    double d[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = xi[i] - (zero ? 0.0 : x[(size_t)other * 6 + i]);
    pg_sym21_mac(lin + (size_t)(v >> 1) * kPgLin, d, y);
  }
}

template <int>
__global__ void __launch_bounds__(kPgBlock) k_pg_cg_matvec(PgCgArgs a) {
  __shared__ double lds[kPgBlock];
  if (a.k > a.sc->done_at) return;
  const int k = blockIdx.x * kPgBlock + threadIdx.x;
  double pq = 0.0;
  if (k < a.g.n) {
    double y[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!a.g.fixed[k]) {
      pg_node_matvec<false>(a.g, a.lin, a.p, a.lambda, k, y);
      pq = pg_dot6(a.p + (size_t)k * 6, y);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) a.q[(size_t)k * 6 + i] = y[i];
  }
  pq = pg_block_sum(pq, lds);
  if (threadIdx.x == 0) a.part_a[blockIdx.x] = pq;
}

template <int>
__global__ void __launch_bounds__(kPgBlock) k_pg_cg_step(PgCgArgs a) {
  __shared__ double lds[kPgBlock];
  if (a.k > a.sc->done_at) return;
  const double pq = pg_sum_partials(a.part_a, a.nb, lds);
  const bool ok = pq > 0.0;
  const double alpha = ok ? a.sc->rz[a.k & 1] / pq : 0.0;
  const int k = blockIdx.x * kPgBlock + threadIdx.x;
  double rz = 0.0, rr = 0.0;
  if (k < a.g.n && !a.g.fixed[k]) {
    double r[6], z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const size_t o = (size_t)k * 6 + i;
      a.x[o] = a.x[o] + alpha * a.p[o];
      r[i] = a.r[o] - alpha * a.q[o];
      a.r[o] = r[i];
    }
    pg_apply_minv(a.minv + (size_t)k * 36, r, z);
#pragma unroll
    for (int i = 0; i < 6; ++i) a.z[(size_t)k * 6 + i] = z[i];
    rz = pg_dot6(r, z);
    rr = pg_dot6(r, r);
  }
  rz = pg_block_sum(rz, lds);
  rr = pg_block_sum(rr, lds);
  if (threadIdx.x == 0) {
    a.part_b[blockIdx.x] = rz, a.part_c[blockIdx.x] = rr;
    if (blockIdx.x == 0 && !ok) a.sc->breakdown = 1;
  }
}

template <int>
__global__ void __launch_bounds__(kPgBlock) k_pg_cg_dir(PgCgArgs a) {
  __shared__ double lds[kPgBlock];
  if (a.k > a.sc->done_at) return;
  const double rz_new = pg_sum_partials(a.part_b, a.nb, lds);
  const double rr = pg_sum_partials(a.part_c, a.nb, lds);
  const bool broke = a.sc->breakdown != 0;
  const bool over = broke || rr <= a.tol2 * a.sc->bnorm2;
  const int k = blockIdx.x * kPgBlock + threadIdx.x;
  if (!over && k < a.g.n && !a.g.fixed[k]) {
    const double beta = rz_new / a.sc->rz[a.k & 1];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const size_t o = (size_t)k * 6 + i;
      a.p[o] = a.z[o] + beta * a.p[o];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.sc->rz[(a.k + 1) & 1] = rz_new;
    a.sc->iters = broke ? a.k : a.k + 1;
    if (over) {
      a.sc->done_at = a.k;  // (a reader of this launch compares k > done_at: false for the old value and for this one)
      __hip_atomic_store(a.host_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

struct PgUpdateArgs {
  PgGraphDev g;
  const double* poses;  // [n][12]
  double* trial;        // [n][12]
  const double* x;      // [n][6] the step
  const double* grad;
  double *part_a, *part_b, *part_c;
  double lambda;
};

template <int>
__global__ void __launch_bounds__(kPgBlock) k_pg_update(PgUpdateArgs a) {
  __shared__ double lds[kPgBlock];
  const int k = blockIdx.x * kPgBlock + threadIdx.x;
  double den = 0.0, rot = 0.0, trans = 0.0;
  if (k < a.g.n) {
    Pose T, out;
#pragma unroll
    for (int q = 0; q < 9; ++q) T.R[q] = a.poses[(size_t)k * 12 + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) T.t[q] = a.poses[(size_t)k * 12 + 9 + q];
    out = T;
    if (!a.g.fixed[k]) {
      double d[6], b[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) d[i] = a.x[(size_t)k * 6 + i], b[i] = a.grad[(size_t)k * 6 + i];
      Pose delta;
      so3_exp_matrix(d, delta.R);
      delta.t[0] = d[3], delta.t[1] = d[4], delta.t[2] = d[5];
      pose_mul(delta, T, out);
#pragma unroll
      for (int i = 0; i < 6; ++i) den += d[i] * (a.lambda * d[i] - b[i]);
#pragma unroll
      for (int q = 0; q < 9; ++q) rot = fmax(rot, fabs(delta.R[q] - (q % 4 == 0 ? 1.0 : 0.0)));
#pragma unroll
      for (int q = 0; q < 3; ++q) trans = fmax(trans, fabs(delta.t[q]));
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) a.trial[(size_t)k * 12 + q] = out.R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) a.trial[(size_t)k * 12 + 9 + q] = out.t[q];
  }
  den = pg_block_sum(den, lds);
  rot = pg_block_max(rot, lds);
  trans = pg_block_max(trans, lds);
  if (threadIdx.x == 0) a.part_a[blockIdx.x] = den, a.part_b[blockIdx.x] = rot, a.part_c[blockIdx.x] = trans;
}

template <int>
__global__ void __launch_bounds__(kPgBlock) k_pg_try_reduce(PgScalars* sc, const double* part_a, const double* part_b, const double* part_c, int nb_n, const double* part_chi2,
                                                            int nb_e, int which) {
  __shared__ double lds[kPgBlock];
  const double den = pg_sum_partials(part_a, nb_n, lds);
  const double rot = pg_max_partials(part_b, nb_n, lds);
  const double trans = pg_max_partials(part_c, nb_n, lds);
  const double chi2 = pg_sum_partials(part_chi2, nb_e, lds);
  if (threadIdx.x == 0) {
    sc->den = den;
    sc->rot_max = rot;
    sc->trans_max = trans;
    sc->chi2[which] = chi2;
  }
}

template <int>
__global__ void __launch_bounds__(kPgBlock) k_pg_multiply(PgGraphDev g, const double* __restrict__ lin, const double* __restrict__ x, double lambda, double* __restrict__ y) {
  const int k = blockIdx.x * kPgBlock + threadIdx.x;
  if (k >= g.n) return;
  double out[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (!g.fixed[k]) pg_node_matvec<true>(g, lin, x, lambda, k, out);
#pragma unroll
  for (int i = 0; i < 6; ++i) y[(size_t)k * 6 + i] = out[i];
}

// C = T_new T_old^-1: T_old^-1 = (R^T, -(R^T t)), then pose_mul; rounded to float, column-major
template <int>
__global__ void __launch_bounds__(kPgBlock) k_pg_corrections(const double* __restrict__ T_new, const double* __restrict__ T_old, int n, float* __restrict__ C) {
  const int k = blockIdx.x * kPgBlock + threadIdx.x;
  if (k >= n) return;
  Pose a, inv, c;
  const double* o = T_old + (size_t)k * 12;
#pragma unroll
  for (int q = 0; q < 9; ++q) a.R[q] = T_new[(size_t)k * 12 + q];
#pragma unroll
  for (int q = 0; q < 3; ++q) a.t[q] = T_new[(size_t)k * 12 + 9 + q];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) inv.R[r * 3 + cc] = o[cc * 3 + r];
    inv.t[r] = -pose_mul_r(o[0 * 3 + r], o[1 * 3 + r], o[2 * 3 + r], o[9], o[10], o[11]);
  }
  pose_mul(a, inv, c);
  float* out = C + (size_t)k * 16;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) out[cc * 4 + r] = (float)c.R[r * 3 + cc];
    out[12 + r] = (float)c.t[r];
  }
  out[3] = out[7] = out[11] = 0.f;
  out[15] = 1.f;
}

}  // namespace ngk

// ---- the host side ----
namespace {

using namespace ngk;

constexpr int kPgLmMaxTries = 10;             // the inner tries of step_lm (Params::lm_max_iter's default)
constexpr double kPgInitLambdaFactor = 1e-9;  // Params::lm_init_lambda_factor's default
constexpr int kPgPeekEvery = 64;              // CG iterations between two glances at the pinned done word

void pg_colmajor_to_pose(const double* T, double* P) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) P[r * 3 + c] = T[c * 4 + r];
    P[9 + r] = T[12 + r];
  }
}
void pg_pose_to_colmajor(const double* P, double* T) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[c * 4 + r] = P[r * 3 + c];
    T[12 + r] = P[9 + r];
    T[r * 4 + 3] = 0.0;
  }
  T[3] = T[7] = T[11] = 0.0;
  T[15] = 1.0;
}

void pg_refuse(const char* entry, ngpg::Refusal r, size_t where) {
  if (r != ngpg::kOk) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": " + ngpg::refusal_text(r) + " (item " + std::to_string(where) + ")"};
}

int pg_blocks(size_t items) { return (int)std::max<size_t>(1, (items + kPgBlock - 1) / kPgBlock); }

// device images of the graph: edges, flags and lists when the topology changed, poses when the host's are newer
void pg_sync_device(ngicp* h) {
  ngicp::PoseGraph& g = h->pg;
  const size_t n = g.fixed.size(), m = g.ij.size() / 2;
  if (g.topo_dirty) {
    std::vector<int> off, ent;
    ngpg::build_csr(n, g.ij.data(), m, off, ent);
    g.d_ij.ensure(std::max<size_t>(1, m) * sizeof(int2));
    g.d_Z.ensure(std::max<size_t>(1, m) * 12 * sizeof(double));
    g.d_info.ensure(std::max<size_t>(1, m) * 36 * sizeof(double));
    g.d_eflag.ensure(std::max<size_t>(1, m));
    g.d_fixed.ensure(std::max<size_t>(1, n));
    g.d_off.ensure((n + 1) * sizeof(int));
    g.d_ent.ensure(std::max<size_t>(1, 2 * m) * sizeof(int));
    std::vector<double> Zp(m * 12);
    for (size_t e = 0; e < m; ++e) pg_colmajor_to_pose(g.Z.data() + e * 16, Zp.data() + e * 12);
    // (blocking copies: the staging vectors are this function's)
    if (m) {
      HIP_TRY(hipMemcpy(g.d_ij.p, g.ij.data(), m * sizeof(int2), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(g.d_Z.p, Zp.data(), m * 12 * sizeof(double), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(g.d_info.p, g.info.data(), m * 36 * sizeof(double), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(g.d_eflag.p, g.eflag.data(), m, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(g.d_ent.p, ent.data(), 2 * m * sizeof(int), hipMemcpyHostToDevice));
    }
    if (n) HIP_TRY(hipMemcpy(g.d_fixed.p, g.fixed.data(), n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g.d_off.p, off.data(), (n + 1) * sizeof(int), hipMemcpyHostToDevice));
    // per-node and per-edge workspaces
    const size_t nn = std::max<size_t>(1, n), mm = std::max<size_t>(1, m);
    for (DevBuf& b : g.d_lin) b.ensure(ngpg::edge_lin_bytes(mm));
    g.d_diag.ensure(nn * 36 * sizeof(double));
    g.d_minv.ensure(nn * 36 * sizeof(double));
    for (DevBuf* b : {&g.d_grad, &g.d_x, &g.d_r, &g.d_z, &g.d_p, &g.d_q}) b->ensure(nn * 6 * sizeof(double));
    g.d_part.ensure((size_t)(3 * pg_blocks(n) + pg_blocks(m)) * sizeof(double));
    g.d_sc.ensure(sizeof(PgScalars));
    for (DevBuf& b : g.d_poses) b.ensure(ngpg::pose_bytes(nn));
    g.topo_dirty = false;
    g.poses_dirty = true;
  }
  if (g.poses_dirty) {
    std::vector<double> P(n * 12);
    for (size_t k = 0; k < n; ++k) pg_colmajor_to_pose(g.poses.data() + k * 16, P.data() + k * 12);
    g.cur = 0;
    if (n) HIP_TRY(hipMemcpy(g.d_poses[0].p, P.data(), n * 12 * sizeof(double), hipMemcpyHostToDevice));
    g.poses_dirty = false;
  }
  if (!g.pin) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&g.pin), sizeof(PgScalars) + 64, hipHostMallocDefault));
  if (!g.ev_a) HIP_TRY(hipEventCreate(&g.ev_a));
  if (!g.ev_b) HIP_TRY(hipEventCreate(&g.ev_b));
}

PgGraphDev pg_dev(const ngicp* h) {
  const ngicp::PoseGraph& g = h->pg;
  PgGraphDev d;
  d.n = (int)g.fixed.size();
  d.m = (int)(g.ij.size() / 2);
  d.ij = g.d_ij.as<int2>();
  d.Z = g.d_Z.as<double>();
  d.info = g.d_info.as<double>();
  d.eflag = g.d_eflag.as<unsigned char>();
  d.fixed = g.d_fixed.as<unsigned char>();
  d.off = g.d_off.as<int>();
  d.ent = g.d_ent.as<int>();
  return d;
}

struct PgParts {
  double *a, *b, *c, *chi2;
  int nb_n, nb_e;
};
PgParts pg_parts(const ngicp* h) {
  const ngicp::PoseGraph& g = h->pg;
  PgParts p;
  p.nb_n = pg_blocks(g.fixed.size());
  p.nb_e = pg_blocks(g.ij.size() / 2);
  p.a = g.d_part.as<double>();
  p.b = p.a + p.nb_n;
  p.c = p.b + p.nb_n;
  p.chi2 = p.c + p.nb_n;
  return p;
}

void pg_launch_linearize(ngicp* h, const double* poses, int which) {
  ngicp::PoseGraph& g = h->pg;
  const PgParts pt = pg_parts(h);
  PgLinArgs a;
  a.g = pg_dev(h);
  a.poses = poses;
  a.lin = g.d_lin[which].as<double>();
  a.part_chi2 = pt.chi2;
  a.kind = g.robust_kind;
  a.c = g.robust_width;
  a.c2 = g.robust_width * g.robust_width;
  hipLaunchKernelGGL(k_pg_linearize<0>, dim3((unsigned)pt.nb_e), dim3(kPgBlock), 0, h->stream, a);
}
void pg_launch_assemble(ngicp* h, int which, bool want_max) {
  ngicp::PoseGraph& g = h->pg;
  const PgParts pt = pg_parts(h);
  hipLaunchKernelGGL(k_pg_assemble<0>, dim3((unsigned)pt.nb_n), dim3(kPgBlock), 0, h->stream, pg_dev(h), (const double*)g.d_lin[which].as<double>(), g.d_diag.as<double>(),
                     g.d_grad.as<double>(), pt.a);
  if (want_max)
    hipLaunchKernelGGL(k_pg_lin_reduce<0>, dim3(1), dim3(kPgBlock), 0, h->stream, g.d_sc.as<PgScalars>(), (const double*)pt.chi2, pt.nb_e, which, (const double*)pt.a, pt.nb_n);
}
PgScalars pg_read_scalars(ngicp* h) {
  ngicp::PoseGraph& g = h->pg;
  HIP_TRY(hipMemcpyAsync(g.pin + 64, g.d_sc.p, sizeof(PgScalars), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  PgScalars s;
  std::memcpy(&s, g.pin + 64, sizeof(s));
  return s;
}
void pg_download_poses(ngicp* h) {
  ngicp::PoseGraph& g = h->pg;
  const size_t n = g.fixed.size();
  std::vector<double> P(n * 12);
  if (n) HIP_TRY(hipMemcpy(P.data(), g.d_poses[g.cur].p, n * 12 * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < n; ++k) pg_pose_to_colmajor(P.data() + k * 12, g.poses.data() + k * 16);
}

void pg_check_range(const ngicp* h, const char* entry, int first, size_t n, const void* arr) {
  const size_t have = h->pg.fixed.size();
  if (!arr || n == 0) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": a null array or n == 0"};
  if (first < 0 || (size_t)first > have || n > have - (size_t)first) throw ArgError{NGICP_ERR_ARG, std::string(entry) + ": node ids outside the graph"};
}

}  // namespace

extern "C" {

int ngicp_pose_graph_clear(ngicp_t* h) {
  return guarded(h, [&] {
    ngicp::PoseGraph& g = h->pg;
    HIP_TRY(hipStreamSynchronize(h->stream));
    g.poses.clear(), g.fixed.clear(), g.ij.clear(), g.Z.clear(), g.info.clear(), g.eflag.clear(), g.snapshot.clear();
    g.topo_dirty = g.poses_dirty = true;
  });
}

int ngicp_pose_graph_size(const ngicp_t* h, size_t* nodes, size_t* edges) {
  if (!h) return NGICP_ERR_ARG;
  if (nodes) *nodes = h->pg.fixed.size();
  if (edges) *edges = h->pg.ij.size() / 2;
  return NGICP_OK;
}

int ngicp_pose_graph_add_nodes(ngicp_t* h, const double* T_colmajor_n16, const unsigned char* fixed, size_t n, int* first_id_out) {
  return guarded(h, [&] {
    ngicp::PoseGraph& g = h->pg;
    size_t bad = 0;
    pg_refuse("ngicp_pose_graph_add_nodes", ngpg::check_add_nodes(g.fixed.size(), T_colmajor_n16, n, &bad), bad);
    if (first_id_out) *first_id_out = (int)g.fixed.size();
    g.poses.insert(g.poses.end(), T_colmajor_n16, T_colmajor_n16 + n * 16);
    for (size_t k = 0; k < n; ++k) g.fixed.push_back(fixed && fixed[k] ? 1 : 0);
    g.topo_dirty = true;
  });
}

int ngicp_pose_graph_add_edges(ngicp_t* h, const int* ij_n2, const double* Z_colmajor_n16, const double* info_n36, const unsigned char* robust_flags, size_t n,
                               int* first_edge_out) {
  return guarded(h, [&] {
    ngicp::PoseGraph& g = h->pg;
    size_t bad = 0;
    pg_refuse("ngicp_pose_graph_add_edges", ngpg::check_add_edges(g.fixed.size(), g.ij.size() / 2, ij_n2, Z_colmajor_n16, info_n36, n, &bad), bad);
    if (first_edge_out) *first_edge_out = (int)(g.ij.size() / 2);
    g.ij.insert(g.ij.end(), ij_n2, ij_n2 + 2 * n);
    g.Z.insert(g.Z.end(), Z_colmajor_n16, Z_colmajor_n16 + n * 16);
    g.info.insert(g.info.end(), info_n36, info_n36 + n * 36);
    for (size_t e = 0; e < n; ++e) g.eflag.push_back(robust_flags && robust_flags[e] ? 1 : 0);
    g.topo_dirty = true;
  });
}

int ngicp_pose_graph_get_edges(ngicp_t* h, int first, size_t n, int* ij_n2, double* Z_colmajor_n16, double* info_n36, unsigned char* robust_flags) {
  return guarded(h, [&] {
    const ngicp::PoseGraph& g = h->pg;
    const size_t m = g.ij.size() / 2;
    if (n == 0 || first < 0 || (size_t)first > m || n > m - (size_t)first) throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_get_edges: edge ids outside the graph, or n == 0"};
    const size_t f = (size_t)first;
    if (ij_n2) std::memcpy(ij_n2, g.ij.data() + 2 * f, 2 * n * sizeof(int));
    if (Z_colmajor_n16) std::memcpy(Z_colmajor_n16, g.Z.data() + 16 * f, 16 * n * sizeof(double));
    if (info_n36) std::memcpy(info_n36, g.info.data() + 36 * f, 36 * n * sizeof(double));
    if (robust_flags) std::memcpy(robust_flags, g.eflag.data() + f, n);
  });
}

int ngicp_pose_graph_set_fixed(ngicp_t* h, const int* ids, const unsigned char* flags, size_t n) {
  return guarded(h, [&] {
    ngicp::PoseGraph& g = h->pg;
    if (!ids || !flags || n == 0) throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_set_fixed: a null array or n == 0"};
    for (size_t k = 0; k < n; ++k)
      if (ids[k] < 0 || (size_t)ids[k] >= g.fixed.size()) throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_set_fixed: unknown node id " + std::to_string(ids[k])};
    for (size_t k = 0; k < n; ++k) g.fixed[(size_t)ids[k]] = flags[k] ? 1 : 0;
    g.topo_dirty = true;
  });
}

int ngicp_pose_graph_get_fixed(ngicp_t* h, int first, size_t n, unsigned char* flags_out) {
  return guarded(h, [&] {
    pg_check_range(h, "ngicp_pose_graph_get_fixed", first, n, flags_out);
    std::memcpy(flags_out, h->pg.fixed.data() + first, n);
  });
}

int ngicp_pose_graph_set_robust(ngicp_t* h, int kind, double width) {
  return guarded(h, [&] {
    if (kind < NGICP_ROBUST_NONE || kind > NGICP_ROBUST_GEMAN_MCCLURE) throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_set_robust: unknown kernel"};
    if (!(width > 0.0) || !std::isfinite(width)) throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_set_robust: the width must be positive and finite"};
    h->pg.robust_kind = kind;
    h->pg.robust_width = width;
  });
}

int ngicp_pose_graph_get_poses(ngicp_t* h, int first, size_t n, double* T_colmajor_n16) {
  return guarded(h, [&] {
    pg_check_range(h, "ngicp_pose_graph_get_poses", first, n, T_colmajor_n16);
    std::memcpy(T_colmajor_n16, h->pg.poses.data() + (size_t)first * 16, n * 16 * sizeof(double));
  });
}

int ngicp_pose_graph_set_poses(ngicp_t* h, int first, size_t n, const double* T_colmajor_n16) {
  return guarded(h, [&] {
    pg_check_range(h, "ngicp_pose_graph_set_poses", first, n, T_colmajor_n16);
    for (size_t k = 0; k < n; ++k) pg_refuse("ngicp_pose_graph_set_poses", ngpg::check_pose16(T_colmajor_n16 + k * 16), k);
    std::memcpy(h->pg.poses.data() + (size_t)first * 16, T_colmajor_n16, n * 16 * sizeof(double));
    h->pg.poses_dirty = true;
  });
}

int ngicp_pose_graph_linearize(ngicp_t* h, double* chi2_out, double* edge_r_m6, double* edge_s_w_m2, double* grad_n6, double* diag_n36) {
  return guarded(h, [&] {
    ngicp::PoseGraph& g = h->pg;
    const size_t n = g.fixed.size(), m = g.ij.size() / 2;
    pg_sync_device(h);
    pg_launch_linearize(h, g.d_poses[g.cur].as<double>(), 0);
    pg_launch_assemble(h, 0, true);
    const PgScalars s = pg_read_scalars(h);
    if (chi2_out) *chi2_out = s.chi2[0];
    if ((edge_r_m6 || edge_s_w_m2) && m) {
      std::vector<double> lin(m * kPgLin);
      HIP_TRY(hipMemcpy(lin.data(), g.d_lin[0].p, lin.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (size_t e = 0; e < m; ++e) {
        if (edge_r_m6) std::memcpy(edge_r_m6 + e * 6, lin.data() + e * kPgLin + kPgR, 6 * sizeof(double));
        if (edge_s_w_m2) edge_s_w_m2[2 * e] = lin[e * kPgLin + kPgS], edge_s_w_m2[2 * e + 1] = lin[e * kPgLin + kPgW];
      }
    }
    if (grad_n6 && n) HIP_TRY(hipMemcpy(grad_n6, g.d_grad.p, n * 6 * sizeof(double), hipMemcpyDeviceToHost));
    if (diag_n36 && n) HIP_TRY(hipMemcpy(diag_n36, g.d_diag.p, n * 36 * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int ngicp_pose_graph_multiply(ngicp_t* h, double lambda, const double* x_n6, double* y_n6) {
  return guarded(h, [&] {
    ngicp::PoseGraph& g = h->pg;
    const size_t n = g.fixed.size();
    if (!x_n6 || !y_n6 || n == 0) throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_multiply: a null array or an empty graph"};
    if (!std::isfinite(lambda)) throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_multiply: lambda is not finite"};
    pg_sync_device(h);
    pg_launch_linearize(h, g.d_poses[g.cur].as<double>(), 0);
    HIP_TRY(hipMemcpyAsync(g.d_x.p, x_n6, n * 6 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_pg_multiply<0>, dim3((unsigned)pg_blocks(n)), dim3(kPgBlock), 0, h->stream, pg_dev(h), (const double*)g.d_lin[0].as<double>(),
                       (const double*)g.d_x.as<double>(), lambda, g.d_q.as<double>());
    HIP_TRY(hipMemcpyAsync(y_n6, g.d_q.p, n * 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
  });
}

int ngicp_pose_graph_optimize(ngicp_t* h, const ngicp_pg_options* opt_in, ngicp_pg_result* res) {
  return guarded(h, [&] {
    ngicp::PoseGraph& g = h->pg;
    if (!res) throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_optimize: null result"};
    ngicp_pg_options o = {64, 2e-3, 5e-4, 1e-8, 1000};
    if (opt_in) o = *opt_in;
    if (o.max_iterations < 0 || o.cg_max_iterations < 1 || !(o.rot_eps > 0.0) || !(o.trans_eps > 0.0) || !(o.cg_tol >= 0.0) || !std::isfinite(o.cg_tol))
      throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_optimize: options out of range"};
    const size_t n = g.fixed.size(), m = g.ij.size() / 2;
    const size_t loose = ngpg::ungauged_components(n, g.ij.data(), m, g.fixed.data());
    if (loose) throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_optimize: " + std::to_string(loose) + " connected component(s) hold no fixed node; nothing was changed"};
    std::memset(res, 0, sizeof(*res));
    g.snapshot = g.poses;
    g.kernel_ms = 0.0;
    size_t n_free = 0;
    for (unsigned char f : g.fixed) n_free += f ? 0 : 1;
    if (m == 0 || n_free == 0) {  // nothing to move
      res->converged = 1;
      if (m == 0) return;
    }
    pg_sync_device(h);
    const PgParts pt = pg_parts(h);
    PgScalars* sc = g.d_sc.as<PgScalars>();
    int* host_done = reinterpret_cast<int*>(g.pin);
    HIP_TRY(hipEventRecord(g.ev_a, h->stream));
    int lin = 0;  // the linearisation buffer of the current poses
    pg_launch_linearize(h, g.d_poses[g.cur].as<double>(), lin);
    pg_launch_assemble(h, lin, true);
    PgScalars s = pg_read_scalars(h);
    double chi2 = s.chi2[lin];
    res->initial_chi2 = res->final_chi2 = chi2;
    double lambda = kPgInitLambdaFactor * s.maxdiag;
    bool done = n_free == 0;
    while (!done && res->iterations < o.max_iterations) {
      double nu = 2.0;
      res->iterations += 1;
      for (int trial = 0; trial < kPgLmMaxTries; ++trial) {
        PgCgArgs a;
        a.g = pg_dev(h);
        a.lin = g.d_lin[lin].as<double>();
        a.diag = g.d_diag.as<double>();
        a.grad = g.d_grad.as<double>();
        a.minv = g.d_minv.as<double>();
        a.x = g.d_x.as<double>(), a.r = g.d_r.as<double>(), a.z = g.d_z.as<double>(), a.p = g.d_p.as<double>(), a.q = g.d_q.as<double>();
        a.part_a = pt.a, a.part_b = pt.b, a.part_c = pt.c;
        a.sc = sc;
        a.host_done = host_done;
        a.lambda = lambda;
        a.tol2 = o.cg_tol * o.cg_tol;
        a.nb = pt.nb_n;
        a.k = 0;
        *host_done = 0;  // (the stream is idle: every try ends in a synchronising read-back)
        const dim3 grid((unsigned)pt.nb_n), block(kPgBlock);
        hipLaunchKernelGGL(k_pg_precond<0>, grid, block, 0, h->stream, a);
        hipLaunchKernelGGL(k_pg_cg_start<0>, dim3(1), block, 0, h->stream, a);
        for (int k = 0; k < o.cg_max_iterations; ++k) {
          if (k % kPgPeekEvery == 0 && __atomic_load_n(host_done, __ATOMIC_RELAXED)) break;
          a.k = k;
          hipLaunchKernelGGL(k_pg_cg_matvec<0>, grid, block, 0, h->stream, a);
          hipLaunchKernelGGL(k_pg_cg_step<0>, grid, block, 0, h->stream, a);
          hipLaunchKernelGGL(k_pg_cg_dir<0>, grid, block, 0, h->stream, a);
        }
        PgUpdateArgs u;
        u.g = a.g;
        u.poses = g.d_poses[g.cur].as<double>();
        u.trial = g.d_poses[g.cur ^ 1].as<double>();
        u.x = a.x;
        u.grad = a.grad;
        u.part_a = pt.a, u.part_b = pt.b, u.part_c = pt.c;
        u.lambda = lambda;
        hipLaunchKernelGGL(k_pg_update<0>, grid, block, 0, h->stream, u);
        pg_launch_linearize(h, u.trial, lin ^ 1);
        hipLaunchKernelGGL(k_pg_try_reduce<0>, dim3(1), block, 0, h->stream, sc, (const double*)pt.a, (const double*)pt.b, (const double*)pt.c, pt.nb_n, (const double*)pt.chi2,
                           pt.nb_e, lin ^ 1);
        s = pg_read_scalars(h);  // the try's one read-back
        const double chi2_t = s.chi2[lin ^ 1];
        const double rho = (chi2 - chi2_t) / s.den;
        const bool small = std::max(s.rot_max / o.rot_eps, s.trans_max / o.trans_eps) < 1;
        const bool rejected = rho < 0;  // NaN is accepted, as in the aligner
        res->cg_iterations += s.iters;
        if (res->n_trace < NGICP_PG_TRACE_CAP) {
          double* row = res->trace + (size_t)res->n_trace * ngpg::kTraceCols;
          row[0] = chi2_t, row[1] = lambda, row[2] = rho, row[3] = (double)s.iters, row[4] = rejected ? 0.0 : 1.0;
          res->n_trace += 1;
        }
        if (rejected) {
          if (small) {
            res->converged = 1;
            done = true;
            break;
          }
          lambda = nu * lambda;
          nu = 2 * nu;
          if (trial + 1 >= kPgLmMaxTries) done = true;
          continue;
        }
        g.cur ^= 1;
        lin ^= 1;
        chi2 = chi2_t;
        res->accepted += 1;
        res->final_chi2 = chi2;
        {
          const double q3 = 2 * rho - 1;  // lm_lambda_accepted's expression (ngicp_lm.h)
          lambda = lambda * std::fmax(1.0 / 3.0, 1 - q3 * q3 * q3);
        }
        if (small) {
          res->converged = 1;
          done = true;
        } else {
          pg_launch_assemble(h, lin, false);
        }
        break;
      }
    }
    HIP_TRY(hipEventRecord(g.ev_b, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g.ev_a, g.ev_b) == hipSuccess) g.kernel_ms = ms;
    pg_download_poses(h);
  });
}

int ngicp_pose_graph_corrections(ngicp_t* h, const int* ids, size_t n, const double* T_old_colmajor_n16, float* C_colmajor_n16) {
  return guarded(h, [&] {
    ngicp::PoseGraph& g = h->pg;
    if (!ids || !C_colmajor_n16 || n == 0) throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_corrections: a null array or n == 0"};
    const size_t have = g.fixed.size(), snap = g.snapshot.size() / 16;
    for (size_t k = 0; k < n; ++k) {
      if (ids[k] < 0 || (size_t)ids[k] >= have) throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_corrections: unknown node id " + std::to_string(ids[k])};
      if (!T_old_colmajor_n16 && (size_t)ids[k] >= snap)
        throw ArgError{NGICP_ERR_ARG, "ngicp_pose_graph_corrections: node " + std::to_string(ids[k]) + " has no snapshot (no optimize has run since it was added)"};
      if (T_old_colmajor_n16) pg_refuse("ngicp_pose_graph_corrections", ngpg::check_pose16(T_old_colmajor_n16 + k * 16), k);
    }
    std::vector<double> P(2 * n * 12);
    for (size_t k = 0; k < n; ++k) {
      pg_colmajor_to_pose(g.poses.data() + (size_t)ids[k] * 16, P.data() + k * 12);
      pg_colmajor_to_pose(T_old_colmajor_n16 ? T_old_colmajor_n16 + k * 16 : g.snapshot.data() + (size_t)ids[k] * 16, P.data() + (n + k) * 12);
    }
    g.d_corr.ensure(P.size() * sizeof(double) + n * 16 * sizeof(float));
    double* dP = g.d_corr.as<double>();
    float* dC = reinterpret_cast<float*>(dP + 2 * n * 12);
    HIP_TRY(hipMemcpyAsync(dP, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_pg_corrections<0>, dim3((unsigned)pg_blocks(n)), dim3(kPgBlock), 0, h->stream, (const double*)dP, (const double*)(dP + n * 12), (int)n, dC);
    HIP_TRY(hipMemcpyAsync(C_colmajor_n16, dC, n * 16 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
  });
}

int ngicp_pose_graph_kernel_ms(const ngicp_t* h, double* ms) {
  if (!h || !ms) return NGICP_ERR_ARG;
  *ms = h->pg.kernel_ms;
  return NGICP_OK;
}

}  // extern "C"
