// The per-iteration hot path: ONE fused kernel per Gauss-Newton/LM trial + one single-block solver.
//
//   k_gicp_pass   (data-parallel over source points, G lanes cooperate on one query)
//       K4  error of the trial pose under the PREVIOUS correspondences / Mahalanobis matrices
//           (NanoGICP::compute_error, /root/reference/include/nano_gicp/impl/nano_gicp_impl.hpp:273-296)
//       K2  float transform, exact 1-NN in the target grid, distance gate, Mahalanobis
//           (NanoGICP::update_correspondences, impl/nano_gicp_impl.hpp:174-211)
//       K3  residual, SE(3) Jacobian, H += J^T M J, b += J^T M e, y0 += e^T M e
//           (NanoGICP::linearize, impl/nano_gicp_impl.hpp:214-270)
//       R0  LDS transpose -> per-group partial sums (fixed order: deterministic, independent of launch order)
//   k_lm_solve    (one block)
//       final reduction of the block partials, then the Levenberg-Marquardt / Gauss-Newton state
//       machine of LsqRegistration (impl/lsq_registration_impl.hpp:89-208) on one lane: 6x6 LDLT,
//       so3_exp, gain ratio, lambda schedule, convergence test, next trial pose.
//
// Why K4 and K2+K3 are fused: the reference evaluates a trial pose xi with compute_error() and, when
// the trial is accepted (the common case), immediately re-linearises at x0 = xi.  Both passes stream
// the same source points, so one pass evaluates the trial's error under the old correspondences AND
// speculatively linearises at xi into the other half of a ping-pong buffer.  If the solver rejects the
// trial, the speculative half is simply overwritten by the next pass; the state visible to the LM
// logic is exactly the reference's (same y0, yi, rho, lambda sequence).  The host never reads back
// inside the loop: the solver publishes a `done` flag and later launches exit immediately.
//
// This header: the arguments of a pass (PassArgs), the default route's kernel (k_gicp_pass) and k_corr_to_original.  It includes the rest
// of the device side, so that including it is including all of it: the terms (ngicp_terms.h), the optimiser's state and step
// (ngicp_lm.h), the search (ngicp_search.h), the solver (ngicp_solve.h), the switch-only routes (ngicp_pass_routes.h) and the staged
// search (ngicp_pass_st.h).  Included by ngicp_api.hip, ngicp_batch.h and ngicp_voxel.h.
#pragma once
#include <type_traits>

#include "../../include/ngicp.h"
#include "ngicp_knn.h"
#include "ngicp_terms.h"
#include "ngicp_lm.h"
#include "ngicp_search.h"
#include "ngicp_solve.h"

namespace ngk {

struct PassArgs {
  const float4* qpts;       // source points in Morton-tile query order, w = sorted source position
  const int2* batches;      // tile-aligned query batches {first qpts index, count <= 32}
  const float* batch_boxes; // [n_batches][6] centre + half extents of each batch in the source frame
  const int* grp_order;     // [n_groups] launch order of the groups (a block takes group grp_order[blockIdx.x]); valid when st->order_valid
  int* grp_cost;            // [n_groups] measured duration of each group's block in the last pass (shader clocks >> 4), or null
  int n_batches;
  const double* cov_src;    // [n][6], source sorted order
  int n_src;
  const float4* tgt;        // sorted target points
  const float4* tgtp;       // the same points as {x, y, z, bitcast(sorted position)} (same sentinel frame): what k_gicp_pass_st copies to LDS
  const Xyz* tgt3;          // the same points packed 12 bytes each (same sentinel frame): what the walks and the tail fetch - a quarter
                            // fewer bytes per candidate and three registers per point instead of four
  const int* tgt_cell_start;
  const unsigned int* tgt_cell_box;  // per-cell (y,z) extents of the target's points (k_cell_boxes; framed like the cell-start table), or null
  const double* cov_tgt;    // [n_tgt][6], target sorted order
  Grid grid;                // target grid
  float4* tpt[2];           // [n_src] the correspondence of each query: {x, y, z of the target point, bitcast(sorted target position or -1)}:
                            // the next pass gets the warm start of its search and K4's target point in ONE load (no corr -> point chain)
  double* mahal[2];         // [n_src][6]
  double gate_sq;           // corr_dist_threshold_^2 (double, impl/nano_gicp_impl.hpp:195)
  float gate_sq_f;          // float upper bound of gate_sq for ring termination
  unsigned char* batch_far; // [n_batches] 1 if some query of the batch looked beyond its ring 1 in the previous pass: only then
                            // are the outer rings of the batch region listed (a wrong guess costs time, not exactness)
  LmState* st;
  double* partials;         // [n_groups][kNumSlots], group-major: a block stores its 32 sums as one 256-byte row
  int mode;                 // bit0: error part, bit1: linearise part, bit2: ignore st->done (test hooks), bit5: the first pass lists region rows,
                            // bit6: honour LmHot::lin_unneeded (k_gicp_pass: K4 alone where the linearisation can never be adopted)
  int stage_grow;           // rings around the batch box that the LDS row list covers (0: no list, search unindexed)
  unsigned long long* dbg_stamps;  // diagnostic only: [wave][kStampStride] s_memtime stamps + counters, or null
  int4* dbg_qstats;                // diagnostic only: per query {ring-1 candidates, ring-1 walks | far walks << 16, far + shell candidates, flags}, or null
  unsigned long long* dbg_span;    // diagnostic only: per block {s_memrealtime (10 ns ticks) at entry, at exit, HW_ID | XCC_ID << 32, group}, or null
  // fused solver: the block whose ticket is the last of the grid reduces the group rows and advances the optimiser in the tail of
  // the SAME launch (no second dispatch per iteration).  Rows and costs are then stored write-through and published by the ticket.
  const int* order_valid;          // device word: grp_order holds a complete order
  unsigned long long* t_first;     // device word: stamped by the first pass of an alignment (block 0), or null
  int fused;
  int* ticket;   // zero before the launch; the last block puts it back (persistent: counts on, pass after pass)
  // persistent: ONE launch per alignment.  A block keeps its groups for the whole alignment (their correspondences and Mahalanobis
  // matrices never leave its CU's L1 / its XCD's L2: no kernel boundary drops them), the blocks meet at the ticket after every pass,
  // the last one to arrive steps the optimiser and releases the next pass through `gen`.
  // k_gicp_head: no solver launch.  Every block of launch i steps the optimiser itself, at its head, with the sums of pass i - 1 (32 rows,
  // added up per subset of groups by the blocks that finished their subset last), then searches at the pose it has just computed.
  const double* crow_in;   // [32][kNumSlots] the subset rows of the previous pass (zero rows for subsets without groups)
  double* crow_out;        // [32][kNumSlots] this pass's
  int* cluster_ticket;     // [32] zero before the launch; the last block of a subset puts its word back
  int* done_flag;          // device word, zero at the start of an alignment: a launch's solver block sets it when the alignment is over
  int persist;
  int first_pass;  // (0 unless the kernel is launched once per pass for an A/B measurement: the ring entry the launch begins with)
  int max_passes;
  int* gen;      // zero before the launch: passes released so far (agent scope), kGenLines copies in cache lines of their own
  SolveArgs sa;
  // robust kernel (robust_term): read by the ROBUST instantiations of k_gicp_pass only, which the host launches exactly when kind != NONE
  int robust_kind;
  double robust_c, robust_c2;
};

constexpr int kStampStride = 24;
#define NG_STAMP(k)                                                                                   \
  do {                                                                                                \
    if (a.dbg_stamps && lane == 0) a.dbg_stamps[(size_t)(blockIdx.x * 4 + wave) * kStampStride + (k)] = __builtin_amdgcn_s_memtime(); \
  } while (0)

template <int G, int WPS = NGICP_PASS_WAVES, bool FUSED = false, bool ROBUST = false>
__global__ void __launch_bounds__(256, WPS) k_gicp_pass(PassArgs a) {
  constexpr int B = 64 / G;  // queries per wave batch
  // Walk windows (see scan_global_outward), measured with the packed points: the default build, whose launches are as long as their
  // slowest chain of window steps, does best with 16-point windows (c3 35.4 -> 34.3 us, c2 32.0 -> 31.2 us against 12; 18 and more
  // cost registers and time); the build for large grids, bound by what its waves fetch, with 12 points and 8-point side windows.
  constexpr int kWin = WPS >= 4 ? 12 : 16, kSideStep = WPS >= 4 ? 8 : 16;
  static_assert(kWin <= kSortedPad, "walk windows may overhang the array by at most the sentinel frame");
  static_assert(B == kBatchQueries, "query batches are built for 32 queries (2 lanes per query)");
  __shared__ double lds[4][kNumSlots];
  // (FUSED is a build of its own: the solver's reduction keeps 28 sixteen-byte loads in flight per thread, and with it in the kernel
  // the 4-waves-per-SIMD build spilled 35-38 registers instead of 2 - c5 41.6 -> 48.3 us per pass with the tail never even executed)
  struct Nothing {};
  union PassShared {
    WaveStage stage[4];
    typename std::conditional<FUSED, SolveShared<256>, Nothing>::type sv;  // the fused solver (the last block of the grid) works where the search tables were
  };
  __shared__ PassShared shm;
  __shared__ int last_block;
  WaveStage* stage_all = shm.stage;
  const LmState* __restrict__ st = a.st;
  // Everything a block needs before it can fetch a point - the done flag, the launch-order flag, its position's group - is requested in
  // ONE go, as scalar loads through the constant address space (none of it changes while the launch runs): the compiler had made six
  // dependent round trips of it (done -> have_lin -> cur -> pose -> order flag -> order entry, the last two as vector loads), ~4 us on
  // every block's path before its first point.
  typedef const int __attribute__((address_space(4))) * ConstIntPtr;
  const int done_now = st->hot.done, have_lin_now = st->hot.have_lin;
  const int cur = st->hot.cur, nxt = cur ^ 1;
  const int lin_unneeded_now = st->hot.lin_unneeded;
  const int order_is_valid = *(ConstIntPtr)(unsigned long long)a.order_valid;             // (both pointers are set for every launch: prepare_loop)
  const int order_entry = ((ConstIntPtr)(unsigned long long)a.grp_order)[blockIdx.x];    // (read whether valid or not: the buffer exists)
  // trial pose (FP64) and its float cast
  double R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = st->hot.xi.R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = st->hot.xi.t[i];
  float Tf[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) Tf[i] = st->xi_f[i];
  // (all of the above is in flight before the first of it is looked at)
  asm volatile("" ::"s"(done_now), "s"(have_lin_now), "s"(cur), "s"(lin_unneeded_now), "s"(order_is_valid), "s"(order_entry), "s"(Tf[0]), "s"(Tf[11]), "s"(R[0]), "s"(t[2]));
  if (!(a.mode & 4) && done_now) return;

  const bool do_err = (a.mode & 1) && have_lin_now;
  const bool do_lin = (a.mode & 2);
  const float4* __restrict__ tpt_old = a.tpt[cur];
  const double* __restrict__ mahal_old = a.mahal[cur];
  float4* __restrict__ tpt_new = a.tpt[nxt];
  double* __restrict__ mahal_new = a.mahal[nxt];
  const Grid& g = a.grid;

  double wave_total = 0.0;  // lane v (< 29) accumulates slot v of this wave over its batches
  unsigned int ncand = 0, nvalid = 0, nstaged = 0;

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (the wave's number in a scalar register: its batch record is then a scalar load)
  const int sub = lane % G, grp = lane / G;
  WaveStage& S = stage_all[wave];
  NG_STAMP(0);
  // A block owns one GROUP of four consecutive batches (one per wave); its partial sums are stored under the group's
  // index, so the result does not depend on the order in which groups are launched.  That order is the solver's business:
  // it sorts the groups by the duration measured in the previous pass, heaviest first (the grid is ~1.7 waves of blocks
  // deep, and the slowest groups take 2-3x the median: started late they would set the kernel's length).
  const int group = order_is_valid ? order_entry : (int)blockIdx.x;
  const unsigned long long t_start = a.grp_cost ? __builtin_amdgcn_s_memtime() : 0ull;
  if (a.dbg_span && threadIdx.x == 0) a.dbg_span[(size_t)blockIdx.x * 4] = __builtin_amdgcn_s_memrealtime();  // (the 100 MHz counter: the same on every CU)
  if (a.t_first && blockIdx.x == 0 && threadIdx.x == 0 && !have_lin_now) *a.t_first = __builtin_amdgcn_s_memrealtime();
  if ((a.mode & 64) && lin_unneeded_now) {  // block-uniform
    // ---- K4 ALONE: the linearisation at this pose can never be adopted (set_lin_unneeded), so the solver reads slot 28 and nothing
    //      else.  A path of its own, taken before the search's state exists: the working pass pays one scalar load and this branch
    //      (folded into the group body's do_lin, the word stayed alive through the search and cost the SGPR-bound kernel 0.5 us per
    //      pass in spilled scalars).  tpt_new, mahal_new, batch_far and the group's cost stay as the last searching pass left them; the
    //      row is what the group body stores with do_lin off, bit for bit: K4's term as there, lanes 0..31 added in lane order
    //      starting from 0.0, the four waves as ((w0 + w1) + w2) + w3, every other slot +0.0. ----
    const int item = group * 4 + wave;
    double term = 0.0;  // the tail's acc[28] of this lane's query
    if (item < a.n_batches) {
      typedef const int __attribute__((address_space(4))) * ConstBatchPtr;
      ConstBatchPtr brec = (ConstBatchPtr)(unsigned long long)a.batches + 2 * (size_t)item;
      const int qbase = brec[0], qcount = brec[1];
      if (lane < qcount) {
        const int i = qbase + lane;
        const float4 sp = a.qpts[i];
        float4 bp_old = make_float4(0.f, 0.f, 0.f, 0.f);
        int j_old = -1;
        double Mold[6] = {0, 0, 0, 0, 0, 0};
        if (have_lin_now) {
          bp_old = tpt_old[i];
          j_old = __float_as_int(bp_old.w);
        }
        if (do_err) {
          const double* M = mahal_old + (size_t)i * 6;
#pragma unroll
          for (int e = 0; e < 6; ++e) Mold[e] = M[e];
        }
        double k4 = 0.0;
        if (do_err && j_old >= 0) {  // impl/nano_gicp_impl.hpp:273-296
          const double ax = (double)sp.x, ay = (double)sp.y, az = (double)sp.z;
          const double tax = R[0] * ax + R[1] * ay + R[2] * az + t[0];
          const double tay = R[3] * ax + R[4] * ay + R[5] * az + t[1];
          const double taz = R[6] * ax + R[7] * ay + R[8] * az + t[2];
          const double ex = (double)bp_old.x - tax, ey = (double)bp_old.y - tay, ez = (double)bp_old.z - taz;
          if constexpr (ROBUST) k4 = err_term_robust(a.robust_kind, a.robust_c, a.robust_c2, ex, ey, ez, Mold);
          else k4 = err_term(ex, ey, ez, Mold);
        }
        term += k4;
      }
    }
    double* red = S.red;
    if (lane < 32) red[lane] = term;
    wave_lds_sync();
    if (lane < kNumSlots) {
      double out = 0.0;
      if (lane == 28)
        for (int l = 0; l < 32; ++l) out += red[l];
      wave_total += out;
      lds[wave][lane] = lane == 28 ? wave_total : 0.0;
    }
    __syncthreads();
    if (threadIdx.x < kNumSlots) {
      const int v = threadIdx.x;
      const double val = ((lds[0][v] + lds[1][v]) + lds[2][v]) + lds[3][v];
      if (FUSED) __hip_atomic_store(a.partials + (size_t)group * kNumSlots + v, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else a.partials[(size_t)group * kNumSlots + v] = val;
    }
    if (a.dbg_span && threadIdx.x == 0) {
      unsigned long long* d = a.dbg_span + (size_t)blockIdx.x * 4;
      d[1] = __builtin_amdgcn_s_memrealtime();
      d[3] = (unsigned long long)(unsigned int)group;
    }
    if constexpr (!FUSED) return;  // (no join with the working path: nothing of this one is alive in it)
  } else {
#define NG_HAVE_LIN have_lin_now
#define NG_ROBUST ROBUST
#include "ngicp_pass_group.inc"
#undef NG_ROBUST
#undef NG_HAVE_LIN
  }
  if constexpr (FUSED) {
  // ---- the solver in the tail of the launch (R0's final sum, impl/nano_gicp_impl.hpp:260-267, and LsqRegistration's step,
  //      impl/lsq_registration_impl.hpp:161-208).  Every store of this block that another block will read was made by wave 0 as a
  //      write-through store; wave 0 drains them, then ONE lane takes a ticket (relaxed, agent scope).  The block that draws the
  //      last ticket of the grid knows that every other block's rows are in memory: one agent-scope acquire (drops this CU's L1;
  //      no other block pays anything), then it reads the rows with agent-scope loads, reduces them in the fixed group order and
  //      advances the optimiser exactly as k_lm_solve does.  (Round 2's version released with a fence per block: an agent-scope
  //      release writes the XCD's whole dirty L2 back - the pass's own 6 MB of outputs, once per block: 36 -> 143 us.) ----
  if (wave == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
      const int tk = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last_block = (tk == (int)gridDim.x - 1) ? 1 : 0;
    }
  }
  __syncthreads();
  if (!last_block) return;
  if (threadIdx.x == 0) {
    __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (for the next launch: ordered by the kernel boundary)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  lm_solve_body<256, true>(a.sa, shm.sv);
  }
}

#include "ngicp_pass_routes.h"
#undef NG_STAMP

}  // namespace ngk
#include "ngicp_pass_st.h"
namespace ngk {

// map correspondences (sorted source slot -> sorted target position) back to ORIGINAL indices
__global__ void __launch_bounds__(256) k_corr_to_original(const float4* __restrict__ tpt, const float4* __restrict__ qpts, const float4* __restrict__ src_sorted,
                                                           const float4* __restrict__ tgt_sorted, int n, int* __restrict__ out_corr, float* __restrict__ out_sqd,
                                                           const float* __restrict__ lin_f) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 sp = qpts[i];
  const int o = __float_as_int(src_sorted[__float_as_int(sp.w)].w);
  const int j = __float_as_int(tpt[i].w);
  out_corr[o] = j >= 0 ? __float_as_int(tgt_sorted[j].w) : -1;
  if (out_sqd) {
    float d = __builtin_inff();
    if (j >= 0) {
      const float3 q = transform_point_rowmajor_f(lin_f, sp.x, sp.y, sp.z);
      d = sqdist(q.x, q.y, q.z, tgt_sorted[j]);
    }
    out_sqd[o] = d;
  }
}

}  // namespace ngk
