// Several alignments of ONE source / target pair in the same launches (ngicp_align_batch, ngicp_fitness_score_batch).
//
// A LANE is one alignment: its own optimiser state, correspondences, Mahalanobis matrices, partial rows, launch order and trace; the
// source, the target, both indices, both covariance sets and every parameter are shared.  The launches carry a lane dimension:
//   k_gicp_pass_batch<2, WPS>   grid (groups, live lanes).  A block finds its lane's PassArgs record in device memory and runs that
//                               group from a pointer to the record, the way k_gicp_queue runs a group from a pointer to its arguments
//                               - but inlined, so the search keeps its registers (no call, no scratch).  The body is the one
//                               k_gicp_pass includes (ngicp_pass_group.inc): same search, same tail, same [group][32] row.
//   k_lm_solve_batch            grid (live lanes): block l runs lm_solve_body<512, false> - k_lm_solve's body - on its lane's SolveArgs
//                               record: own rows, state, trace, launch order, and own {progress word, final image} in pinned memory
//                               (the image is stored before the word, and the device state before both: lm_solve_body).
//   k_fitness / k_fitness_final (ngicp_query.h)   the fitness kernels have a lane dimension of their own (grid row = transform): B
//                               transforms are one launch of the kernels that ngicp_fitness_score launches with one row.
// Which lanes a launch serves travels in its kernel arguments (BatchLaunch::lane): the host drops a lane from the list when it sees
// that lane's done flag, without a copy; the launches already enqueued return at the head of the lane's blocks, as stale launches of
// the single path do.
#pragma once
#include "ngicp_pass.h"
#include "ngicp_query.h"

namespace ngk {

constexpr int kBatchMaxLanes = 64;  // == NGICP_BATCH_MAX_LANES (include/ngicp.h)

struct BatchLaunch {
  const void* pass;        // [lanes of the batch] in device memory: PassArgs records (k_gicp_pass_batch) or VoxelPassArgs records
                           // (k_vgicp_pass_batch, ngicp_voxel_batch.h)
  const SolveArgs* solve;  // likewise
  int lane[kBatchMaxLanes];  // blockIdx.y (pass) / blockIdx.x (solver) -> lane of the batch
};
typedef const BatchLaunch __attribute__((address_space(4))) KernelBatchLaunch;

// One group of one pass of one lane: the prologue of persist_group_body<.., RING = false> (arguments through the constant address space,
// the pose from the state itself, rows stored plainly: the solver is a launch of its own) with k_gicp_pass's scalar wave number, then the
// body every pass kernel includes.  Inlined into the kernel: no call, the search keeps its registers.  (The pose is read here and not
// with load_pose, ngicp_lm.h: with it k_gicp_pass_batch's code came out different, six instructions shorter, and the exact route's
// code objects are kept as they are.)
#define NG_STAMP(k) \
  do {              \
  } while (0)  // (the batch path records no stamps)
template <int G, int WPS>
__device__ __forceinline__ void batch_group_body(KernelPassArgs& a, const int group, WaveStage* stage_all, double (*lds)[kNumSlots]) {
  constexpr bool FUSED = false;
  constexpr int B = 64 / G;
  constexpr int kWin = WPS >= 4 ? 12 : 16, kSideStep = WPS >= 4 ? 8 : 16;  // (see k_gicp_pass)
  static_assert(kWin <= kSortedPad && B == kBatchQueries, "see k_gicp_pass");
  const bool do_lin = (a.mode & 2);
  Grid g;  // (field by field: a reference to a generic Grid cannot bind to the constant address space)
  g.ox = a.grid.ox; g.oy = a.grid.oy; g.oz = a.grid.oz;
  g.h = a.grid.h; g.inv_h = a.grid.inv_h;
  g.nx = a.grid.nx; g.ny = a.grid.ny; g.nz = a.grid.nz;
  g.ncells = a.grid.ncells;
  g.slack = a.grid.slack;
  typedef const double __attribute__((address_space(4))) * ViewPtrD;
  typedef const float __attribute__((address_space(4))) * ViewPtrF;
  KernelStatePtr st4 = (KernelStatePtr)(unsigned long long)a.st;
  const int have_lin = st4->hot.have_lin;
  const int cur = st4->hot.cur & 1, nxt = cur ^ 1;
  ViewPtrD vx = (ViewPtrD)&st4->hot.xi;  // (Pose: R[9] then t[3])
  ViewPtrF vf = (ViewPtrF)st4->xi_f;
  double R[9], t[3];
  float Tf[12];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = vx[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = vx[9 + i];
#pragma unroll
  for (int i = 0; i < 12; ++i) Tf[i] = vf[i];
  const bool do_err = (a.mode & 1) && have_lin;
  const float4* __restrict__ tpt_old = a.tpt[cur];
  const double* __restrict__ mahal_old = a.mahal[cur];
  float4* __restrict__ tpt_new = a.tpt[nxt];
  double* __restrict__ mahal_new = a.mahal[nxt];
  double wave_total = 0.0;
  unsigned int ncand = 0, nvalid = 0, nstaged = 0;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int sub = lane % G, grp = lane / G;
  WaveStage& S = stage_all[wave];
  const unsigned long long t_start = a.grp_cost ? __builtin_amdgcn_s_memtime() : 0ull;
#define NG_HAVE_LIN have_lin
#include "ngicp_pass_group.inc"
#undef NG_HAVE_LIN
}
#undef NG_STAMP

template <int G, int WPS>
__global__ void __launch_bounds__(256, WPS) k_gicp_pass_batch(BatchLaunch bl) {
  __shared__ WaveStage stage[4];
  __shared__ double lds[4][kNumSlots];
  // The lane's record and, through it, what a block needs before it can fetch a point (done flag, order flag, its position's group):
  // scalar loads through the constant address space - neither the record nor the state changes while the launch runs.
  KernelBatchLaunch* kb = (KernelBatchLaunch*)__builtin_amdgcn_kernarg_segment_ptr();
  const int lane_id = kb->lane[blockIdx.y];
  KernelPassArgs* ka = (KernelPassArgs*)(unsigned long long)(reinterpret_cast<const PassArgs*>(kb->pass) + lane_id);
  typedef const int __attribute__((address_space(4))) * ConstIntPtr;
  const int done_now = ((KernelStatePtr)(unsigned long long)ka->st)->hot.done;
  const int order_is_valid = *(ConstIntPtr)(unsigned long long)ka->order_valid;
  const int order_entry = ((ConstIntPtr)(unsigned long long)ka->grp_order)[blockIdx.x];
  asm volatile("" ::"s"(done_now), "s"(order_is_valid), "s"(order_entry));  // (all three in flight before the first is looked at)
  if (done_now) return;
  const int group = order_is_valid ? order_entry : (int)blockIdx.x;
  batch_group_body<G, WPS>(*ka, group, stage, lds);
}

__global__ void __launch_bounds__(kSolveThreads) k_lm_solve_batch(BatchLaunch bl) {
  __shared__ SolveShared<kSolveThreads> sh;
  KernelBatchLaunch* kb = (KernelBatchLaunch*)__builtin_amdgcn_kernarg_segment_ptr();
  const int lane_id = kb->lane[blockIdx.x];
  // the lane's record, fetched as dwords through the constant address space: it ends up in scalar registers, as k_lm_solve's arguments do
  static_assert(sizeof(SolveArgs) % 4 == 0, "SolveArgs is copied as dwords");
  constexpr int kWords = (int)(sizeof(SolveArgs) / 4);
  typedef const int __attribute__((address_space(4))) * ConstIntPtr;
  ConstIntPtr src = (ConstIntPtr)(unsigned long long)(kb->solve + lane_id);
  int w[kWords];
#pragma unroll
  for (int i = 0; i < kWords; ++i) w[i] = src[i];
  SolveArgs a;
  __builtin_memcpy(&a, w, sizeof(a));
  lm_solve_body<kSolveThreads, false>(a, sh);
}

}  // namespace ngk
