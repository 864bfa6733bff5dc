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
//   k_fitness_batch / k_fitness_final_batch   k_fitness with a lane dimension: B transforms, one launch, per lane the same per-point
//                               work and the same fixed FP64 order of sums.
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
// body every pass kernel includes.  Inlined into the kernel: no call, the search keeps its registers.
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
  typedef const LmState __attribute__((address_space(4))) * StatePtr;
  StatePtr st4 = (StatePtr)(unsigned long long)a.st;
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
  typedef const LmState __attribute__((address_space(4))) * StatePtr;
  const int done_now = ((StatePtr)(unsigned long long)ka->st)->hot.done;
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

// k_fitness for transform blockIdx.y of T_colmajor[B][16]: partials[blockIdx.y * gridDim.x + blockIdx.x] = {sum of the counted d2, count}.
// (the same statements as k_fitness, ngicp_query.h: per lane of the batch the sums come out bit for bit as ngicp_fitness_score's)
__global__ void __launch_bounds__(kKnnBlock) k_fitness_batch(const float4* __restrict__ src_sorted, int n, const float* __restrict__ T_colmajor,
                                                             const float4* __restrict__ tgt_sorted, const int* __restrict__ tgt_cells, Grid g, double max_range,
                                                             double2* __restrict__ partials) {
  __shared__ int lds_bounds[36 * kKnnPairs];
  __shared__ double2 wave_part[kKnnBlock / 64];
  const float* __restrict__ Tm = T_colmajor + (size_t)blockIdx.y * 16;
  const int lane = threadIdx.x & 63, sub = threadIdx.x & 1, pair = threadIdx.x >> 1;
  const int i = blockIdx.x * kKnnPairs + pair;
  double s = 0.0, c = 0.0;
  if (i < n) {
    const float4 p = src_sorted[i];
    const float3 t = transform_point_f(Tm, p.x, p.y, p.z);
    PairTopK<2> top;
    knn_search<2, 4>(g, tgt_sorted, tgt_cells, t.x, t.y, t.z, -1, 1, top, lds_bounds + pair, sub, lane);
    const float d2 = top.part.template d<0>();  // slot 0 lives in lane 0 of the pair
    if (sub == 0 && (double)d2 <= max_range) {
      s = (double)d2;
      c = 1.0;
    }
  }
  s = wave_sum(s);
  c = wave_sum(c);
  if (lane == 0) wave_part[threadIdx.x >> 6] = make_double2(s, c);
  __syncthreads();
  if (threadIdx.x == 0) {
    double2 r = wave_part[0];
#pragma unroll
    for (int w = 1; w < kKnnBlock / 64; ++w) {
      r.x += wave_part[w].x;
      r.y += wave_part[w].y;
    }
    partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = r;
  }
}

// block l: out[l] = the sum of partials[l * nb .. l * nb + nb), in k_fitness_final's order
__global__ void __launch_bounds__(kFitnessFinalBlock) k_fitness_final_batch(const double2* __restrict__ partials, int nb, double2* __restrict__ out) {
  __shared__ double2 wave_part[kFitnessFinalBlock / 64];
  const double2* __restrict__ mine = partials + (size_t)blockIdx.x * nb;
  double s = 0.0, c = 0.0;
  for (int b = threadIdx.x; b < nb; b += kFitnessFinalBlock) {
    s += mine[b].x;
    c += mine[b].y;
  }
  s = wave_sum(s);
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = make_double2(s, c);
  __syncthreads();
  if (threadIdx.x == 0) {
    double2 r = wave_part[0];
#pragma unroll
    for (int w = 1; w < kFitnessFinalBlock / 64; ++w) {
      r.x += wave_part[w].x;
      r.y += wave_part[w].y;
    }
    out[blockIdx.x] = r;
  }
}

}  // namespace ngk
