// The solver: the fixed-order reduction of a pass's group rows, the launch order of the next pass, the pose prior's row, one step of
// the optimiser (ngicp_lm.h) and the publication of the advanced state - lm_solve_body, with its block-shared scratch.  The sort of the
// launch order is a function of its own (build_launch_order); the prior's row and the store-back stay in the body: lifted out, each
// changed the code of six kernels.
// k_lm_solve is the launch of its own; the fused tail of k_gicp_pass (ngicp_pass.h) and the head and persistent kernels
// (ngicp_pass_routes.h) call the same body.  k_step_selftest runs one step in both forms (ngicp_step_selftest).
#pragma once
#include "ngicp_lm.h"

namespace ngk {

// --- the solver ----------------------------------------------------------------------------------
constexpr int kSolveSubs = kSolveThreads / 16;  // sub-sums per slot pair (thread = 16 slot pairs x 32 group subsets)
#ifndef NGICP_SOLVE_CHUNK
#define NGICP_SOLVE_CHUNK 40
#endif
constexpr int kSolveChunk = NGICP_SOLVE_CHUNK;                  // 16-byte loads a thread keeps in flight per step: one step covers 32 x 40 = 1280 groups


// The solver's block-shared scratch.  k_lm_solve owns one; the fused tail of k_gicp_pass lays it over the (then idle) search tables.
template <int THREADS>
struct SolveShared {
  double wsum[32][kPartialStride];
  double sums[kPartialStride];
  int ord_cnt[THREADS / 64 - 1][16], ord_pos[THREADS / 64 - 1][16];  // per sorting wave and cost class
  int ord_cost[kMaxOrderGroups];
  unsigned char ord_cls[kMaxOrderGroups];
  int ord_arrived;
  LmHot L;
};

// The launch order of the next pass, from the groups' costs in sh.ord_cost: called by the waves 1 .. THREADS / 64 - 1 of the solver's
// block (wave 0 meanwhile adds the prior's row and steps the optimiser).
template <int THREADS>
__device__ __forceinline__ void build_launch_order(const SolveArgs& a, SolveShared<THREADS>& sh, const int lane, const int wave) {
  auto& ord_cnt = sh.ord_cnt;
  auto& ord_pos = sh.ord_pos;
  auto& ord_cost = sh.ord_cost;
  auto& ord_cls = sh.ord_cls;
  int& ord_arrived = sh.ord_arrived;
  const unsigned long long t_ord = a.dbg_stamps ? __builtin_amdgcn_s_memtime() : 0ull;
  // ---- launch order of the next pass, built by waves 1..7 (costs already in LDS) while lane 0 of wave 0 runs the state machine:
  //      a counting sort into 16 cost classes relative to the slowest group, heaviest class first, ascending group index inside
  //      a class.  (The pass's results do not depend on the launch order.) ----
  // A lone wave is bound by the latency of its own LDS round trips (~600 cycles per 64 groups and loop: 7 us for 866 groups, 17 us
  // for 2217 - longer than the state machine), so every wave sorts a contiguous SLICE of the groups: it counts its slice per class,
  // the seven waves meet at a counter in LDS (all waves of a block are resident: the wait cannot deadlock, and it is bounded), and
  // each then knows where its slice starts inside every class.  No per-lane atomics and no per-class loops: four ballots (one per
  // bit of the class) give every lane the mask of the lanes that share its class; its rank is a popcount, and the lowest lane of
  // each class moves the class's counter in LDS (distinct addresses per class; same-wave LDS operations are ordered).
  constexpr int kSortWaves = THREADS / 64 - 1;
  const int sw = wave - 1;
  auto wsync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  auto same_class = [&](int cls, bool valid) -> unsigned long long {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 4; ++bit) {
      const bool one = (cls >> bit) & 1;
      const unsigned long long bb = __ballot(valid && one);
      m &= one ? bb : ~bb;
    }
    return m;
  };
  if (lane < 16) ord_cnt[sw][lane] = 0;
  int mx = 1;  // (every wave looks at all the costs: no exchange needed for the maximum)
  for (int gi = lane; gi < a.nblocks; gi += 64) mx = max(mx, ord_cost[gi]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
  const float to_class = 16.0f / ((float)mx + 1.0f);  // (a heuristic: float rounding at class boundaries is immaterial)
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int slice = ((a.nblocks + kSortWaves * 64 - 1) / (kSortWaves * 64)) * 64;  // groups per wave, a multiple of 64
  const int g_first = sw * slice, g_last = min(g_first + slice, a.nblocks);
  wsync();
  for (int g0 = g_first; g0 < g_last; g0 += 64) {
    const int gi = g0 + lane;
    const bool valid = gi < g_last;
    const int cls = valid ? 15 - min(15, (int)((float)ord_cost[gi] * to_class)) : 0;
    if (valid) ord_cls[gi] = (unsigned char)cls;
    const unsigned long long m = same_class(cls, valid);
    if (valid && (m & lt) == 0) ord_cnt[sw][cls] += __popcll(m);  // the class's lowest lane
    wsync();
  }
  // the seven waves meet
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if (lane == 0) atomicAdd(&ord_arrived, 1);
  bool met = false;
  for (int spin = 0; spin < (1 << 20); ++spin) {
    if (*reinterpret_cast<volatile int*>(&ord_arrived) >= kSortWaves) {
      met = true;
      break;
    }
    __builtin_amdgcn_s_sleep(2);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (met) {  // (never false in practice; the order of the previous refresh then simply stays)
    if (lane < 16) {  // where this wave's slice starts inside class `lane`
      int run = 0;
      for (int c = 0; c < lane; ++c)
        for (int w = 0; w < kSortWaves; ++w) run += ord_cnt[w][c];
      for (int w = 0; w < sw; ++w) run += ord_cnt[w][lane];
      ord_pos[sw][lane] = run;
    }
    wsync();
    for (int g0 = g_first; g0 < g_last; g0 += 64) {
      const int gi = g0 + lane;
      const bool valid = gi < g_last;
      const int cls = valid ? ord_cls[gi] : 0;
      const unsigned long long m = same_class(cls, valid);
      const int base = ord_pos[sw][cls];
      if (valid) a.grp_order[base + __popcll(m & lt)] = gi;  // within a class: ascending group index
      wsync();
      if (valid && (m & lt) == 0) ord_pos[sw][cls] = base + __popcll(m);
      wsync();
    }
    if (sw == 0 && lane == 0 && a.order_valid) *a.order_valid = 1;
  }
  if (a.dbg_stamps && sw == 0 && lane == 0) a.dbg_stamps[7] = __builtin_amdgcn_s_memtime() - t_ord;
}

// The body of the solver for a block of THREADS threads (512: k_lm_solve; 256: the last block of a fused pass).  AGENT: the group rows
// and costs were written by other blocks of the SAME launch (write-through stores, published by a ticket; the caller has run the
// agent-scope acquire): they are then read with agent-scope loads, which bypass this CU's L1 whatever it holds.
// PERSIST: the solver between two passes of the persistent kernel.  There is no kernel boundary and no fence anywhere: every word another
// block wrote (group rows, costs - and the state image, which the solver of the previous pass, possibly on another XCD, stored) is read
// with agent-scope loads, the state image and the pass's view of it are stored write-through.
template <int THREADS, bool AGENT, bool PERSIST = false>
__device__ __forceinline__ void lm_solve_body(const SolveArgs& a, SolveShared<THREADS>& sh) {
  static_assert(!PERSIST || AGENT, "the persistent solver is an agent-scope one");
  constexpr int kSolveThreads = THREADS;
  constexpr int kSolveSubs = 32;                      // subsets of rows (row g belongs to subset g mod 32), whatever the block size
  constexpr int kThreadSubs = THREADS / 16;           // subsets the block's threads cover at once
  constexpr int kPer = kSolveSubs / kThreadSubs;      // subsets per thread (512 threads: 1, 256 threads: 2)
  constexpr int kSolveChunk = THREADS >= 512 ? NGICP_SOLVE_CHUNK : 14;  // 16-byte loads per subset a thread keeps in flight per step (4 VGPRs each; the fused block has the pass kernel's 168-register budget)
  static_assert(kPer >= 1 && kPer * kThreadSubs == kSolveSubs, "block sizes: 256 or 512 threads");
  auto& wsum = sh.wsum;
  auto& sums = sh.sums;
  auto& ord_cost = sh.ord_cost;
  int& ord_arrived = sh.ord_arrived;
  LmHot& L = sh.L;
  if (threadIdx.x == 0) ord_arrived = 0;  // (visible to every wave after the barriers below)
  LmState* st = a.st;
  LmState* sto = a.st_out ? a.st_out : a.st;
#define NG_SSTAMP(k)                                                                 \
  do {                                                                               \
    if (a.dbg_stamps && threadIdx.x == 0) a.dbg_stamps[k] = __builtin_amdgcn_s_memtime(); \
  } while (0)
  // (as a VECTOR load - an atomic load is never made a scalar one: scalar loads return out of order, so the wait for the kernel arguments the
  // row addresses need would also have waited for this cold word before the first row load could go out.  Persistent: the blocks left
  // the pass loop when they saw the flag.)
  const int done_at_entry = PERSIST ? 0 : __hip_atomic_load(&st->hot.done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  const unsigned long long t_solver_entry = a.dbg_stamps ? __builtin_amdgcn_s_memtime() : 0ull;  // (stored below, once the flag has been looked at:
                                                                                                 // looking at it HERE put a cold scalar round trip in front of every load of the block)
  // ---- deterministic reduction of the group partials.  Thread = (slot pair vp, group subset sb): it adds the rows
  //      sb, sb + 32, sb + 64, ... of its two slots in increasing order, kSolveChunk sixteen-byte loads in flight per step (one step
  //      covers 1280 groups: the whole c3 grid in a single memory round trip, c5 in two); the 32 subset sums of a slot are then added
  //      in subset order.  Fixed order throughout: bit-reproducible, independent of the launch order of the pass. ----
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int vp = threadIdx.x & 15, sb = threadIdx.x >> 4;
  const double2* __restrict__ rows = reinterpret_cast<const double2*>(a.partials) + vp;  // row g: rows[g * 16]
  // Everything the block needs from memory is requested HERE, before the first wait: the state image the serial lane will work on
  // (fetched by the whole block, one coalesced access, instead of by lane 0 after the reduction), the first step of group rows, the
  // groups' measured costs.  Consumed one after the other they were three dependent round trips of ~0.9 us each.
  static_assert(sizeof(LmHot) % 4 == 0, "LmHot is copied as dwords");
  constexpr int kHotWords = (int)(sizeof(LmHot) / 4), kHotPerThread = (kHotWords + kSolveThreads - 1) / kSolveThreads;
  constexpr int kCostPerThread = kMaxOrderGroups / kSolveThreads;
  // (the fused block has three sorting waves instead of seven: the order is refreshed after the first three passes of an alignment -
  // the costs settle with the warm start - and after every fourth from then on, so that it stays off the serial lane's path)
  // (persistent: the blocks keep their groups for the whole alignment; the order built from the costs of the third pass - warm starts in
  // place - goes to the buffer the NEXT alignment launches with)
  const int passes_at_entry = PERSIST ? __hip_atomic_load(&st->hot.passes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : st->hot.passes;
  // (a K4-only pass stores no costs: the order built from the last pass that searched stays, for this alignment's next pass and the next alignment's first)
  const int k4_only_at_entry = (!PERSIST && a.pass_honours_word) ? st->hot.lin_unneeded : 0;
  const bool order_it = a.mode == 0 && a.grp_order && a.nblocks <= kMaxOrderGroups && !k4_only_at_entry && (PERSIST ? passes_at_entry == 2 : (!AGENT || passes_at_entry < 3 || (passes_at_entry & 3) == 3));
  int hv[kHotPerThread];
#pragma unroll
  for (int k = 0; k < kHotPerThread; ++k) {
    const int w = threadIdx.x + k * kSolveThreads;
    if constexpr (PERSIST) hv[k] = w < kHotWords ? __hip_atomic_load(reinterpret_cast<const int*>(&st->hot) + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    else hv[k] = w < kHotWords ? reinterpret_cast<const int*>(&st->hot)[w] : 0;
  }
  // (One CU moves 64 B per clock: the 222 KB of 866 rows are ~3.5k cycles on top of the latency.  Rows beyond the grid are skipped by
  // a branch each: fetching a stand-in row instead - branch-free issue - measured slower, the stand-ins pile up on one channel.)
  const int last_row = (a.nrows ? a.nrows : a.nblocks) - 1, last_grp = a.nblocks - 1;
  // (AGENT: the caller's agent-scope acquire has dropped this CU's L1, the producers stored write-through and no line of these rows
  // can be in this XCD's L2 from before - nobody read them earlier in this launch: plain 16-byte loads, as MI355X_MICROARCH.md's
  // "valid forms" prescribe for the consumer side)
  // (PERSIST: this XCD's L2 may hold the rows of an earlier pass - one of its blocks was the solver then - so the loads say agent scope)
  auto load_row = [](const double2* q) -> double2 {
    if constexpr (PERSIST) {
      const double* d = reinterpret_cast<const double*>(q);
      return make_double2(__hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_load(d + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    } else {
      return *q;
    }
  };
  // (The order of the sums never depends on the block size: 32 subsets of rows; a thread of a 256-thread block takes two of them.)
  double2 p[kPer * kSolveChunk];
#pragma unroll
  for (int sI = 0; sI < kPer; ++sI)
#pragma unroll
    for (int j = 0; j < kSolveChunk; ++j) {
      const int gi = sb + sI * kThreadSubs + j * kSolveSubs;
      p[sI * kSolveChunk + j] = gi <= last_row ? load_row(rows + (size_t)gi * (kNumSlots / 2)) : make_double2(0.0, 0.0);
    }
  int oc[kCostPerThread];
#pragma unroll
  for (int k = 0; k < kCostPerThread; ++k) {
    const int gi = threadIdx.x + k * kSolveThreads;
    if constexpr (PERSIST) oc[k] = (order_it && gi <= last_grp) ? __hip_atomic_load(a.grp_cost + gi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    else oc[k] = (order_it && gi <= last_grp) ? a.grp_cost[gi] : 0;
  }
  // the pose prior's record, one double per lane of wave 0, behind the last load of the same batch and in front of its first wait (no
  // kernel writes the record: a plain load on every route).  Here, where the flag's test ends the basic block anyway: a branch among the
  // loads above would split the block they are scheduled in.
  double prior_v = 0.0;
  if (a.prior && threadIdx.x < kPriorDoubles) prior_v = a.prior[threadIdx.x];
  if (a.mode == 0 && done_at_entry) return;  // (a scalar load issued at the top: it does not wait for the vector loads above)
  if (a.dbg_stamps && threadIdx.x == 0) a.dbg_stamps[0] = t_solver_entry;  // (working launches only)
  // The serial lane works on the LDS image of the state in place (a register-resident copy needs ~260 VGPRs: it spills at two
  // waves per SIMD), and wave 0 stores it back with one coalesced pass.
#pragma unroll
  for (int k = 0; k < kHotPerThread; ++k) {
    const int w = threadIdx.x + k * kSolveThreads;
    if (w < kHotWords) reinterpret_cast<int*>(&L)[w] = hv[k];
  }
  if (order_it) {  // the groups' costs, for the launch order built further down (visible after the barriers below)
#pragma unroll
    for (int k = 0; k < kCostPerThread; ++k) {
      const int gi = threadIdx.x + k * kSolveThreads;
      if (gi < a.nblocks) ord_cost[gi] = oc[k];
    }
  }
  {
    double a0[kPer], a1[kPer];
#pragma unroll
    for (int sI = 0; sI < kPer; ++sI) {
      a0[sI] = p[sI * kSolveChunk].x;  // (not 0.0 + p[0]: the compiler places that add, and a wait for the first load alone, before the other loads)
      a1[sI] = p[sI * kSolveChunk].y;
#pragma unroll
      for (int j = 1; j < kSolveChunk; ++j) {
        a0[sI] += p[sI * kSolveChunk + j].x;
        a1[sI] += p[sI * kSolveChunk + j].y;
      }
    }
    for (int g0 = kSolveSubs * kSolveChunk; g0 + sb <= last_row; g0 += kSolveSubs * kSolveChunk) {  // larger grids: further steps
#pragma unroll
      for (int sI = 0; sI < kPer; ++sI)
#pragma unroll
        for (int j = 0; j < kSolveChunk; ++j) {
          const int gi = g0 + sb + sI * kThreadSubs + j * kSolveSubs;
          p[sI * kSolveChunk + j] = gi <= last_row ? load_row(rows + (size_t)gi * (kNumSlots / 2)) : make_double2(0.0, 0.0);
        }
#pragma unroll
      for (int sI = 0; sI < kPer; ++sI)
#pragma unroll
        for (int j = 0; j < kSolveChunk; ++j) {
          a0[sI] += p[sI * kSolveChunk + j].x;
          a1[sI] += p[sI * kSolveChunk + j].y;
        }
    }
    NG_SSTAMP(1);
#pragma unroll
    for (int sI = 0; sI < kPer; ++sI) {
      wsum[sb + sI * kThreadSubs][2 * vp] = a0[sI];
      wsum[sb + sI * kThreadSubs][2 * vp + 1] = a1[sI];
    }
  }
  __syncthreads();
  if (threadIdx.x < kPartialStride) {
    const int v = threadIdx.x;
    double t = 0.0;
    if (v < kNumSlots)
      for (int sb = 0; sb < kSolveSubs; ++sb) t += wsum[sb][v];
    sums[v] = t;
  }
  __syncthreads();
  NG_SSTAMP(2);
  if (a.sums_out && threadIdx.x < kPartialStride) a.sums_out[threadIdx.x] = sums[threadIdx.x];
  if (a.mode == 3) return;  // reduce only (point-sharded stepping: the caller all-reduces sums_out)
  if (order_it && wave >= 1) build_launch_order<THREADS>(a, sh, lane, wave);
  if (wave != 0) return;
  if (a.prior) {
    // ---- the pose prior: one more (virtual) block row, evaluated at xi - the pose the pass was evaluated at - and added to the sums
    //      AFTER the fixed-order reduction, one addition per sum (include/ngicp.h, "pose prior").  Every mode below then sees the summed
    //      H, b, y0, yi.  The residual (so3_log: one dependent chain) is computed by every lane on values all lanes agree on; the 36
    //      elements of J_p and the 28 sums run one per lane (prior_jac_elem, prior_row_elem: prior_row's own expressions).
    //      Scratch: wsum, idle since the barrier above (only threads of this wave read it, before that barrier). ----
    double* const P = &wsum[0][0];  // [0, 48) the record, [48, 84) J_p row-major, [84, 90) r
    if (lane < kPriorDoubles) P[lane] = prior_v;
    wave_sync();
    double r[6], theta_sq, jc;
    prior_residual(L.xi, P, r, theta_sq, jc);
    if (lane < 36) P[kPriorDoubles + lane] = prior_jac_elem(lane / 6, lane % 6, r[0], r[1], r[2], theta_sq, jc, L.xi.t[0], L.xi.t[1], L.xi.t[2]);
#pragma unroll
    for (int q = 0; q < 6; ++q)
      if (lane == 36 + q) P[kPriorDoubles + 36 + q] = r[q];
    wave_sync();
    // lanes 0..26: H's triangle and b; lane 27: the cost into y0; lane 28: the cost into yi
    if (lane < kPriorRowSums + 1) sums[lane] += prior_row_elem(lane < kPriorRowSums ? lane : kPriorRowSums - 1, P + kPriorDoubles, P + 12, P + kPriorDoubles + 36);
    wave_sync();
  }
  if (a.mode == 2) {  // compute_error hook
    if (lane == 0) st->hot.y0 = sums[28];
    return;
  }
  if (a.mode != 1 && !a.serial_step) {
    // the step on the whole wave (lm_step_wave); the float pose of the next pass goes out as one store by twelve lanes
    NG_SSTAMP(3);
    lm_step_wave(L, a.cfg, sums, a.trace, a.max_trace_rows, !(a.pass_honours_word && L.lin_unneeded), lane);
    NG_SSTAMP(4);
    wave_sync();
    NG_SSTAMP(5);
    if (!L.done && lane < 12) {
      const float f = (float)reinterpret_cast<const double*>(&L.xi)[lane];
      if constexpr (PERSIST) __hip_atomic_store(&st->xi_f[pose_elem_to_rows(lane)], f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else sto->xi_f[pose_elem_to_rows(lane)] = f;
    }
  } else if (lane == 0) {
    if (a.mode == 1) {  // linearize hook
      adopt_new(L, sums);
    } else {
      const LmConfig& cfg = a.cfg;
      NG_SSTAMP(3);
      lm_step(L, cfg, sums, a.trace, a.max_trace_rows, !(a.pass_honours_word && L.lin_unneeded));
      NG_SSTAMP(4);
      NG_SSTAMP(5);
      if (!L.done) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float f = (float)(c < 3 ? L.xi.R[r * 3 + c] : L.xi.t[r]);
            // (persistent: solvers of different passes sit on different XCDs - a plain store would leave one dirty copy of the word per L2)
            if constexpr (PERSIST) __hip_atomic_store(&st->xi_f[r * 4 + c], f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else sto->xi_f[r * 4 + c] = f;
          }
        }
      }
    }
  }
  // wave 0 stores the state image back (lane 0's LDS writes are ordered before the other lanes' reads by the fence pair)
  if (a.mode == 0 && lane == 0 && L.done) {
    L.t_done = __builtin_amdgcn_s_memrealtime();
    if (a.t_first) L.t_first = PERSIST ? __hip_atomic_load(a.t_first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *a.t_first;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const bool finished_now = a.mode == 0 && L.done != 0;
  if constexpr (!PERSIST) {
    // The state image goes back BEFORE the progress word is released (and, at the end of an alignment, before the fence below): when
    // the host sees `done`, the device state it may read next - cur, have_lin, the float pose - is the final one.
    // (xi_f is not carried into the other buffer of k_gicp_head when the alignment ends: after `done` nothing reads it - the exported
    // distances use hot.lin_f, and linearize, compute_error and the next align write xi_f afresh)
    for (int w = lane; w < (int)(sizeof(LmHot) / 4); w += 64) reinterpret_cast<int*>(&sto->hot)[w] = reinterpret_cast<const int*>(&L)[w];
  }
  // The end of an alignment goes to the host WITHOUT a copy or a stream synchronisation: the image is written to pinned memory
  // here, then (system-scope release) the done flag; the host, which polls that word anyway, reads the image as soon as it sees
  // it - the launches it had enqueued ahead return at once behind its back.
  if (finished_now && a.final_host) {
    for (int w = lane; w < (int)(sizeof(LmHot) / 4); w += 64)
      __hip_atomic_store(reinterpret_cast<int*>(a.final_host) + w, reinterpret_cast<const int*>(&L)[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __builtin_amdgcn_wave_barrier();
  }
  // progress for the host (it keeps a few (pass, solve) pairs in flight and stops feeding the stream when it sees the flag)
  if (a.mode == 0 && a.progress_host && lane == 0)
    __hip_atomic_store(a.progress_host, (L.passes & kProgressMask) | (L.done ? kProgressDone : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // (ordered behind the image by the fence above when done)
  if constexpr (PERSIST) {
    for (int w = lane; w < (int)(sizeof(LmHot) / 4); w += 64)
      __hip_atomic_store(reinterpret_cast<int*>(&st->hot) + w, reinterpret_cast<const int*>(&L)[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the next pass's view of the state (LmState::view)
    int v = 0;
    if (lane < 24) {
      v = reinterpret_cast<const int*>(&L.xi)[lane];
    } else if (lane < 36) {
      const int r = (lane - 24) >> 2, cI = (lane - 24) & 3;
      v = __float_as_int((float)(cI < 3 ? L.xi.R[r * 3 + cI] : L.xi.t[r]));
    } else if (lane == kViewDone) {
      v = L.done;
    } else if (lane == kViewCur) {
      v = L.cur;
    } else if (lane == kViewHaveLin) {
      v = L.have_lin;
    }
    __hip_atomic_store(st->view + (size_t)L.passes * kViewWords + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (pass L.passes comes next)
  }
  NG_SSTAMP(6);
#undef NG_SSTAMP
}

__global__ void __launch_bounds__(kSolveThreads) k_lm_solve(SolveArgs a) {
  __shared__ SolveShared<kSolveThreads> sh;
  lm_solve_body<kSolveThreads, false>(a, sh);
}

// Test hook: ONE optimiser step in both forms, lm_step on lane 0 and lm_step_wave on the wave, from the same state image, sums and
// configuration; one block of one wave per problem.
//   in  (kStepSelftestIn doubles): x0 12, xi 12, delta 12, H 36, b 6, y0, d 6, lambda, nu | iter, trial, have_lin, cur, n_trace,
//       lin_unneeded | max_iterations, lm_max_iterations, optimizer, rot_eps, trans_eps, lm_init_lambda_factor | sums 32 | searched
//   out (2 records of kStepSelftestRecord bytes, serial then wave; zeroed by the caller): the LmHot image, the trace row (8 doubles;
//       written when n_trace == 0), d (6 doubles), {done, converged, lm_failed, trial} as doubles
constexpr int kStepSelftestIn = 132;
constexpr size_t kStepSelftestRecord = sizeof(LmHot) + 18 * sizeof(double);
static_assert(sizeof(LmHot) % 8 == 0, "the trace row behind the image is 8-byte aligned");
__global__ void __launch_bounds__(64) k_step_selftest(const double* __restrict__ in, int n_problems, unsigned char* __restrict__ out) {
  __shared__ LmHot L;
  __shared__ double sums[kPartialStride];
  static_assert(kPartialStride >= 32, "32 reduced sums");
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= n_problems) return;
  const double* p = in + (size_t)blockIdx.x * kStepSelftestIn;
  LmConfig cfg;
  cfg.max_iterations = (int)p[93];
  cfg.lm_max_iterations = (int)p[94];
  cfg.optimizer = (int)p[95];
  cfg.rot_eps = p[96];
  cfg.trans_eps = p[97];
  cfg.lm_init_lambda_factor = p[98];
  const bool searched = p[131] != 0.0;
  for (int form = 0; form < 2; ++form) {
    unsigned char* rec = out + ((size_t)blockIdx.x * 2 + form) * kStepSelftestRecord;
    double* tail = reinterpret_cast<double*>(rec + sizeof(LmHot));
    __syncthreads();
    for (int w = lane; w < (int)(sizeof(LmHot) / 4); w += 64) reinterpret_cast<int*>(&L)[w] = 0;
    if (lane < 32) sums[lane] = p[99 + lane];
    __syncthreads();
    if (lane < 36) reinterpret_cast<double*>(&L.x0)[lane] = p[lane];  // x0, xi, delta are contiguous
    if (lane < 36) L.H[lane] = p[36 + lane];
    if (lane < 6) L.b[lane] = p[72 + lane], L.d[lane] = p[79 + lane];
    if (lane == 0) {
      L.y0 = p[78];
      L.lambda = p[85];
      L.nu = p[86];
      L.iter = (int)p[87];
      L.trial = (int)p[88];
      L.have_lin = (int)p[89];
      L.cur = (int)p[90];
      L.n_trace = max(0, (int)p[91]);
      L.lin_unneeded = (int)p[92];
    }
    __syncthreads();
    if (form == 0) {
      if (lane == 0) lm_step(L, cfg, sums, tail, 1, searched);
    } else {
      lm_step_wave(L, cfg, sums, tail, 1, searched, lane);
    }
    __syncthreads();
    for (int w = lane; w < (int)(sizeof(LmHot) / 4); w += 64) reinterpret_cast<int*>(rec)[w] = reinterpret_cast<const int*>(&L)[w];
    if (lane < 6) tail[8 + lane] = L.d[lane];
    if (lane == 0) tail[14] = L.done, tail[15] = L.converged, tail[16] = L.lm_failed, tail[17] = L.trial;
  }
}
static_assert(offsetof(LmHot, xi) == offsetof(LmHot, x0) + sizeof(Pose) && offsetof(LmHot, delta) == offsetof(LmHot, xi) + sizeof(Pose), "x0, xi, delta are contiguous");

}  // namespace ngk
