// The three switch-only routes of an alignment: k_gicp_head (one launch per iteration, every block steps the
// optimiser at its head), k_gicp_queue (a resident grid drawing groups from a counter) and k_gicp_persist (one launch per alignment),
// with persist_group_body, the group body the last two call, and their shared-memory globals.
// Included by ngicp_pass.h only, inside namespace ngk, between the definition of NG_STAMP and its #undef: the group body
// (ngicp_pass_group.inc) stamps through that macro.
#pragma once
#ifndef NG_STAMP
#error "ngicp_pass_routes.h is included by ngicp_pass.h, where NG_STAMP is defined"
#endif

// One group of one pass for the PERSISTENT kernel, which calls it once per group and pass (a function of its own: inlined into that
// kernel's loops, everything the loops keep alive pushed the search's registers into scratch memory - 2.5x the time per pass).  The
// arguments are read where the hardware put them, through the constant address space (a.field is then a scalar load the compiler may
// repeat instead of keeping the value, exactly as in a kernel of its own); the trial pose comes from entry pass_no of the ring of views.
// RING false (k_gicp_queue, one launch per pass): the pose comes from the state itself, which does not change while the launch runs, and
// the block's row is stored plainly - the solver launch reads it behind a kernel boundary.
template <int G, int WPS, bool RING, class A>
__device__ __forceinline__ void persist_group_body(A& a, const int group, const int pass_no, WaveStage* stage_all, double (*lds)[kNumSlots]) {
  constexpr bool FUSED = RING;  // (persistent: the block's row and cost are stored write-through)
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
  // the pass's view of the state: entry pass_no of the ring (see LmState::view) - it does not change while the pass runs
  typedef const int __attribute__((address_space(4))) * ViewPtr;
  typedef const double __attribute__((address_space(4))) * ViewPtrD;
  typedef const float __attribute__((address_space(4))) * ViewPtrF;
  KernelStatePtr st4 = (KernelStatePtr)(unsigned long long)a.st;
  ViewPtr vw = (ViewPtr)(unsigned long long)(a.st->view + (size_t)(a.first_pass + pass_no) * kViewWords);
  const int have_lin = RING ? vw[kViewHaveLin] : st4->hot.have_lin;
  const int cur = (RING ? vw[kViewCur] : st4->hot.cur) & 1, nxt = cur ^ 1;  // (indices into two-element arrays of pointers, whatever the memory holds)
  ViewPtrD vx = RING ? (ViewPtrD)(vw + kViewXi) : (ViewPtrD)&st4->hot.xi;  // (Pose: R[9] then t[3], as in the view)
  ViewPtrF vf = RING ? (ViewPtrF)(vw + kViewXiF) : (ViewPtrF)st4->xi_f;
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
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % G, grp = lane / G;
  WaveStage& S = stage_all[wave];
  NG_STAMP(0);
  const unsigned long long t_start = a.grp_cost ? __builtin_amdgcn_s_memtime() : 0ull;
#define NG_HAVE_LIN have_lin
#include "ngicp_pass_group.inc"
#undef NG_HAVE_LIN
}

// ---- k_gicp_head: ONE launch per iteration, without a grid-wide meeting.  What the solver launch costs an iteration is not its work
//      (~1.6 us of serial FP64 and one read) but its dispatch and the two kernel boundaries around it (13.6 us of 48 at c3).  Here the
//      kernel boundary between two passes is the only synchronisation: the blocks of pass i add their rows up per SUBSET of groups
//      (subset = group index mod 32, the solver's own summation order: the last block of a subset to finish - a ticket per subset,
//      rows written through, read back with agent-scope loads, no fence - adds its subset's rows in ascending group order), and every
//      block of launch i + 1 begins by reading the state image and those 32 rows, adds them in subset order and runs the optimiser's
//      step ITSELF (lm_step, the very function the solver runs; same inputs, same order, so every block arrives at the same pose, and
//      at the bits the two-launch path arrives at).  Block 0 of every launch is the SOLVER BLOCK: the same step through lm_solve_body,
//      with everything that leaves the kernel - the advanced state image (into the other of two buffers: the launch's own blocks are
//      still reading this one), trace rows, the progress word, the final image for the host, the next launch order (into the other
//      of two order buffers, for the same reason).  One more launch than passes: the head that consumes the last pass's rows. ----
struct HeadShared {
  LmHot L;
  double sums[kPartialStride];
  double crow[kSolveRowSubsets][kNumSlots + 1];
};
__device__ __forceinline__ double uniform_double(double v) {  // (a value every lane holds alike, into scalar registers)
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

template <int G, int WPS>
__global__ void __launch_bounds__(256, WPS) k_gicp_head(PassArgs a) {
  constexpr bool FUSED = true;  // (rows and costs are stored write-through: another block of this launch reads the rows)
  constexpr int B = 64 / G;
  constexpr int kWin = WPS >= 4 ? 12 : 16, kSideStep = WPS >= 4 ? 8 : 16;  // (see k_gicp_pass)
  static_assert(kWin <= kSortedPad && B == kBatchQueries, "see k_gicp_pass");
  __shared__ double lds[4][kNumSlots];
  union HeadPassShared {
    WaveStage stage[4];
    SolveShared<256> sv;  // the solver block
    HeadShared hs;        // a search block's head, before its search tables
  };
  __shared__ HeadPassShared shm;
  __shared__ int last_block;
  // Everything the head needs from memory is requested at once - the done word, the state image, the 32 subset rows - and looked at
  // afterwards: one round trip instead of three in a row.
  const unsigned long long t_entry = a.dbg_stamps ? __builtin_amdgcn_s_memtime() : 0ull;
  const LmState* __restrict__ st = a.st;
  const int n_groups = (int)gridDim.x - 1;
  {
    HeadShared& H = shm.hs;
    constexpr int kHotWords = (int)(sizeof(LmHot) / 4);
    static_assert(kHotWords <= 2 * 256, "two words of the state image per thread");
    static_assert(kSolveRowSubsets * kNumSlots == 256 * 4, "a thread fetches four doubles of the subset rows");
    const int done_before = *a.done_flag;  // (an earlier launch has ended the alignment; the host had enqueued this one ahead)
    const int w0 = threadIdx.x, w1 = threadIdx.x + 256;
    const int i0 = reinterpret_cast<const int*>(&st->hot)[w0], i1 = w1 < kHotWords ? reinterpret_cast<const int*>(&st->hot)[w1] : 0;
    const int c = threadIdx.x >> 3, v0 = (threadIdx.x & 7) * 4;
    const double* src = a.crow_in + c * kNumSlots + v0;
    const double r0 = src[0], r1 = src[1], r2 = src[2], r3 = src[3];  // (zeros before the first pass)
    if (done_before) return;
    reinterpret_cast<int*>(&H.L)[w0] = i0;
    if (w1 < kHotWords) reinterpret_cast<int*>(&H.L)[w1] = i1;
    H.crow[c][v0] = r0; H.crow[c][v0 + 1] = r1; H.crow[c][v0 + 2] = r2; H.crow[c][v0 + 3] = r3;
  }
  __syncthreads();
  const bool pending = shm.hs.L.pending != 0;  // (block-uniform)
  if (blockIdx.x == 0) {
    // ---- the solver block
    __syncthreads();  // (lm_solve_body lays its scratch over the head's)
    if (pending) {
      lm_solve_body<256, false>(a.sa, shm.sv);  // (a.sa: partials = the 32 subset rows, st_out = the other state buffer)
      __syncthreads();
      if (threadIdx.x == 0 && shm.sv.L.done) *a.done_flag = 1;
    } else {
      // the first launch of an alignment: nothing to consume yet; the state moves on unchanged, marked as having a pass under way
      LmState* sto = a.sa.st_out;
      for (int w = threadIdx.x; w < (int)(sizeof(LmHot) / 4); w += 256) reinterpret_cast<int*>(&sto->hot)[w] = reinterpret_cast<const int*>(&st->hot)[w];
      if (threadIdx.x < 12) sto->xi_f[threadIdx.x] = st->xi_f[threadIdx.x];
      __syncthreads();
      if (threadIdx.x == 0) sto->hot.pending = 1;
    }
    return;
  }
  // ---- head of a search block: the state this pass runs at.  Wave 0 adds the subset rows (lane v: slot v, subsets in order - the
  //      solver's own order) and its lane 0 steps the optimiser; the other waves wait at the barrier.
  if (pending && threadIdx.x < 64) {
    HeadShared& H = shm.hs;
    if (threadIdx.x < kPartialStride) {
      double tsum = 0.0;
      if (threadIdx.x < kNumSlots)
        for (int c = 0; c < kSolveRowSubsets; ++c) tsum += H.crow[c][threadIdx.x];
      H.sums[threadIdx.x] = tsum;
    }
    wave_lds_sync();
    if (threadIdx.x == 0) lm_step(H.L, a.sa.cfg, H.sums, nullptr, 0);  // (no trace row: the solver block writes it)
  }
  __syncthreads();
  if (shm.hs.L.done) return;  // (block-uniform; the solver block tells the host)
  const int have_lin = __builtin_amdgcn_readfirstlane(shm.hs.L.have_lin);
  const int cur = __builtin_amdgcn_readfirstlane(shm.hs.L.cur) & 1, nxt = cur ^ 1;
  double R[9], t[3];
  float Tf[12];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = uniform_double(shm.hs.L.xi.R[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = uniform_double(shm.hs.L.xi.t[i]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Tf[r * 4 + c] = (float)R[r * 3 + c];
    Tf[r * 4 + 3] = (float)t[r];
  }
  __syncthreads();  // (the search tables lie where the head's scratch was)
  const bool do_err = (a.mode & 1) && have_lin;
  const bool do_lin = (a.mode & 2);
  const float4* __restrict__ tpt_old = a.tpt[cur];
  const double* __restrict__ mahal_old = a.mahal[cur];
  float4* __restrict__ tpt_new = a.tpt[nxt];
  double* __restrict__ mahal_new = a.mahal[nxt];
  const Grid& g = a.grid;
  double wave_total = 0.0;
  unsigned int ncand = 0, nvalid = 0, nstaged = 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % G, grp = lane / G;
  WaveStage& S = shm.stage[wave];
  if (a.dbg_stamps && lane == 0) {  // diagnostic only: entry, end of the head
    unsigned long long* d = a.dbg_stamps + (size_t)(blockIdx.x * 4 + wave) * kStampStride;
    d[20] = t_entry;
    d[21] = __builtin_amdgcn_s_memtime();
  }
  NG_STAMP(0);
  const int slot = (int)blockIdx.x - 1;
  const int group = (a.grp_order && a.order_valid && *a.order_valid) ? a.grp_order[slot] : slot;
  const unsigned long long t_start = a.grp_cost ? __builtin_amdgcn_s_memtime() : 0ull;
  if (a.t_first && slot == 0 && threadIdx.x == 0 && !have_lin) *a.t_first = __builtin_amdgcn_s_memrealtime();
#define NG_HAVE_LIN have_lin
#include "ngicp_pass_group.inc"
#undef NG_HAVE_LIN
  // ---- tail: the last block of the group's subset adds the subset's rows
  const int c = group % kSolveRowSubsets;
  if (wave == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
      const int members = (n_groups - c + kSolveRowSubsets - 1) / kSolveRowSubsets;
      const int tk = __hip_atomic_fetch_add(a.cluster_ticket + c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last_block = (tk == members - 1) ? 1 : 0;
    }
  }
  __syncthreads();
  if (a.dbg_stamps && lane == 0) a.dbg_stamps[(size_t)(blockIdx.x * 4 + wave) * kStampStride + 22] = __builtin_amdgcn_s_memtime();  // (ticket drawn)
  if (!last_block || wave != 0) return;
  if (lane < kNumSlots) {
    // rows c, c + 32, c + 64, ... in ascending order, sixteen loads in flight at a time; rows beyond the grid add 0.0 (as the solver does)
    constexpr int kChunk = 16;
    const double* rows = a.partials + lane;
    double acc = 0.0;
    for (int g0 = c; g0 < n_groups; g0 += kSolveRowSubsets * kChunk) {
      double v[kChunk];
#pragma unroll
      for (int j = 0; j < kChunk; ++j) {
        const int gi = g0 + j * kSolveRowSubsets;
        v[j] = gi < n_groups ? __hip_atomic_load(rows + (size_t)gi * kNumSlots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      }
      if (g0 == c) acc = v[0]; else acc += v[0];
#pragma unroll
      for (int j = 1; j < kChunk; ++j) acc += v[j];
    }
    a.crow_out[c * kNumSlots + lane] = acc;
  }
  if (lane == 0) __hip_atomic_store(a.cluster_ticket + c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (for the next launch: ordered by the kernel boundary)
  if (a.dbg_stamps && lane == 0) a.dbg_stamps[(size_t)(blockIdx.x * 4 + wave) * kStampStride + 23] = __builtin_amdgcn_s_memtime();  // (subset row stored)
}

// ---- the persistent kernel: ONE launch per alignment.  A thin loop over passes and over the block's groups around two CALLED functions
//      (the group body above, the solver): what the loop keeps alive does not compete with the search for registers.  The functions
//      find the kernel's arguments where the hardware put them (the kernel-argument segment), and share the block's LDS as
//      namespace-scope variables (allocated to this kernel only). ----
union PersistShared {
  WaveStage stage[4];
  SolveShared<256> sv;  // the solver (the last block to arrive) works where the search tables were
};
__shared__ PersistShared g_persist_shm;
__shared__ double g_persist_lds[4][kNumSlots];
__shared__ int g_persist_last;
typedef const PassArgs __attribute__((address_space(4))) KernelPassArgs;

// (ka: the kernel's argument segment, handed down by the kernel itself - inside a called function __builtin_amdgcn_kernarg_segment_ptr()
// is the pointer to the kernel's IMPLICIT arguments, behind the explicit ones)
// (Arguments of a called function arrive in vector registers: made wave-uniform again with v_readfirstlane, so that a.field is a
// scalar load and group / pass_no live in scalar registers.)
__device__ __forceinline__ KernelPassArgs* uniform_args(KernelPassArgs* ka) {
  const unsigned long long v = (unsigned long long)ka;
  const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)v), hi = __builtin_amdgcn_readfirstlane((unsigned int)(v >> 32));
  return (KernelPassArgs*)(((unsigned long long)hi << 32) | lo);
}
template <int G, int WPS>
__device__ __attribute__((noinline)) void persist_group_call(KernelPassArgs* ka, int group, int pass_no) {
  persist_group_body<G, WPS, true>(*uniform_args(ka), __builtin_amdgcn_readfirstlane(group), __builtin_amdgcn_readfirstlane(pass_no), g_persist_shm.stage, g_persist_lds);
}

__device__ __attribute__((noinline)) void persist_solve_call(KernelPassArgs* ka) {
  const char* kargs = (const char*)uniform_args(ka);
  lm_solve_body<256, true, true>(*reinterpret_cast<const SolveArgs*>(kargs + offsetof(PassArgs, sa)), g_persist_shm.sv);
}

// ---- k_gicp_queue: one launch per pass, as k_gicp_pass, but a grid of as many blocks as are RESIDENT together, each drawing its next
//      group from a counter (launch order = the order of the draws: heaviest first as before) instead of leaving a freed slot to the
//      dispatcher, which does not refill it at once (c5, 2217 groups over 1024 slots: the slots 15-20 % empty between rounds).  No
//      block waits for another; the solver is a launch of its own as ever. ----
template <int G, int WPS>
__device__ __attribute__((noinline)) void queue_group_call(KernelPassArgs* ka, int group) {
  persist_group_body<G, WPS, false>(*uniform_args(ka), __builtin_amdgcn_readfirstlane(group), 0, g_persist_shm.stage, g_persist_lds);
}

template <int G, int WPS>
__global__ void __launch_bounds__(256, WPS) k_gicp_queue(PassArgs a) {
  if (!(a.mode & 4) && a.st->hot.done) return;
  KernelPassArgs* ka = (KernelPassArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const bool ordered = a.grp_order && a.order_valid && *a.order_valid;
  const int n_groups = (a.n_batches + 3) / 4;
  // The first group of a block is the one of its own number (a thousand blocks drawing from ONE word at the same moment queue up at the
  // memory channel that holds it: measured +10 us per pass at c3, +28 at c5); from then on position gridDim.x + draw.
  int slot = (int)blockIdx.x;
  for (;;) {
    if (a.t_first && slot == 0 && threadIdx.x == 0 && !a.st->hot.have_lin) *a.t_first = __builtin_amdgcn_s_memrealtime();
    queue_group_call<G, WPS>(ka, ordered ? a.grp_order[slot] : slot);
    if (threadIdx.x == 0) g_persist_last = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int draw = g_persist_last;
    __syncthreads();  // (the word is written again in the next turn; the group's row of sums in LDS has been read)
    slot = (int)gridDim.x + draw;
    if (slot >= n_groups) {
      // every block draws exactly one number beyond the groups - n_groups draws in all; the last puts the counter back for the next launch
      if (draw == n_groups - 1 && threadIdx.x == 0) __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
  }
}

template <int G, int WPS>
__global__ void __launch_bounds__(256, WPS) k_gicp_persist(PassArgs a) {
  KernelPassArgs* ka = (KernelPassArgs*)__builtin_amdgcn_kernarg_segment_ptr();  // == &a: where the hardware put the arguments
  const bool ordered = a.grp_order && a.order_valid && *a.order_valid;  // (fixed for the whole alignment: the solver builds the NEXT alignment's order)
  const int n_groups = (a.n_batches + 3) / 4;
  for (int pass_no = 0; pass_no < a.max_passes; ++pass_no) {
    {
      // (the address is made opaque HERE, behind the wait that released the pass: no load of the entry can be placed earlier)
      const int* vw_g = a.st->view + (size_t)(a.first_pass + pass_no) * kViewWords;
      asm volatile("" : "+s"(vw_g));
      typedef const int __attribute__((address_space(4))) * ViewPtr;
      ViewPtr vw = (ViewPtr)(unsigned long long)vw_g;
      if (vw[kViewDone]) break;
      if (a.t_first && blockIdx.x == 0 && threadIdx.x == 0 && !vw[kViewHaveLin])
        __hip_atomic_store(a.t_first, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // The grid is as many blocks as are resident together; block b takes the positions b, 2P - 1 - b, 2P + b, ... of the launch order
    // (heaviest first, then back and forth), the same ones in every pass: a group's correspondences and Mahalanobis matrices stay
    // in its block's CU / XCD from pass to pass.
    for (int turn = 0;; ++turn) {
      const int slot = turn * (int)gridDim.x + ((turn & 1) ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x);
      if (slot >= n_groups) break;
      __syncthreads();  // (the block's row of sums in LDS has been read)
      persist_group_call<G, WPS>(ka, ordered ? a.grp_order[slot] : slot, pass_no);
    }
    // ---- the blocks meet here after every pass.  Every store of this block that another block will read was made by wave 0 as a
    //      write-through store; wave 0 drains them, then one lane takes a ticket (relaxed, agent scope; the ticket counts on, pass after
    //      pass).  The last block to arrive steps the optimiser (no fence: lm_solve_body<.., PERSIST> reads what other blocks wrote with
    //      agent-scope loads and stores the state write-through), then releases the next pass; the others wait for that with one
    //      polling lane each.  Every block of the grid is resident (the host sizes the grid by the occupancy of this very kernel and
    //      launches it cooperatively), the wait is bounded all the same: a block that gives up raises `gen` to a value no pass reaches,
    //      so that every other block leaves too and the grid drains. ----
    constexpr int kGenFailed = 1 << 30;
    if (threadIdx.x < 64) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (threadIdx.x == 0) {
        const int tk = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        g_persist_last = (tk == (pass_no + 1) * (int)gridDim.x - 1) ? 1 : 0;
      }
    }
    __syncthreads();
    static_assert(kGenLines == 256, "one thread of the releasing block per copy of the release word");
    if (g_persist_last) {  // (block-uniform)
      if (a.sa.pass_ticks && threadIdx.x == 0) a.sa.pass_ticks[2 * pass_no] = __builtin_amdgcn_s_memrealtime();
      persist_solve_call(ka);
      if (threadIdx.x < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the state image and the next view were stored by wave 0: its own counter covers them)
      __syncthreads();
      if (a.sa.pass_ticks && threadIdx.x == 0) a.sa.pass_ticks[2 * pass_no + 1] = __builtin_amdgcn_s_memrealtime();
      __hip_atomic_fetch_max(a.gen + threadIdx.x * kGenStride, pass_no + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (threadIdx.x == 0) g_persist_last = 0;
    } else if (a.persist == 2) {
      return;  // (A/B measurement only, one pass per launch: nobody waits)
    } else if (threadIdx.x == 0) {
      // (every poll goes out to memory, and the blocks still working feel ~770 pollers: c3 41 us per pass at one poll per microsecond
      // and block, 36-37 at one per 3.4 us - s_sleep's maximum; sleeping without polls for 3/4 of the previous period first: no better)
      const int* my_gen = a.gen + ((int)blockIdx.x % kGenLines) * kGenStride;
      int seen = 0;
      for (int spin = 0; spin < (1 << 20); ++spin) {  // (~5 s)
        seen = __hip_atomic_load(my_gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen > pass_no) break;
        __builtin_amdgcn_s_sleep(127);
      }
      g_persist_last = (seen <= pass_no || seen >= kGenFailed) ? 2 : 0;
    }
    __syncthreads();
    if (g_persist_last == 2) {  // (block-uniform; the host sees no done flag and falls back to one launch per pass)
      __hip_atomic_fetch_max(a.gen + threadIdx.x * kGenStride, kGenFailed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
    __syncthreads();  // (g_persist_last is written again in the next pass)
  }
}
