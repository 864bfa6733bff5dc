// The optimiser: the device-resident state (LmHot, LmState, the persistent kernel's ring of views), what a pass takes from it
// (PassPose, load_pose), the solver's arguments (SolveArgs) and LsqRegistration's step in its two forms - lm_step on one lane,
// lm_step_wave on a wave - over ONE set of element expressions (ngicp_math.h, lm_gain_den ...).
// Included by the solver (ngicp_solve.h), by every pass kernel (ngicp_pass.h, ngicp_pass_routes.h, ngicp_batch.h, ngicp_voxel.h: the
// state and the pose; k_gicp_head: lm_step itself) and read by the host (ngicp_handle.h, ngicp_align.h, ngicp_api.hip: the structs,
// tri21 and the kSolve* / kProgress* constants).
#pragma once
#include <stddef.h>

#include "ngicp_math.h"
#include "ngicp_terms.h"

namespace ngk {

struct LmConfig {
  int max_iterations;
  int lm_max_iterations;
  int optimizer;  // 0 GN, 1 LM
  double rot_eps, trans_eps;
  double lm_init_lambda_factor;
};

// Device-resident optimiser state (one per handle).  The solver keeps a private register copy of the
// `hot` part while it works (one batch of loads, one batch of stores; no store->load round trips
// through memory on its serial critical path); `cold` fields are write-only for the solver.
struct LmHot {
  Pose x0;      // current estimate
  Pose xi;      // trial pose the next pass evaluates (== x0 for the first pass / GN)
  Pose delta;   // last step
  double H[36]; // row-major (symmetric), current linearisation
  double b[6];
  double y0;
  double d[6];
  double lambda, nu;
  double cand_total;   // sum over passes of target points distance-tested
  double valid_total;  // sum over passes of gated-in correspondences
  double staged_total; // sum over passes of queries served through the LDS row list of their batch region
  int iter;       // outer iteration index i (impl/lsq_registration_impl.hpp:101-102)
  int trial;      // LM trial index
  int have_lin;   // 0 until the first linearisation exists
  int cur;        // ping-pong half holding the CURRENT correspondences / Mahalanobis
  int done;
  int converged;
  int nr_iterations;
  int lm_failed;
  int n_trace;
  int passes;     // passes that did work
  int pending;    // k_gicp_head only: the rows of a finished pass wait for the next launch's head to step the optimiser with them
  double final_H[36];  // H of the last accepted step, row-major (final_hessian_, impl/lsq_registration_impl.hpp:155,203); identity until then
  unsigned long long t_first, t_done;  // 100 MHz counter at the start of the alignment's first pass / when the solver set `done`
  float lin_f[12];  // float pose (rows of [R|t]) the CURRENT correspondences were searched with: xi_f of the pass that was adopted last
  int lin_unneeded;    // the linearisation at xi can never be adopted, whatever the pass of xi finds (set_lin_unneeded): K4's sum is all the solver reads
  int search_passes;   // passes that searched and linearised: `passes` less the K4-only ones
};
// What a pass needs of the state, as 64 dwords (256 bytes, two cache lines of their own).  The persistent kernel reads the view of pass p
// from entry p of a RING of views that begins at LmState::view and continues behind the state (the solver that ends pass p - 1 stores
// it write-through): an address no CU and no L2 of this launch has touched before cannot be stale anywhere, so the blocks read it
// with plain scalar loads, exactly as a launch-per-pass kernel reads the state - and the compiler may reload the values instead of
// keeping 40 registers alive through the search.
constexpr int kViewXi = 0;     // [24] the trial pose xi: R (9 doubles), t (3 doubles)
constexpr int kViewXiF = 24;   // [12] float(xi), rows of [R|t]
constexpr int kViewDone = 36, kViewCur = 37, kViewHaveLin = 38;
struct LmState {
  LmHot hot;
  float xi_f[12];  // float(xi): rows of [R|t], the matrix used for the NN query (impl/nano_gicp_impl.hpp:178)
  // entry 0 of the persistent kernel's ring of per-pass views (kView*); entries 1 .. max_passes follow at a stride of kViewWords.
  // Every entry lies in cache lines of its own (L2: 128 bytes, scalar cache: 64) with an unused gap behind it: reading entry p must
  // not bring any byte of entry p + 1 into a cache before the solver has written it.
  alignas(512) int view[128];
};
constexpr int kViewWords = 128;
// The release word of the persistent kernel exists kGenLines times, 128 bytes apart; block b waits on copy b % kGenLines.  (With ONE
// word, the ~770 waiting blocks' agent-scope polls - every one goes out to memory - queued on a single channel: whatever else mapped
// to that channel waited behind them, and the blocks still working took 2.5x as long.)
constexpr int kGenLines = 256, kGenStride = 32;
static_assert(sizeof(LmState) % 512 == 0 && offsetof(LmState, view) % 512 == 0, "ring entries are 512-byte aligned");

// What a pass block takes from the state before it touches a point: the trial pose in FP64 and in float, and the flags.
struct PassPose {
  double R[9], t[3];
  float Tf[12];
  int have_lin, cur;
};
typedef const LmState __attribute__((address_space(4))) * KernelStatePtr;  // the state read with scalar loads: it does not change during a launch
// S: a pointer to the state, generic (k_vgicp_pass, k_vgicp_pass_n) or KernelStatePtr (k_vgicp_pass_batch).  The `done` flag is the
// caller's to test.
template <class S>
__device__ __forceinline__ void load_pose(S st, PassPose& p) {
  p.have_lin = st->hot.have_lin;
  p.cur = st->hot.cur;
#pragma unroll
  for (int i = 0; i < 9; ++i) p.R[i] = st->hot.xi.R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) p.t[i] = st->hot.xi.t[i];
#pragma unroll
  for (int i = 0; i < 12; ++i) p.Tf[i] = st->xi_f[i];
}

struct SolveArgs {
  LmState* st;
  LmConfig cfg;
  const double* partials;  // [nblocks][kNumSlots] group-major (nblocks == 1: one pre-reduced vector)
  int nblocks;
  double* trace;           // [max_rows][8]
  int max_trace_rows;
  int mode;                // 0: LM/GN state machine; 1: reduce -> H/b/y0 (linearize hook); 2: reduce -> y0 = yi (error hook); 3: reduce only
  double* sums_out;        // optional [kPartialStride] reduced sums (29 sums + 2 counters + 1 pad)
  int* grp_order;          // [nblocks] out: groups sorted by measured cost, heaviest first (mode 0 only), or null
  const int* grp_cost;     // [nblocks] in: duration of each group's block in the pass just finished
  unsigned long long* dbg_stamps;  // diagnostic only: [8] s_memtime stamps of the last launch, or null
  int* progress_host;      // pinned host memory, or null: {passes done | kProgressDone} published after every step (mode 0)
  LmHot* final_host;       // pinned host memory, or null: the state image, written when the alignment is done, BEFORE the done flag goes out
  int* order_valid;        // device word: the solver has published a group order (heaviest first) for the next pass
  const unsigned long long* t_first;  // device word the first pass of an alignment stamps (100 MHz counter)
  LmState* st_out;         // where the advanced state goes (null: back to st).  k_gicp_head: the blocks of the launch read st while its solver block writes
  int nrows;               // rows of `partials` (0: nblocks, one per group).  k_gicp_head: 32 rows, already added up per subset by the pass's blocks
  int persist;             // the solver runs between two passes of ONE launch: every word other blocks (on other XCDs) wrote or will read
                           // goes through agent-scope loads / write-through stores, and the launch order it builds is for the NEXT alignment
  int pass_honours_word;   // the pass kernel of this route skips search and linearisation when LmHot::lin_unneeded says so (PassArgs::mode bit 6):
                           // such a pass counts in `passes` but not in `search_passes`, and its costs do not refresh the launch order
  int serial_step;         // env NGICP_SERIAL_STEP=1: lane 0 of wave 0 runs lm_step (the reference form) instead of the wave running lm_step_wave
                           // (fills the padding in front of the next pointer: the size of the struct, and of PassArgs, does not change)
  unsigned long long* pass_ticks;  // persist: [2 * max passes] 100 MHz ticks {last block arrived, next pass released} per pass, or null
  const double* prior;     // the pose prior's record in device memory (kPriorDoubles: R_p 9, t_p 3, Lambda 36; written by the host before
                           // the launch, never by a kernel), or null: no prior.  Wave 0 adds prior_row at xi to the reduced sums (modes 0, 1, 2)
};

static_assert(offsetof(SolveArgs, pass_ticks) == offsetof(SolveArgs, pass_honours_word) + 8, "serial_step takes no room of its own");

// Upper-triangular packing used by the pass: index of (r,c), r <= c, in the 21-vector
__host__ __device__ __forceinline__ int tri21(int r, int c) { return r * 6 - (r * (r - 1)) / 2 + (c - r); }

constexpr int kMaxOrderGroups = 4096;  // launch-order sort: groups whose costs fit the solver's LDS and one load round (8 per thread)
constexpr int kSolveThreads = 512;  // 8 waves = 2 per SIMD: the serial lane keeps a 256-VGPR budget, the reduction gets 512 loaders
constexpr int kSolveRowSubsets = 32;  // the solver adds the group rows in 32 subsets (row g belongs to subset g mod 32), then the subsets in order
constexpr int kProgressDone = 1 << 30, kProgressMask = kProgressDone - 1;

__device__ __forceinline__ bool is_converged_dev(const Pose& d, double rot_eps, double trans_eps) {  // impl/lsq_registration_impl.hpp:118-127
  double rmax = 0.0, tmax = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rmax = fmax(rmax, 1.0 / rot_eps * fabs(d.R[r * 3 + c] - (r == c ? 1.0 : 0.0)));
    tmax = fmax(tmax, 1.0 / trans_eps * fabs(d.t[r]));
  }
  return fmax(rmax, tmax) < 1;
}

// The scalar expressions of the LM step, ONE definition each for the serial step (lm_step) and the wave-level one (lm_step_wave):
// the denominator of the gain ratio (impl/lsq_registration_impl.hpp:196), |d|^2 of the trace row, lambda after an accepted trial (:202).
__device__ __forceinline__ double lm_gain_den(const double* d, const double* b, const double lambda) {
  double den = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) den += d[i] * (lambda * d[i] - b[i]);
  return den;
}
__device__ __forceinline__ double lm_step_norm2(const double* d) {
  double dn = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) dn += d[i] * d[i];
  return dn;
}
__device__ __forceinline__ double lm_lambda_accepted(const double lambda, const double rho) {
  const double q = 2 * rho - 1;
  return lambda * fmax(1.0 / 3.0, 1 - q * q * q);
}

// d = (H + lambda I)^-1 (-b); delta = (so3_exp(d[0:3]), d[3:6]); xi = delta * x0
__device__ __forceinline__ void make_trial(LmHot& L, double lambda_add) {
  double A[36], rhs[6];
#pragma unroll
  for (int i = 0; i < 36; ++i) A[i] = L.H[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    A[i * 6 + i] += lambda_add;
    rhs[i] = -L.b[i];
  }
  ldlt6_solve(A, rhs, L.d);
  pose_identity(L.delta);
  so3_exp_matrix(L.d, L.delta.R);
  L.delta.t[0] = L.d[3];
  L.delta.t[1] = L.d[4];
  L.delta.t[2] = L.d[5];
  pose_mul(L.delta, L.x0, L.xi);
}

// The trial just made (LM) can only END the alignment or be tried again from the SAME linearisation, so the linearisation its pass would
// produce at xi can never be adopted:
//   1. its step already satisfies the convergence test: accepted, lm_step sets `converged` and `done` without adopt_new
//      (impl/lsq_registration_impl.hpp:110,118-127); rejected, lm_advance ends the alignment too (:191-194);
//   2. it is the trial of the last outer iteration (iter + 1 >= max_iterations): accepted means done (:101-102); rejected means another
//      trial from the unchanged H, b (for which this holds again) or "lm not converged" (:105-108,207).
// Both are known here, one pass ahead.  A pass kernel that honours the word (PassArgs::mode bit 6) then evaluates K4 alone.
__device__ __forceinline__ void set_lin_unneeded(LmHot& L, const LmConfig& cfg) {
  L.lin_unneeded = (is_converged_dev(L.delta, cfg.rot_eps, cfg.trans_eps) || L.iter + 1 >= cfg.max_iterations) ? 1 : 0;
}

// new linearisation (reduced sums in LDS) becomes current
__device__ __forceinline__ void adopt_new(LmHot& L, const double* sums) {
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) L.H[r * 6 + c] = L.H[c * 6 + r] = sums[tri21(r, c)];
#pragma unroll
  for (int i = 0; i < 6; ++i) L.b[i] = sums[21 + i];
  L.y0 = sums[27];
  L.cur ^= 1;
  L.have_lin = 1;
  // (the pass that produced these sums searched with float(xi); later passes may have moved xi_f on - a trial that was not adopted, or
  // the accepted step that ended the alignment - so the squared distances of the current correspondences are taken at this pose)
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) L.lin_f[r * 4 + c] = (float)L.xi.R[r * 3 + c];
    L.lin_f[r * 4 + 3] = (float)L.xi.t[r];
  }
}

// One step of LsqRegistration's optimiser on the register-resident state.  Returns true when H was
// accepted as final_hessian_ (impl/lsq_registration_impl.hpp:155,203).
__device__ __forceinline__ bool lm_advance(LmHot& L, const LmConfig& cfg, const double* sums, double* trace, int max_trace_rows) {
  const double yi = sums[28];
  L.passes += 1;
  L.cand_total += sums[29];
  L.valid_total += sums[30];
  L.staged_total += sums[31];

  if (cfg.optimizer == 0) {
    // ---- Gauss-Newton: impl/lsq_registration_impl.hpp:142-158, one pass per outer iteration ----
    adopt_new(L, sums);
    L.nr_iterations = L.iter;
    make_trial(L, 0.0);
    L.x0 = L.xi;
    L.converged = is_converged_dev(L.delta, cfg.rot_eps, cfg.trans_eps) ? 1 : 0;
    L.iter += 1;
    if (L.converged || L.iter >= cfg.max_iterations) L.done = 1;
    return true;
  }

  // ---- Levenberg-Marquardt: impl/lsq_registration_impl.hpp:161-208 ----
  if (!L.have_lin) {
    // first pass: linearisation at the initial guess
    adopt_new(L, sums);
    L.nr_iterations = 0;
    if (L.lambda < 0.0) {
      double m = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) m = fmax(m, fabs(L.H[i * 6 + i]));
      L.lambda = cfg.lm_init_lambda_factor * m;
    }
    L.nu = 2.0;
    L.trial = 0;
    if (cfg.lm_max_iterations <= 0) {  // the reference's inner loop would not run: "lm not converged"
      L.lm_failed = 1;
      L.done = 1;
      return false;
    }
    make_trial(L, L.lambda);
    set_lin_unneeded(L, cfg);
    return false;
  }

  const double den = lm_gain_den(L.d, L.b, L.lambda), dn = lm_step_norm2(L.d);
  const double rho = (L.y0 - yi) / den;
  const bool rejected = rho < 0;  // NaN is accepted, as upstream
  if (trace && L.n_trace < max_trace_rows) {
    double* row = trace + (size_t)L.n_trace * kTraceCols;
    row[0] = L.iter; row[1] = L.trial; row[2] = L.y0; row[3] = yi;
    row[4] = rho; row[5] = L.lambda; row[6] = sqrt(dn); row[7] = rejected ? 0.0 : 1.0;
    L.n_trace += 1;
  }
  if (rejected) {
    if (is_converged_dev(L.delta, cfg.rot_eps, cfg.trans_eps)) {  // :191-194 — x0 stays, step reports success
      L.converged = 1;
      L.done = 1;
      return false;
    }
    L.lambda = L.nu * L.lambda;
    L.nu = 2 * L.nu;
    L.trial += 1;
    if (L.trial >= cfg.lm_max_iterations) {  // :207 -> "lm not converged!!", break (:105-108)
      L.lm_failed = 1;
      L.converged = 0;
      L.done = 1;
      return false;
    }
    make_trial(L, L.lambda);
    set_lin_unneeded(L, cfg);
    return false;
  }
  // accepted (:201-204); final_hessian_ = H is written by the caller BEFORE the state is advanced
  return true;
}

// One step of the optimiser's state machine with the sums of a finished pass (the serial lane of the solver; k_gicp_head's blocks run it
// redundantly, each for itself): lm_advance, and on an accepted trial the bookkeeping of LsqRegistration::align's outer loop.
// searched: the pass that produced `sums` searched and linearised (false: K4 alone, a route that honours LmHot::lin_unneeded).
__device__ __forceinline__ void lm_step(LmHot& L, const LmConfig& cfg, const double* sums, double* trace, int max_trace_rows, const bool searched = true) {
  const bool gn = cfg.optimizer == 0;
  L.search_passes += searched ? 1 : 0;
  const bool accepted = lm_advance(L, cfg, sums, trace, max_trace_rows);
  if (accepted) {
#pragma unroll
    for (int i = 0; i < 36; ++i) L.final_H[i] = L.H[i];
    if (!gn) {
      // LM accept: x0 = xi, lambda update, convergence, next outer iteration (impl/lsq_registration_impl.hpp:201-204,110)
      const double rho = (L.y0 - sums[28]) / lm_gain_den(L.d, L.b, L.lambda);
      L.x0 = L.xi;
      L.lambda = lm_lambda_accepted(L.lambda, rho);
      L.converged = is_converged_dev(L.delta, cfg.rot_eps, cfg.trans_eps) ? 1 : 0;
      L.iter += 1;
      if (L.converged || L.iter >= cfg.max_iterations) {
        L.done = 1;
      } else {
        // the speculative linearisation at xi (== new x0) becomes current
        adopt_new(L, sums);
        L.nr_iterations = L.iter;
        L.nu = 2.0;
        L.trial = 0;
        make_trial(L, L.lambda);
        set_lin_unneeded(L, cfg);
      }
    }
  }
  if (gn && !L.done) L.xi = L.x0;  // GN: the next pass linearises at the updated estimate
}

// ---- the same step on a whole wave (lm_step_wave) --------------------------------------------------------------------------------
// Every lane of ONE wave calls these with the same arguments; L and sums lie in LDS.  Whatever has at most 36 independent elements
// runs one element per lane (the factorisation, the division by the pivots, pose_mul, the copies and the float casts); what is a short
// dependent chain (the gain ratio, the substitutions, so3_exp, the convergence test) is computed by every lane on values all lanes
// agree on.  Decisions are taken from such values only, so control flow is wave-uniform.  The element expressions are lm_step's own
// (ngicp_math.h, lm_gain_den ...): the two forms agree bit for bit (ngicp_step_selftest).
__device__ __forceinline__ void wave_sync() {  // LDS written by some lanes of the wave is read by others
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double wave_lane_f64(const double v, const int src_lane) {  // src_lane: a compile-time constant
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src_lane), __builtin_amdgcn_readlane(__double2loint(v), src_lane));
}
__device__ __forceinline__ double wave_fetch_f64(const double v, const int src_lane) {  // per-lane source
  return __hiloint2double(__builtin_amdgcn_ds_bpermute(src_lane << 2, __double2hiint(v)), __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2loint(v)));
}
__device__ __forceinline__ bool wave_agree(const bool b) { return __builtin_amdgcn_readfirstlane(b ? 1 : 0) != 0; }
// where element e of a Pose (R row-major, then t) sits in a float pose (rows of [R|t])
__device__ __forceinline__ int pose_elem_to_rows(const int e) { return e < 9 ? (e / 3) * 4 + e % 3 : (e - 9) * 4 + 3; }

__device__ __forceinline__ void adopt_new_wave(LmHot& L, const double* sums, const int lane) {
  if (lane < 36) {
    const int i = lane / 6, j = lane - 6 * i;
    L.H[lane] = sums[tri21(min(i, j), max(i, j))];
  }
  if (lane < 6) L.b[lane] = sums[21 + lane];
  if (lane < 12) L.lin_f[pose_elem_to_rows(lane)] = (float)reinterpret_cast<const double*>(&L.xi)[lane];
  if (lane == 0) {
    L.y0 = sums[27];
    L.cur ^= 1;
    L.have_lin = 1;
  }
}

// make_trial and, when `lin_word`, set_lin_unneeded (iter: the value L.iter has by then)
__device__ __forceinline__ void make_trial_wave(LmHot& L, const LmConfig& cfg, const double lambda_add, const bool lin_word, const int iter, const int lane) {
  wave_sync();
  const bool act = lane < 36;
  const int i = act ? lane / 6 : 0, j = act ? lane - 6 * i : 0;
  const int r = max(i, j), c = min(i, j);
  double a = act ? L.H[lane] : 0.0;
  if (act && i == j) a += lambda_add;
  double y[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) y[e] = -L.b[e];
  // pose_mul's right-hand operand for this lane's output: column (lane % 3) of x0.R, or x0.t
  const bool out_t = lane >= 9;
  const int orow = lane < 12 ? (out_t ? lane - 9 : lane / 3) : 0, ocol = lane < 9 ? lane % 3 : 0;
  double xb[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) xb[m] = out_t ? L.x0.t[m] : L.x0.R[m * 3 + ocol];
  // ---- ldlt6_solve's factorisation, element (i, j) on lane 6 i + j ----
  int piv[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    int p = k;
    double best = fabs(wave_lane_f64(a, 7 * k));
#pragma unroll
    for (int q = k + 1; q < 6; ++q) {
      const double v = fabs(wave_lane_f64(a, 7 * q));
      if (v > best) {
        best = v;
        p = q;
      }
    }
    p = __builtin_amdgcn_readfirstlane(p);
    piv[k] = p;
    if (p != k) {  // rows k and p, then columns k and p: element (i, j) comes from (s(i), s(j)), s the transposition
      const int si = i == k ? p : (i == p ? k : i), sj = j == k ? p : (j == p ? k : j);
      a = wave_fetch_f64(a, si * 6 + sj);
    }
    if (k < 5) {
      const double dk = wave_lane_f64(a, 7 * k);
      if (dk != 0.0 && isfinite(dk)) {
        const double scaled = ldlt_scale(a, dk);
        if (act && j == k && i > k) a = scaled;
        // (the serial form updates the lower triangle and mirrors it: lane (i, j) evaluates element (max, min))
        const double upd = ldlt_update(wave_fetch_f64(a, r * 6 + c), wave_fetch_f64(a, r * 6 + k), dk, wave_fetch_f64(a, c * 6 + k));
        if (act && i > k && j > k) a = upd;
      }
    }
  }
  // ---- the substitutions: every lane, on the factor's 21 entries as wave-uniform values; the six divisions on the diagonal's lanes ----
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int q = k + 1; q < 6; ++q)
      if (piv[k] == q) {
        const double t = y[k];
        y[k] = y[q];
        y[q] = t;
      }
  double lo[15];
#pragma unroll
  for (int q = 1; q < 6; ++q)
#pragma unroll
    for (int e = 0; e < q; ++e) lo[q * (q - 1) / 2 + e] = wave_lane_f64(a, q * 6 + e);
#pragma unroll
  for (int q = 0; q < 6; ++q)
#pragma unroll
    for (int e = 0; e < q; ++e) y[q] = ldlt_subst(y[q], lo[q * (q - 1) / 2 + e], y[e]);
  {
    double mine = y[0];
#pragma unroll
    for (int q = 1; q < 6; ++q) mine = lane == 7 * q ? y[q] : mine;
    const double dv = ldlt_diag(mine, a);
#pragma unroll
    for (int q = 0; q < 6; ++q) y[q] = wave_lane_f64(dv, 7 * q);
  }
#pragma unroll
  for (int q = 5; q >= 0; --q)
#pragma unroll
    for (int e = q + 1; e < 6; ++e) y[q] = ldlt_subst(y[q], lo[e * (e - 1) / 2 + q], y[e]);
#pragma unroll
  for (int k = 5; k >= 0; --k)
#pragma unroll
    for (int q = k + 1; q < 6; ++q)
      if (piv[k] == q) {
        const double t = y[k];
        y[k] = y[q];
        y[q] = t;
      }
  // ---- delta = (so3_exp(d[0:3]), d[3:6]) on every lane; xi = delta * x0, one output per lane ----
  Pose delta;
  so3_exp_matrix(y, delta.R);
  delta.t[0] = y[3];
  delta.t[1] = y[4];
  delta.t[2] = y[5];
  double ar[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) ar[m] = orow == 0 ? delta.R[m] : (orow == 1 ? delta.R[3 + m] : delta.R[6 + m]);
  const double at = orow == 0 ? delta.t[0] : (orow == 1 ? delta.t[1] : delta.t[2]);
  const double xr = pose_mul_r(ar[0], ar[1], ar[2], xb[0], xb[1], xb[2]), xt = pose_mul_t(ar[0], ar[1], ar[2], xb[0], xb[1], xb[2], at);
  if (lane < 12) reinterpret_cast<double*>(&L.xi)[lane] = out_t ? xt : xr;
  const bool conv = lin_word ? is_converged_dev(delta, cfg.rot_eps, cfg.trans_eps) : false;
  if (lane == 0) {
#pragma unroll
    for (int e = 0; e < 6; ++e) L.d[e] = y[e];
    L.delta = delta;
    if (lin_word) L.lin_unneeded = (conv || iter + 1 >= cfg.max_iterations) ? 1 : 0;
  }
}

// lm_step, executed by the 64 lanes of one wave.  The image L is complete (for any lane of this wave) after a wave_sync().
__device__ __forceinline__ void lm_step_wave(LmHot& L, const LmConfig& cfg, const double* sums, double* trace, int max_trace_rows, const bool searched, const int lane) {
  const double yi = sums[28];
  int iter = L.iter;
  double lambda = L.lambda;
  const int have_lin = L.have_lin;
  if (lane == 0) {
    L.search_passes += searched ? 1 : 0;
    L.passes += 1;
    L.cand_total += sums[29];
    L.valid_total += sums[30];
    L.staged_total += sums[31];
  }
  // Every path that goes on makes ONE trial, at the end (make_trial_wave is the bulk of the code: one copy of it, not one per path).
  const bool gn = cfg.optimizer == 0;
  bool go_on = true;  // wave-uniform
  if (gn) {
    // ---- Gauss-Newton (lm_advance's first branch; the rest behind the trial) ----
    adopt_new_wave(L, sums, lane);
    lambda = 0.0;
  } else if (!wave_agree(have_lin != 0)) {
    // ---- Levenberg-Marquardt, first pass: linearisation at the initial guess ----
    adopt_new_wave(L, sums, lane);
    if (wave_agree(lambda < 0.0)) {
      double m = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) m = fmax(m, fabs(sums[tri21(i, i)]));
      lambda = cfg.lm_init_lambda_factor * m;
    }
    go_on = cfg.lm_max_iterations > 0;
    if (lane == 0) {
      L.nr_iterations = 0;
      L.lambda = lambda;
      L.nu = 2.0;
      L.trial = 0;
      if (!go_on) L.lm_failed = 1, L.done = 1;
    }
  } else {
    double d[6], b[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) d[e] = L.d[e], b[e] = L.b[e];
    const double y0 = L.y0, nu = L.nu;
    const int trial = L.trial, n_trace = L.n_trace;
    const double rho = (y0 - yi) / lm_gain_den(d, b, lambda);
    const bool rejected = wave_agree(rho < 0);  // NaN is accepted, as upstream
    if (trace && n_trace < max_trace_rows && lane == 0) {
      double* row = trace + (size_t)n_trace * kTraceCols;
      row[0] = iter; row[1] = trial; row[2] = y0; row[3] = yi;
      row[4] = rho; row[5] = lambda; row[6] = sqrt(lm_step_norm2(d)); row[7] = rejected ? 0.0 : 1.0;
      L.n_trace = n_trace + 1;
    }
    const bool conv = wave_agree(is_converged_dev(L.delta, cfg.rot_eps, cfg.trans_eps));  // (of the trial just evaluated: both branches ask)
    if (rejected) {
      const bool failed = !conv && trial + 1 >= cfg.lm_max_iterations;
      go_on = !conv && !failed;
      if (!conv) lambda = nu * lambda;
      if (lane == 0) {
        if (conv) {
          L.converged = 1, L.done = 1;
        } else {
          L.lambda = lambda;
          L.nu = 2 * nu;
          L.trial = trial + 1;
          if (failed) L.lm_failed = 1, L.converged = 0, L.done = 1;
        }
      }
    } else {
      // accepted: final_H = H, x0 = xi, lambda, convergence, next outer iteration
      if (lane < 36) L.final_H[lane] = L.H[lane];
      if (lane < 12) reinterpret_cast<double*>(&L.x0)[lane] = reinterpret_cast<const double*>(&L.xi)[lane];
      lambda = lm_lambda_accepted(lambda, rho);
      iter += 1;
      go_on = !(conv || iter >= cfg.max_iterations);
      if (lane == 0) {
        L.lambda = lambda;
        L.converged = conv ? 1 : 0;
        L.iter = iter;
        if (!go_on) L.done = 1;
      }
      if (go_on) {
        adopt_new_wave(L, sums, lane);
        if (lane == 0) {
          L.nr_iterations = iter;
          L.nu = 2.0;
          L.trial = 0;
        }
      }
    }
  }
  if (!wave_agree(go_on)) return;
  make_trial_wave(L, cfg, lambda, !gn, iter, lane);
  if (gn) {
    // lm_advance's Gauss-Newton bookkeeping and lm_step's final_H (its `xi = x0` copies what x0 was just given)
    wave_sync();
    if (lane < 12) reinterpret_cast<double*>(&L.x0)[lane] = reinterpret_cast<const double*>(&L.xi)[lane];
    if (lane < 36) L.final_H[lane] = L.H[lane];
    const bool conv = wave_agree(is_converged_dev(L.delta, cfg.rot_eps, cfg.trans_eps));
    if (lane == 0) {
      L.nr_iterations = iter;
      L.converged = conv ? 1 : 0;
      L.iter = iter + 1;
      if (conv || iter + 1 >= cfg.max_iterations) L.done = 1;
    }
  }
}

}  // namespace ngk
