// The exact 1-NN search's building blocks: the packed target points, the total order on candidates (nn_better, group_min), the
// build switches of the walks with what was measured for each, a wave's LDS tables (WaveStage), the outward walks along an x-sorted
// run (scan_global_outward, scan_quad_outward) and the per-query shell walk (nn_shells).
// Included by ngicp_pass.h for the group body (ngicp_pass_group.inc, whatever kernel includes it) and for ngicp_pass_st.h; the host
// launches k_pack_pos / k_pack_xyz when it builds a target index.
#pragma once
#include "ngicp_grid.h"

namespace ngk {

struct alignas(4) Xyz { float x, y, z; };
__device__ __forceinline__ float sqdist(float qx, float qy, float qz, const Xyz& p) {
  const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
  float r = dx * dx;
  r = r + dy * dy;
  r = r + dz * dz;
  return r;
}

// the float pose (xi_f / lin_f: rows of [R|t], row-major 3x4) times a point, in the NN query's order: ((c0*x + c1*y) + c2*z) + c3.
// (not transform_point_f, ngicp_cloudops.h: that one takes a column-major 4x4 and adds in another order)
__device__ __forceinline__ float3 transform_point_rowmajor_f(const float* Tf, float x, float y, float z) {
  float3 q;
  q.x = ((Tf[0] * x + Tf[1] * y) + Tf[2] * z) + Tf[3];
  q.y = ((Tf[4] * x + Tf[5] * y) + Tf[6] * z) + Tf[7];
  q.z = ((Tf[8] * x + Tf[9] * y) + Tf[10] * z) + Tf[11];
  return q;
}

// sorted float4 points (with their sentinel frame) -> the same points carrying their sorted position instead of their original index
__global__ void __launch_bounds__(256) k_pack_pos(const float4* __restrict__ in, int n_padded, int pad, float4* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_padded) return;
  const float4 p = in[i];
  const bool real = i >= pad && i < n_padded - pad;
  out[i] = make_float4(p.x, p.y, p.z, __int_as_float(real ? i - pad : -1));
}

// sorted float4 points (with their sentinel frame) -> the packed copy
__global__ void __launch_bounds__(256) k_pack_xyz(const float4* __restrict__ in, int n, Xyz* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = in[i];
  out[i] = Xyz{p.x, p.y, p.z};
}

// --- cooperative exact 1-NN ------------------------------------------------------------------
template <int G>
__device__ __forceinline__ void group_min(float& d, int& p) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    const float od = __shfl_xor(d, o);
    const int op = __shfl_xor(p, o);
    const bool take = (od < d) || (od == d && (unsigned)op < (unsigned)p);
    d = take ? od : d;
    p = take ? op : p;
  }
}

// Nearest-neighbour candidates are ranked by (squared distance, sorted target position).  The reference
// keeps the first point its kd-tree visits among exactly equidistant ones (impl/nanoflann_impl.hpp:184-211),
// which no other index can mirror (SURVEY.md §7 "Ties"); a total order makes the winner independent of how
// rows are dealt to lanes and of the order in which windows are looked at.
__device__ __forceinline__ bool nn_better(float d, int p, float best, int bestp) { return d < best || (d == best && (unsigned)p < (unsigned)bestp); }

// --- the fused pass ------------------------------------------------------------------------------
// Work decomposition: a wave owns ONE tile-aligned batch of up to 32 consecutive queries in Morton-tile order (a
// compact 3-D blob; batches are cut at index-build time so that none leaves its tile); a block is the four waves of
// four consecutive batches (a GROUP: they share most of their target rows, and with them the CU's L1).  Per batch:
//   index    the wave pushes the batch's bounding box through the trial pose, grows it by as many rings as fit the
//            row table (up to the number that covers the distance gate) and fetches, in ONE round trip, the bounds
//            of every (y,z) row of that region in the cell-sorted target (a row is one contiguous, x-sorted run).
//            The NON-EMPTY rows go into an LDS list, nearest ring first: empty space costs nothing afterwards;
//   search   2 lanes per query set it up (transform, cell, warm start from the previous correspondence).  Every (query, row)
//            pair that the (y,z)-gap test does not rule out becomes a UNIT in an LDS queue; whichever lane is free pops the
//            next unit and walks that row: the bounds of the row's cells around qx, then 12-point windows from where qx sits
//            (interpolated) outward, right / left, only while the x-gap alone does not rule the rest out.  Results meet in a
//            per-query 64-bit LDS atomic min on (distance bits, position).  Ring 1 (the 3 x 3 window rows) first; a query that
//            is not provably exact after it queues the listed rows that can still hold a closer point; rings beyond the list
//            use the per-query shell walk;
//   tail     lanes 0..31, one query each, FP64: K4 error under the previous correspondences, gate, Mahalanobis,
//            residual / Jacobian / normal equations.  Its operands were requested before the search.
// Target points are NOT staged in LDS: measured on MI355X, copying a region's rows (LDS-DMA, 640 points per wave) cost
// more than it saved - the 8 MB target lives in L2 / Infinity Cache, a walk touches 8-16 points of a row, and the LDS
// the copies needed held occupancy at 8 waves per CU.  What pays is the row LIST (which rows exist, where they start)
// and 12 waves per CU hiding the walks' latency.
// Partial sums are stored per GROUP ([group][slot]: one 256-byte row per block), so that the result does not depend on the
// order in which the groups are launched - which the solver sorts by measured cost.
constexpr int kStageRowsPerLane = 4;
constexpr int kStageRows = 64 * kStageRowsPerLane;  // (y,z) rows of a batch region
constexpr int kStageXs = 20;         // cells per row of the region
constexpr int kStageMaxGrow = 6;

#ifndef NGICP_PASS_WAVES
#define NGICP_PASS_WAVES 3  // waves per SIMD the pass kernel is compiled for by default.  4 fits (128 VGPRs with 6 spilled dwords, 40 KB LDS per
                            // block) and was measured: c3 +5 %, c2 +6 %, c5 -5 % in time - twelve waves already saturate a CU's gather path on
                            // a grid of one round of blocks; the host launches the 4-wave build on grids of more than two rounds
#endif
#ifndef NGICP_WALK_WINDOW
#define NGICP_WALK_WINDOW 12
#endif

#ifndef NGICP_WALK_PREFETCH
#define NGICP_WALK_PREFETCH 0  // (measured: c3 32.8 -> 35.8 us, c5 39.2 -> 41.2: the extra requests cost more than the warm lines save) 0: none; 1: the adjacent point of the next window(s); 2: their far end (scan_global_outward)
#endif
#ifndef NGICP_PRE_FAR
#define NGICP_PRE_FAR 0  // (measured: exact, no faster - c3 34.1 vs 33.7 us, c5 43.1 vs 41.3) listed rows queued together with the ring-1 units when the warm start says they will be needed (ngicp_pass_group.inc)
#endif
#ifndef NGICP_ALIGNED_WINDOWS
#define NGICP_ALIGNED_WINDOWS 0
#endif
constexpr int kWalkWindow = NGICP_WALK_WINDOW;  // points per walk window (one memory round trip); <= kSortedPad
static_assert(kWalkWindow <= kSortedPad && kWalkWindow % 2 == 0, "walk windows may overhang the array by at most the sentinel frame");

constexpr int kUnitCap = 288;         // queued (query, row) walks per round (ring 1 needs 32 queries x 9 rows)

struct WaveStage {
  union {
    struct {
      int4 live[kStageRows];  // one record per NON-EMPTY row of the region, nearest ring first: {y | z << 16, points, first point, -}
      int qstat[32][3];       // diagnostic counters (PassArgs::dbg_qstats)
    };
    double red[16 * 30];  // the per-batch reduction reuses the (then idle) tables as scratch, sixteen queries at a time
  };
  // Work distribution inside the wave: a (query, row) walk is a UNIT.  Units are queued here and popped by whichever lane is
  // free, so a query that needs twenty rows is served by twenty lanes instead of its own two while the lanes of queries that
  // needed one row would idle.  Results meet in qkey by a 64-bit atomic min on (distance bits, position): the total order.
  unsigned long long qkey[32];  // per query: nearest so far
  float4 qtab[32];              // per query: transformed coordinates
  // a unit, of ring 1 and of a listed row alike: {query | row code << 5 | (start - run start) << 9, run start, run end, (y,z) gap}; row code:
  // 0..8 the row's place in the 3 x 3 window, 9 a listed row (whose run is the whole row).  Written by whoever queues the unit, so that the
  // drain needs nothing but the unit and its query's two words.
  int unit_q[kUnitCap], unit_s[kUnitCap], unit_e[kUnitCap];
  float unit_g[kUnitCap];
  int q_tail, q_head;
};
static_assert(sizeof(WaveStage) <= 9872 && 4 * sizeof(WaveStage) + 4 * 32 * sizeof(double) <= 40 * 1024 + 512,
              "four of these and the block's row of sums are the pass kernel's 40 KB of LDS per block: more, and a CU holds a block less");

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Outward scan of an x-sorted run [s, e) in GLOBAL memory from a starting guess m: walk right, then left, each until the
// x-gap alone rules the rest out.  Any start is correct (a side only stops once it is past qx AND out of reach); a good
// start (interpolated from the cell geometry: points of a dense scan line are nearly equidistant in x) makes the cost
// O(points within reach) with no search at all.  This is what keeps dense scan lines affordable.
template <int W = kWalkWindow, int kStep = kWalkWindow, class PT>
__device__ __forceinline__ void scan_global_outward(const PT* __restrict__ tgt, int s, int e, int m, float qx, float qy, float qz, float gyz, float gate_sq,
                                                    float& best, int& pos, unsigned int& ncand, unsigned int& gsteps) {
  if (e <= s) return;
  gsteps += 0x10000u;
  m = min(max(m, s), e - 1);
  // ONE loop body serves the three kinds of step (the 8 points around the start, then 8 more to the right while that side is
  // alive, then to the left): a window [w, w + 8) of the run, always read in increasing position, so that c[0] / c[7] are its
  // smallest / largest x and, among equal distances, the first one met has the smallest position (strict `<` below).
  // Most walks end after the first window: both neighbours are ruled out by their x-gap alone.
  // Packed 12-byte points are read FOUR AT A TIME as three 16-byte loads (windows begin at a multiple of four points, i.e. of 48
  // bytes; the array and its sentinel frame are 16-byte aligned): 12 load instructions per 16-point window instead of 16.  What a
  // launch queues on is the CU's address path, per wave instruction (scripts/micro/vmem_issue.hip).
  constexpr bool kQuadLoads = NGICP_ALIGNED_WINDOWS && sizeof(PT) == 12 && W % 4 == 0 && kStep % 4 == 0;
  const int w0 = kQuadLoads ? ((m - W / 2) & ~3) : m - W / 2;
  int w = w0, dir = 0, lo = w0, hi = w0 + W;  // [lo, hi) has been read
  int wn = W;  // points of the current window: W around the start, kStep on either side after that.  Measured with W = 12: side windows
               // of 8 / 6 / 4 points examine 8 / 12 / 16 % fewer candidates and cost c3 +3 / +7 / +18 %, c2 +1 / +6 / +16 % in time (more
               // dependent steps) but c5 -3 % (8 points): the build for large grids, bound by what its waves fetch, uses 8
  static_assert(kStep >= 2 && kStep <= W, "side windows are at most as long as the first");
  bool go_left = false;
  for (;;) {
    // No index clamps: a window that overhangs [s, e) reads points of the neighbouring runs (genuine target points: they can
    // only be legitimate candidates) or the sentinels that frame the array (infinitely far).  The x-gap tests below only
    // look at the window's last / first point when its right / left end is inside the run.
    const PT* __restrict__ q = tgt + w;  // one address, immediate offsets
    PT c[W];
    if constexpr (kQuadLoads) {
      const float4* __restrict__ q4 = reinterpret_cast<const float4*>(q);
      float4 r[3 * W / 4];
#pragma unroll
      for (int j = 0; j < 3 * W / 4; ++j)
        if (j < 3 * kStep / 4 || wn == W) r[j] = q4[j];
#pragma unroll
      for (int j = 0; j < W / 4; ++j) {
        if (j < kStep / 4 || wn == W) {
          const float4 r0 = r[3 * j], r1 = r[3 * j + 1], r2 = r[3 * j + 2];
          c[4 * j].x = r0.x; c[4 * j].y = r0.y; c[4 * j].z = r0.z;
          c[4 * j + 1].x = r0.w; c[4 * j + 1].y = r1.x; c[4 * j + 1].z = r1.y;
          c[4 * j + 2].x = r1.z; c[4 * j + 2].y = r1.w; c[4 * j + 2].z = r2.x;
          c[4 * j + 3].x = r2.y; c[4 * j + 3].y = r2.z; c[4 * j + 3].z = r2.w;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < W; ++j)
        if (j < kStep || wn == W) c[j] = q[j];
    }
    // Software prefetch: one word of the window(s) the walk would read NEXT (after the first window: the one on either side; later: the
    // next in the walk's direction), requested together with this window and looked at only after it has been worked on.  Four in ten
    // walks go on to a second window, and a step whose line is already in the L2 is a third of a step that goes out to memory.
    unsigned int pf = 0;
    if constexpr (NGICP_WALK_PREFETCH != 0) {
      if (dir >= 0 && hi < e) pf ^= *reinterpret_cast<const unsigned int*>(tgt + (hi + (NGICP_WALK_PREFETCH > 1 ? kStep - 1 : 0)));
      if (dir <= 0 && lo > s) pf ^= *reinterpret_cast<const unsigned int*>(tgt + (lo - (NGICP_WALK_PREFETCH > 1 ? kStep : 1)));
    }
    float lb = sqdist(qx, qy, qz, c[0]);
    int lj = 0;
#pragma unroll
    for (int j = 1; j < W; ++j) {
      if (j < kStep || wn == W) {
        const float d = sqdist(qx, qy, qz, c[j]);
        if (d < lb) { lb = d; lj = j; }
      }
    }
    if (nn_better(lb, w + lj, best, pos)) { best = lb; pos = w + lj; }
    ncand += wn;
    ++gsteps;
    if constexpr (NGICP_WALK_PREFETCH != 0) gsteps += (pf == 0x7fc0beefu) ? 0x100u : 0u;  // (keeps the prefetched word alive until here; gsteps is a diagnostic counter)
    const float lim = fminf(best, gate_sq), dr = (wn == W ? c[W - 1].x : c[kStep - 1].x) - qx, dl = qx - c[0].x;
    const bool more_right = hi < e && !(dr > 0.f && dr * dr + gyz > lim);
    const bool more_left = lo > s && !(dl > 0.f && dl * dl + gyz > lim);
    if (dir == 0) go_left = more_left;
    if (dir >= 0 && more_right) {
      dir = 1;
      w = hi;
      hi += kStep;
      wn = kStep;
    } else if (dir >= 0 ? go_left : more_left) {
      dir = -1;
      lo -= kStep;
      w = lo;
      wn = kStep;
    } else {
      break;
    }
  }
}

// The same walk done by the FOUR lanes of a quad on one run: lane ql of the quad reads the points w + ql, w + ql + 4, ... of a window,
// so one load instruction of the quad covers four consecutive points (48 contiguous bytes) and a W-point window is W / 4 wave
// instructions instead of W.  The CU's address path is what a launch queues on (a scattered gather costs it ~20 cycles per wave
// instruction plus ~0.7 per distinct line, scripts/micro/vmem_issue.hip), and a dependent step of a walk is as long as the
// instructions of the waves queued ahead of it: four times fewer of them per window.  All control flow is quad-uniform; (best, pos)
// come back identical on the four lanes.  The winner is the same as scan_global_outward's: smallest (distance, position).
#ifndef NGICP_WALK_LANES
#define NGICP_WALK_LANES 1
#endif
constexpr int kWalkLanes = NGICP_WALK_LANES;  // 1: a lane walks a run by itself; 4: a quad does
template <int CTRL>
__device__ __forceinline__ int quad_perm_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }
template <int CTRL>
__device__ __forceinline__ float quad_perm_f(float v) { return __int_as_float(quad_perm_i<CTRL>(__float_as_int(v))); }
template <int W, int kStep, class PT>
__device__ __forceinline__ void scan_quad_outward(const PT* __restrict__ tgt, int s, int e, int m, float qx, float qy, float qz, float gyz, float gate_sq,
                                                  float& best, int& pos, unsigned int& ncand, unsigned int& gsteps, int ql) {
  static_assert(W % 4 == 0 && kStep % 4 == 0 && kStep >= 4 && kStep <= W, "windows are dealt to the four lanes of a quad");
  constexpr int PER = W / 4, PERS = kStep / 4;
  if (e <= s) return;
  gsteps += 0x10000u;
  m = min(max(m, s), e - 1);
  int w = m - W / 2, dir = 0, lo = m - W / 2, hi = m - W / 2 + W;  // [lo, hi) has been read
  int wn = W;
  bool go_left = false;
  for (;;) {
    const PT* __restrict__ q = tgt + (w + ql);  // (no index clamps: see scan_global_outward)
    PT c[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (j < PERS || wn == W) c[j] = q[4 * j];
    float lb = sqdist(qx, qy, qz, c[0]);
    int lj = 0;
#pragma unroll
    for (int j = 1; j < PER; ++j) {
      if (j < PERS || wn == W) {
        const float d = sqdist(qx, qy, qz, c[j]);
        if (d < lb) { lb = d; lj = j; }
      }
    }
    int lp = w + ql + 4 * lj;
    // the window's first / last x: lane 0's first point, lane 3's last
    const float xl = quad_perm_f<0x00>(c[0].x), xr = quad_perm_f<0xff>(wn == W ? c[PER - 1].x : c[PERS - 1].x);
    {
      const float od = quad_perm_f<0xb1>(lb);
      const int op = quad_perm_i<0xb1>(lp);
      if (nn_better(od, op, lb, lp)) { lb = od; lp = op; }
    }
    {
      const float od = quad_perm_f<0x4e>(lb);
      const int op = quad_perm_i<0x4e>(lp);
      if (nn_better(od, op, lb, lp)) { lb = od; lp = op; }
    }
    if (nn_better(lb, lp, best, pos)) { best = lb; pos = lp; }
    if (ql == 0) ncand += wn;
    ++gsteps;
    const float lim = fminf(best, gate_sq), dr = xr - qx, dl = qx - xl;
    const bool more_right = hi < e && !(dr > 0.f && dr * dr + gyz > lim);
    const bool more_left = lo > s && !(dl > 0.f && dl * dl + gyz > lim);
    if (dir == 0) go_left = more_left;
    if (dir >= 0 && more_right) {
      dir = 1;
      w = hi;
      hi += kStep;
      wn = kStep;
    } else if (dir >= 0 ? go_left : more_left) {
      dir = -1;
      lo -= kStep;
      w = lo;
      wn = kStep;
    } else {
      break;
    }
  }
}

// Outer shells (Chebyshev radius > rdone) without a row list; continues from the (best, pos) found in rings 0..rdone
// until the exactness bound or the distance gate ends the search.  Rows whose (y,z) gap already exceeds the reach are skipped
// without a memory access; the bounds of the others are fetched in chunks of 4 rows before any row is walked (most shell
// rows are empty, so a lane pays one memory round trip per chunk instead of one per row); the walks are x-pruned like
// everywhere else, so a large distance gate costs O(R^2) rows per shell, not O(R^3) points.
template <int G, class PT>
__device__ __forceinline__ void nn_shells(const Grid& g, const PT* __restrict__ tgt, const int* __restrict__ cell_start, float qx, float qy, float qz,
                                          int cx, int cy, int cz, float gate_sq_f, int sub, int rdone, float& best, int& pos, unsigned int& ncand) {
  const int rmax = max(max(g.nx, g.ny), g.nz);
  unsigned int steps = 0;
  for (int r = rdone;; ++r) {
    const float bound = unexplored_bound_sq(g, qx, qy, qz, cx, cy, cz, r);
    if (best <= bound || bound >= gate_sq_f || r >= rmax) break;
    // shell r + 1: rows t = sub, sub + G, ... of the (2R+1)^2 (y,z) window clipped to the grid
    const int R = r + 1;
    const int z0 = max(cz - R, 0), z1 = min(cz + R, g.nz - 1);
    const int y0 = max(cy - R, 0), y1 = min(cy + R, g.ny - 1);
    const int xa = max(cx - R, 0), xb = min(cx + R, g.nx - 1);
    const bool lo = cx - R >= 0, hi = cx + R <= g.nx - 1;
    const int wy = y1 - y0 + 1;
    const int nrows = wy * (z1 - z0 + 1);
    const float xfrac = fminf(fmaxf((qx - (g.ox + (float)xa * g.h)) / ((float)(xb + 1 - xa) * g.h), 0.f), 1.f);
    for (int t0 = sub; t0 < nrows; t0 += 4 * G) {
      int s0[4], e0[4], s1[4], e1[4];
      float gap[4];
      const float lim = fminf(best, gate_sq_f);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + u * G;
        const bool ok = t < nrows;
        const int z = z0 + (ok ? t : 0) / wy, y = y0 + (ok ? t : 0) % wy;
        const int row = (z * g.ny + y) * g.nx;
        const bool face = z == cz - R || z == cz + R || y == cy - R || y == cy + R;
        gap[u] = row_gap_sq(g, y, z, cy, cz, qy, qz);
        const bool want = ok && gap[u] <= lim;
        // face rows: one run [xa, xb] (marked by s1 = -1); interior rows: the two end cells
        const int a0 = face ? xa : cx - R, a1 = face ? xb + 1 : cx - R + 1;
        const bool use0 = want && (face || lo), use1 = want && !face && hi;
        s0[u] = use0 ? cell_start[row + a0] : 0;
        e0[u] = use0 ? cell_start[row + a1] : 0;
        s1[u] = use1 ? cell_start[row + cx + R] : (face ? -1 : 0);
        e1[u] = use1 ? cell_start[row + cx + R + 1] : 0;
      }
#pragma unroll 1
      for (int u = 0; u < 4; ++u) {
        int a0 = s0[0], b0 = e0[0], a1 = s1[0], b1 = e1[0];
        float gp = gap[0];
#pragma unroll
        for (int v = 1; v < 4; ++v)
          if (u == v) a0 = s0[v], b0 = e0[v], a1 = s1[v], b1 = e1[v], gp = gap[v];
        if (gp > fminf(best, gate_sq_f)) continue;
        // a face row starts where qx sits in it; the end cells start at their end nearest to the query
        if (b0 > a0) scan_global_outward(tgt, a0, b0, a1 < 0 ? a0 + (int)(xfrac * (float)(b0 - a0)) : b0 - 1, qx, qy, qz, gp, gate_sq_f, best, pos, ncand, steps);
        if (b1 > a1 && a1 >= 0) scan_global_outward(tgt, a1, b1, a1, qx, qy, qz, gp, gate_sq_f, best, pos, ncand, steps);
      }
    }
    if (G > 1) group_min<G>(best, pos);
  }
}

}  // namespace ngk
