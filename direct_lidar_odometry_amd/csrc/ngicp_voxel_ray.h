// Free-space clearing of the rolling voxel map along a scan's rays (include/ngicp.h "rolling voxel map: clearing along
// rays"): per map voxel, how many rays pass through it (miss) and how many end in it (hit); the voxels seen through often enough go.
// The project's own definition; no fidelity to an outside library is claimed.
//
//   count    k_roll_ray_count: one thread per ray, in the source's stored (cell-sorted) order, so the lanes of a wave hold neighbouring
//            rays of similar length.  q = transform_point_f(T, a), c0 / c1 = the cells of the origin and of q (voxel_cell); the walk
//            from c0 to c1 takes |dc_x| + |dc_y| + |dc_z| steps, each along the axis whose next lattice plane the ray meets first
//            (three parameters per step, computed afresh from the cell in double; ties to the lowest axis).  A counted step probes the
//            map's table once (read only); on an occupied cell the record's mean is tested against the ray's line and miss[v] gets one
//            integer atomicAdd.  Behind the walk one probe of c1 and one atomicAdd on hit[v].  The three totals are block sums through
//            LDS and one 64-bit integer atomic per block and total.  *bad when the origin or a point has no cell.
//   flags    k_roll_ray_flags: keep[v] from miss, hit and the stamps; the removal itself is the eviction's (scan, k_roll_compact).
// Every sum is an integer sum: nothing depends on the order in which threads arrive, and two runs are bit-equal.
#pragma once
#include "ngicp_voxel_roll.h"

namespace ngk {

// what a clear counts with, as the kernel takes it
struct RollRayArgs {
  float o[3];        // the origin, in the map frame
  float inv_res;     // 1.0f / (float)res: the mode's cell rule
  double res;
  int near_cells, back_cells, max_steps;
  int use_radius;    // radius_cells > 0
  double r2;         // (radius_cells * res)^2
};

// totals[0 .. 2] += the block's sums of a, b, c (every thread of the block calls this)
__device__ __forceinline__ void roll_ray_block_totals(unsigned int a, unsigned int b, unsigned int c, unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long part[3][256 / 64];
  unsigned long long v[3] = {a, b, c};
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) part[k][wave] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < 256 / 64; ++w) s += part[threadIdx.x][w];
    if (s) atomicAdd(totals + threadIdx.x, s);
  }
}

// One thread per ray s (the point's position in the stored cloud).  table may be null (an empty map that never had one): no cell is
// occupied.  miss / hit: [n_vox] counters, cleared by the caller.  totals: {counted steps, of them in occupied cells, misses}.
__global__ void __launch_bounds__(256) k_roll_ray_count(const float4* __restrict__ pts, int n, RollPose T, RollRayArgs a, const ulonglong2* __restrict__ table, unsigned int mask,
                                                         const double* __restrict__ rec, unsigned int* __restrict__ miss, unsigned int* __restrict__ hit,
                                                         unsigned long long* __restrict__ totals, int* __restrict__ bad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned int n_counted = 0, n_occupied = 0, n_miss = 0;
  if (s < n) {
    const float4 p = pts[s];
    const float3 q = transform_point_f(T.m, p.x, p.y, p.z);
    int cur[3], c1[3];
    const bool ok0 = voxel_cell(a.o[0], a.o[1], a.o[2], a.inv_res, cur[0], cur[1], cur[2]);
    const bool ok1 = voxel_cell(q.x, q.y, q.z, a.inv_res, c1[0], c1[1], c1[2]);
    if (!ok0 || !ok1) {
      atomicOr(bad, 1);
    } else {
      const double od[3] = {(double)a.o[0], (double)a.o[1], (double)a.o[2]};
      const double d[3] = {(double)q.x - od[0], (double)q.y - od[1], (double)q.z - od[2]};
      int left[3], sgn[3];  // steps still to take along the axis; their direction
      double inv[3];
      int N = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int dc = c1[k] - cur[k];
        left[k] = dc < 0 ? -dc : dc;
        sgn[k] = dc > 0 ? 1 : (dc < 0 ? -1 : 0);
        inv[k] = 1.0 / d[k];  // (read only where left[k] > 0: there d[k] != 0)
        N += left[k];
      }
      const double dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
      const int last = min(N - 1 - a.back_cells, a.max_steps);  // the last counted step (the cell behind step j is "step j")
      for (int j = 1; j <= last; ++j) {
        int ax = -1;
        double best = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (left[k] > 0) {
            const double t = ((double)(cur[k] + (sgn[k] > 0 ? 1 : 0)) * a.res - od[k]) * inv[k];
            if (ax < 0 || t < best) {  // (a tie stays with the lower axis)
              ax = k;
              best = t;
            }
          }
        }
        // (j <= last < N: an axis has steps left, ax >= 0; the selects below keep cur / left in registers)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (k == ax) {
            cur[k] += sgn[k];
            --left[k];
          }
        }
        if (j < a.near_cells) continue;
        ++n_counted;
        if (!table) continue;
        unsigned int probes = 0;
        const int v = voxel_lookup(table, mask, voxel_pack(cur[0], cur[1], cur[2]), probes);
        if (v < 0) continue;
        ++n_occupied;
        bool is_miss = true;
        if (a.use_radius) {
          const double* m = rec + (size_t)v * kVoxRec;
          const double w0 = m[0] - od[0], w1 = m[1] - od[1], w2 = m[2] - od[2];
          const double ts = ((w0 * d[0] + w1 * d[1]) + w2 * d[2]) / dd;
          const double e0 = w0 - ts * d[0], e1 = w1 - ts * d[1], e2 = w2 - ts * d[2];
          is_miss = ((e0 * e0 + e1 * e1) + e2 * e2) <= a.r2;
        }
        if (is_miss) {
          ++n_miss;
          atomicAdd(miss + v, 1u);
        }
      }
      if (table) {
        unsigned int probes = 0;
        const int v = voxel_lookup(table, mask, voxel_pack(c1[0], c1[1], c1[2]), probes);
        if (v >= 0) atomicAdd(hit + v, 1u);
      }
    }
  }
  roll_ray_block_totals(n_counted, n_occupied, n_miss, totals);
}

// keep[v] = 0 when voxel v goes: seen through at least min_miss times, never hit, and not protected by its stamp
__global__ void __launch_bounds__(256) k_roll_ray_flags(const unsigned int* __restrict__ miss, const unsigned int* __restrict__ hit, const long long* __restrict__ stamps, int n,
                                                         unsigned int min_miss, long long keep_stamp, int* __restrict__ keep) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const bool gone = miss[v] >= min_miss && hit[v] == 0u && (keep_stamp <= 0 || stamps[v] < keep_stamp);
  keep[v] = gone ? 0 : 1;
}

}  // namespace ngk
