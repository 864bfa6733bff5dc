// Queries on the indexed clouds that the registration path does not use: the fitness score of an alignment, exact k-NN of
// arbitrary points on either index (k_knn_queries, ngicp_knn.h) and radius search.
//
//   fitness   pcl::Registration::getFitnessScore(max_range).  PCL's sources are not under /root/reference (nor installed here): the
//             definition is RESTATED FROM MEMORY, not pinned: transform the input cloud by final_transformation_
//             (pcl::transformPointCloud), take every transformed point's exact 1-NN squared distance d2 in the target (float), and
//             when d2 <= max_range (compared in double: max_range is a SQUARED distance) add it to a double sum and count the point;
//             the score is sum / count, or DBL_MAX when nothing counts.  The per-point d2 are bit-identical to the engine's other
//             paths (transform_point_f, sqdist: no FMA); the sum is a fixed-order reduction (per lane, per wave, per block, then one
//             block over the block partials), so it is bitwise reproducible but may differ from PCL's sequential sum in the last bits.
//   radius    KdTreeFLANN::radiusSearch (include/nano_gicp/nanoflann.hpp:155-175): RadiusResultSet<float,int> keeps a point when
//             its float squared distance is STRICTLY below the float-converted radius (impl/nanoflann_impl.hpp:239-262: the radius
//             is a squared distance).  The reference trees are unsorted (nanoflann.hpp:68,113-117) and return kd-tree visiting order;
//             here the same set comes back in ascending (d2, original index) order.
//
// Radius search pipeline (host: ngicp_api.hip):
//   k_radius_walk<false>   per query, the cell rows (y, z) that overlap the cube [q - r, q + r]; a row's cells x0..x1 are one
//                          contiguous span of the cell-sorted points, walked kRadLanes points at a time; counts[q] = hits
//   k_scan64_tiles / k_scan2_tile_sums / k_scan64_apply   64-bit exclusive scan of the counts -> offsets[nq + 1]
//   k_radius_walk<true>    the same walk, one 64-bit key per hit: (float bits of d2) << 32 | original index (d2 >= 0, so the
//                          key order is the (d2, index) order)
//   k_seg_sort_short       segments of 2..kSegShort keys: one wave per segment, bitonic sort in LDS
//   k_seg_sort_long        longer segments: one block per segment, the same network in global memory
//   k_radius_unpack        keys -> index + d2 (ngicp_radius_fetch)
#pragma once
#include "ngicp_cloudops.h"
#include "ngicp_knn.h"

namespace ngk {

// ---------------------------------------------------------------------------------------------
// fitness score
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {  // butterfly: every lane ends with the same, fixed-order sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// A pair of lanes per source point, in the source's cell-sorted order (neighbouring pairs walk neighbouring target cells); the
// exact 1-NN is knn_search with k = 1.  Grid (blocks, B): row blockIdx.y serves transform blockIdx.y of T_colmajor[B][16];
// partials[blockIdx.y * gridDim.x + blockIdx.x] = {sum of the counted d2, count}.  ngicp_fitness_score launches B = 1,
// ngicp_fitness_score_batch one row per lane: the same kernel, so a lane's sums are the single call's bit for bit.
__global__ void __launch_bounds__(kKnnBlock) k_fitness(const float4* __restrict__ src_sorted, int n, const float* __restrict__ T_colmajor,
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

// block l: out[l] = the sum of partials[l * nb .. l * nb + nb), in a fixed order (strided per thread, then wave butterflies, then the
// waves in order)
constexpr int kFitnessFinalBlock = 256;
__global__ void __launch_bounds__(kFitnessFinalBlock) k_fitness_final(const double2* __restrict__ partials, int nb, double2* __restrict__ out) {
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

// ---------------------------------------------------------------------------------------------
// radius search
// ---------------------------------------------------------------------------------------------
constexpr int kRadLanes = 16;   // lanes per query: a row span is tested 16 points per round trip
constexpr int kRadBlock = 256;  // 16 queries per block

// cells [a, b] of one axis that may hold a point within `reach` of q (clamped: the border cells hold the clamped outliers)
__device__ __forceinline__ void cell_span(float o, float inv_h, int nc, float q, float reach, int& a, int& b) {
  const float lo = floorf((q - reach - o) * inv_h), hi = floorf((q + reach - o) * inv_h);
  a = (int)fminf(fmaxf(lo, 0.f), (float)(nc - 1));
  b = (int)fminf(fmaxf(hi, 0.f), (float)(nc - 1));
}

// radius: the float squared radius (a hit is d2 < radius); reach: a conservative bound of sqrt(radius) plus the grid's slack (the
// float distance test decides membership, the cell range only has to contain every hit).  kFill = false: counts[q] = hits, and
// the queries with more than kSegShort hits are listed in long_list (order irrelevant: each segment is sorted on its own).
// kFill = true: the keys of query q go to keys[offsets[q] ..  offsets[q + 1]).
constexpr int kSegShort = 512;  // longest segment sorted by one wave in LDS (see k_seg_sort_short)
template <bool kFill>
__global__ void __launch_bounds__(kRadBlock) k_radius_walk(const float4* __restrict__ sorted, const int* __restrict__ cells, Grid g, const float4* __restrict__ queries,
                                                           int nq, float radius, float reach, int* __restrict__ counts, const unsigned long long* __restrict__ offsets,
                                                           unsigned long long* __restrict__ keys, int* __restrict__ long_list, int* __restrict__ n_long) {
  const int lane = threadIdx.x & 63, sub = lane & (kRadLanes - 1), grp = lane / kRadLanes;
  const int q = (blockIdx.x * kRadBlock + threadIdx.x) / kRadLanes;
  if (q >= nq) return;  // (the whole group)
  const float4 p = queries[q];
  int x0, x1, y0, y1, z0, z1;
  cell_span(g.ox, g.inv_h, g.nx, p.x, reach, x0, x1);
  cell_span(g.oy, g.inv_h, g.ny, p.y, reach, y0, y1);
  cell_span(g.oz, g.inv_h, g.nz, p.z, reach, z0, z1);
  unsigned long long out = 0, end = 0;
  if (kFill) {
    out = offsets[q];
    end = offsets[q + 1];
  }
  int cnt = 0;
  const unsigned int below = (1u << sub) - 1u;
  for (int z = z0; z <= z1; ++z)
    for (int y = y0; y <= y1; ++y) {
      const int row = (z * g.ny + y) * g.nx;
      const int s = cells[row + x0], e = cells[row + x1 + 1];
      for (int base = s; base < e; base += kRadLanes) {
        const int i = base + sub;
        float d = 0.f;
        int id = 0;
        bool hit = false;
        if (i < e) {
          const float4 c = sorted[i];
          d = sqdist(p.x, p.y, p.z, c);
          id = __float_as_int(c.w);
          hit = d < radius;
        }
        const unsigned int m = (unsigned int)(__ballot(hit) >> (grp * kRadLanes)) & 0xffffu;
        if (kFill && hit) {
          const unsigned long long at = out + (unsigned long long)(cnt + __popc(m & below));
          if (at < end) keys[at] = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)id;
        }
        cnt += __popc(m);
      }
    }
  if (!kFill && sub == 0) {
    counts[q] = cnt;
    if (cnt > kSegShort) long_list[atomicAdd(n_long, 1)] = q;
  }
}

// 64-bit exclusive scan of int counts: tile sums here, their scan by k_scan2_tile_sums (ngicp_grid.h), then the per-element offsets
__global__ void __launch_bounds__(kScanBlock) k_scan64_tiles(const int* __restrict__ counts, int n, unsigned long long* __restrict__ tile_sums) {
  __shared__ unsigned long long lds[4];
  const int base = blockIdx.x * kScanTile + threadIdx.x * kScanPerThread;
  unsigned long long s = 0;
#pragma unroll
  for (int j = 0; j < kScanPerThread; ++j) s += (base + j < n) ? (unsigned long long)(unsigned int)counts[base + j] : 0ull;
  unsigned long long total;
  block_exclusive_scan64(s, lds, total);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}
// out[i] = exclusive prefix of counts, out[n] = the total (out has n + 1 entries)
__global__ void __launch_bounds__(kScanBlock) k_scan64_apply(const int* __restrict__ counts, int n, const unsigned long long* __restrict__ tile_offsets,
                                                             unsigned long long* __restrict__ out) {
  __shared__ unsigned long long lds[4];
  const int base = blockIdx.x * kScanTile + threadIdx.x * kScanPerThread;
  unsigned long long c[kScanPerThread];
  unsigned long long s = 0;
#pragma unroll
  for (int j = 0; j < kScanPerThread; ++j) {
    c[j] = (base + j < n) ? (unsigned long long)(unsigned int)counts[base + j] : 0ull;
    s += c[j];
  }
  unsigned long long total;
  unsigned long long ex = block_exclusive_scan64(s, lds, total) + tile_offsets[blockIdx.x];
#pragma unroll
  for (int j = 0; j < kScanPerThread; ++j) {
    const int i = base + j;
    if (i < n) out[i] = ex;
    ex += c[j];
    if (i == n - 1) out[n] = ex;
  }
}

// Ascending sort of a[0..n) by the bitonic network in its "flip" form: every comparator puts the minimum at the lower index, so the
// network for the next power of two sorts n elements when the missing ones are taken as +infinity - a comparator whose upper index
// is >= n is skipped.  Thread tid of nt runs comparators tid, tid + nt, ... of each step; sync() orders the steps.
template <class Sync>
__device__ __forceinline__ void bitonic_sort_u64(unsigned long long* a, int n, int tid, int nt, Sync sync) {
  int np = 1;
  while (np < n) np <<= 1;
  for (int k = 2; k <= np; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (np >> 1); t += nt) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // t with a 0 inserted at bit log2(j)
        const int u = j == (k >> 1) ? (i ^ (k - 1)) : (i ^ j);  // the flip (mirror inside the k-block), then half-cleaners
        if (u < n) {
          const unsigned long long lo = a[i], hi = a[u];
          if (hi < lo) {
            a[i] = hi;
            a[u] = lo;
          }
        }
      }
      sync();
    }
}

// Segments of 2..kSegShort keys, one wave each (4 per block), sorted in the wave's 4 KB of LDS.  kSegShort = 512 keeps the LDS of a
// block at 16 KB, so that 8 blocks (32 waves, the CU's maximum) fit in the CU's 160 KB: LDS does not limit the occupancy.
constexpr int kSegBlock = 256;
__global__ void __launch_bounds__(kSegBlock) k_seg_sort_short(const unsigned long long* __restrict__ offsets, int nq, unsigned long long* __restrict__ keys) {
  __shared__ unsigned long long lds[kSegBlock / 64][kSegShort];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * (kSegBlock / 64) + wave;
  if (q >= nq) return;
  const unsigned long long off = offsets[q];
  const int len = (int)(offsets[q + 1] - off);
  if (len < 2 || len > kSegShort) return;  // (wave-uniform)
  unsigned long long* a = lds[wave];
  auto wave_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  for (int t = lane; t < len; t += 64) a[t] = keys[off + t];
  wave_sync();
  bitonic_sort_u64(a, len, lane, 64, wave_sync);
  for (int t = lane; t < len; t += 64) keys[off + t] = a[t];
}

// Segments of more than kSegShort keys (listed by k_radius_walk<false>): one block each, the same network in place in global memory
constexpr int kSegLongBlock = 1024;
__global__ void __launch_bounds__(kSegLongBlock) k_seg_sort_long(const unsigned long long* __restrict__ offsets, const int* __restrict__ long_list,
                                                                 unsigned long long* __restrict__ keys) {
  const int q = long_list[blockIdx.x];
  const unsigned long long off = offsets[q];
  const int len = (int)(offsets[q + 1] - off);
  bitonic_sort_u64(keys + off, len, (int)threadIdx.x, kSegLongBlock, [] { __syncthreads(); });
}

__global__ void __launch_bounds__(256) k_radius_unpack(const unsigned long long* __restrict__ keys, size_t n, int* __restrict__ idx, float* __restrict__ d2) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long k = keys[i];
    idx[i] = (int)(unsigned int)(k & 0xffffffffull);
    d2[i] = __uint_as_float((unsigned int)(k >> 32));
  }
}

}  // namespace ngk
