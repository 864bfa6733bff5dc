// Correlative pose search against the voxel map (include/ngicp.h "voxel pose search"): an exhaustive search over a
// lattice of poses - B base poses times a window of whole-voxel shifts - in the manner of Olson's correlative scan matcher (ICRA 2009).
// A pose's score is the number of source points that land in occupied voxels: an integer, so the sums are order-free, atomics are
// deterministic and a host restates every result exactly (tests/_pose_search_model.py).  The project's own definition, and a query:
// nothing an alignment or a hook left on the handle is read or written.  Part of ngicp_api.hip's translation unit (included there
// behind every other kernel); the planning arithmetic is ngicp_pose_search_plan.h.
//
//   k_ps_map_box   the cell bounding box of the map: the table's slots grid-strided, a block's box in LDS (integer atomicMin / atomicMax),
//                  then at most six global atomics per block - none where the block cannot improve the box it reads.
//   k_ps_src_box   grid (blocks, poses): the cell bounding box of the source over every base pose, reduced the same way.
//   k_ps_occ_fill  one thread per table slot: an occupied key inside the grid sets its bit with a 64-bit atomicOr.
//   k_ps_score     grid (point chunks, poses), 256 threads.  The pose through the constant address space (scalar loads: uniform per
//                  block).  The chunk's cells are staged in LDS relative to the grid (first bit of the window, row y, row z; -1: the
//                  point has no cell or its window misses the grid).  Work items are (point, shift row (sy, sz)) pairs, the rows of one
//                  point on neighbouring lanes: their LDS counters lie a row apart (no two lanes of a point share an address) and their
//                  grid words a grid row apart.  An item reads its window of 2 ex + 1 bits from two words and adds 1 to the block's
//                  volume in LDS for every set bit; at the end the non-zero counters go to score[pose] with integer atomicAdd.  No
//                  floating point after the cell.
//   k_ps_topk      the first `top` keys of each segment of the input in ascending order; a key is (2^31 - 1 - score) << 32 | entry, so
//                  ascending keys are descending score, then ascending pose, then ascending shift index.  Level 0 reads the scores (a
//                  segment is a whole number of poses), further levels merge 64 segments' keys per block until one block is left: a
//                  single one-block pass over 2^24 entries would take `top` sweeps of all of them.
// The kernels are templates on an unused int, as ngicp_scan_context.h's are: the compiler then emits them behind every kernel the
// library had, and the code object up to there is laid out as it was without this header.
#pragma once
#include <hip/hip_runtime.h>

#include "ngicp_pose_search_plan.h"

namespace ngk {

constexpr int kPsBlock = 256;
constexpr int kPsChunk = 1024;            // source points per score block: 12 KB of staged cells beside the volume
constexpr int kPsBoxBlocks = 64;          // blocks per pose of k_ps_src_box, and of k_ps_map_box in all
constexpr int kPsPoseChunk = 16384;       // poses per launch (the grid's y limit is 65535)
constexpr int kPsTopSegMin = 4096;        // level 0 of the top-k: whole poses up to about this many entries per block
constexpr int kPsTopFan = 64;             // further levels: segments merged per block
constexpr unsigned long long kPsNoKey = ~0ull;

struct PsGrid {  // ngps::Plan as the kernels take it
  int org[3];
  int nx, ny, nz;
  int row_words;
};

struct PsScoreArgs {
  const float4* src;   // source points in the index's sorted order
  int n_src;
  const float* T;      // [poses][16] column-major, pose blockIdx.y of THIS launch first
  float inv_res;
  const unsigned long long* grid;
  PsGrid g;
  int ex, ey, ez;
  int n_shifts;
  int* score;          // [poses][n_shifts], this launch's first pose first
};

// a block's box in LDS -> the global one: the values only ever fall (lo) or rise (hi), so a block that cannot improve what it reads
// skips the atomic
__device__ __forceinline__ void ps_box_commit(const int* sh, int* box) {
  if (threadIdx.x < 6 && sh[0] <= sh[3]) {  // (an empty block box: nothing to say)
    const int a = threadIdx.x, v = sh[a];
    const int cur = __atomic_load_n(&box[a], __ATOMIC_RELAXED);
    if (a < 3) {
      if (v < cur) atomicMin(&box[a], v);
    } else if (v > cur) {
      atomicMax(&box[a], v);
    }
  }
}

__device__ __forceinline__ void ps_box_init(int* sh) {
  if (threadIdx.x < 6) sh[threadIdx.x] = threadIdx.x < 3 ? 0x7fffffff : (int)0x80000000;
  __syncthreads();
}

__device__ __forceinline__ void ps_box_add(int* sh, int ix, int iy, int iz) {
  // Most points change nothing: the plain reads keep the LDS atomics rare.  The reads race with other lanes' atomics, and that is safe
  // ONLY because each bound moves one way (lo falls, hi rises): a stale value is a looser bound, so it can cause an atomic that was not
  // needed, never skip one that was.  A bound that could move both ways would need the atomic unconditionally.
  if (ix < sh[0]) atomicMin(&sh[0], ix);
  if (iy < sh[1]) atomicMin(&sh[1], iy);
  if (iz < sh[2]) atomicMin(&sh[2], iz);
  if (ix > sh[3]) atomicMax(&sh[3], ix);
  if (iy > sh[4]) atomicMax(&sh[4], iy);
  if (iz > sh[5]) atomicMax(&sh[5], iz);
}

__device__ __forceinline__ void ps_key_cell(unsigned long long key, int& ix, int& iy, int& iz) {
  ix = (int)(key & 0x1fffffull) - kVoxBias;
  iy = (int)((key >> 21) & 0x1fffffull) - kVoxBias;
  iz = (int)((key >> 42) & 0x1fffffull) - kVoxBias;
}

// box[0..2] = min, box[3..5] = max of the cells of the table's keys
template <int U>
__global__ void __launch_bounds__(kPsBlock) k_ps_map_box(const ulonglong2* __restrict__ table, unsigned int slots, int* __restrict__ box) {
  __shared__ int sh[6];
  ps_box_init(sh);
  for (unsigned int i = blockIdx.x * kPsBlock + threadIdx.x; i < slots; i += gridDim.x * kPsBlock) {
    const unsigned long long key = table[i].x;
    if (key == kVoxEmpty) continue;
    int ix, iy, iz;
    ps_key_cell(key, ix, iy, iz);
    ps_box_add(sh, ix, iy, iz);
  }
  __syncthreads();
  ps_box_commit(sh, box);
}

typedef const float __attribute__((address_space(4))) PsPoseFloat;

// pose blockIdx.y of T as the passes' row-major 3x4 float pose
__device__ __forceinline__ void ps_load_pose(const float* T, float (&Tf)[12]) {
  PsPoseFloat* Tm = (PsPoseFloat*)(unsigned long long)(T + (size_t)blockIdx.y * 16);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) Tf[r * 4 + c] = Tm[c * 4 + r];
}

// box[0..5] over c_b(p) of every point that has a cell, every pose of the launch
template <int U>
__global__ void __launch_bounds__(kPsBlock) k_ps_src_box(const float4* __restrict__ src, int n, const float* T, float inv_res, int* __restrict__ box) {
  __shared__ int sh[6];
  float Tf[12];
  ps_load_pose(T, Tf);
  ps_box_init(sh);
  for (int i = blockIdx.x * kPsBlock + threadIdx.x; i < n; i += gridDim.x * kPsBlock) {
    const float4 sp = src[i];
    const float3 q = transform_point_rowmajor_f(Tf, sp.x, sp.y, sp.z);
    int cx, cy, cz;
    if (voxel_cell(q.x, q.y, q.z, inv_res, cx, cy, cz)) ps_box_add(sh, cx, cy, cz);
  }
  __syncthreads();
  ps_box_commit(sh, box);
}

// grid words are zero on entry; guards and the bits past nx stay zero
template <int U>
__global__ void __launch_bounds__(kPsBlock) k_ps_occ_fill(const ulonglong2* __restrict__ table, unsigned int slots, PsGrid g, unsigned long long* __restrict__ grid) {
  const unsigned int i = blockIdx.x * kPsBlock + threadIdx.x;
  if (i >= slots) return;
  const unsigned long long key = table[i].x;
  if (key == kVoxEmpty) return;
  int ix, iy, iz;
  ps_key_cell(key, ix, iy, iz);
  const int lx = ix - g.org[0], ly = iy - g.org[1], lz = iz - g.org[2];
  if ((unsigned int)lx >= (unsigned int)g.nx || (unsigned int)ly >= (unsigned int)g.ny || (unsigned int)lz >= (unsigned int)g.nz) return;
  atomicOr(&grid[((size_t)lz * g.ny + ly) * g.row_words + 1 + (lx >> 6)], 1ull << (lx & 63));
}

template <int U>
__global__ void __launch_bounds__(kPsBlock) k_ps_score(PsScoreArgs a) {
  extern __shared__ int ps_lds[];  // [n_shifts] the block's volume, then three rows of kPsChunk: window start bit, row y, row z
  int* vol = ps_lds;
  int* px = ps_lds + a.n_shifts;
  int* py = px + kPsChunk;
  int* pz = py + kPsChunk;
  float Tf[12];
  ps_load_pose(a.T, Tf);
  for (int s = threadIdx.x; s < a.n_shifts; s += kPsBlock) vol[s] = 0;
  const int first = blockIdx.x * kPsChunk;
  const int np = min(kPsChunk, a.n_src - first);
  for (int j = threadIdx.x; j < np; j += kPsBlock) {
    const float4 sp = a.src[first + j];
    const float3 q = transform_point_rowmajor_f(Tf, sp.x, sp.y, sp.z);
    int cx, cy, cz, pos = -1;
    if (voxel_cell(q.x, q.y, q.z, a.inv_res, cx, cy, cz)) {
      const int l = cx - a.ex - a.g.org[0];  // local x of the window's first bit (|.| < 2^22)
      if (l + 2 * a.ex >= 0 && l <= a.g.nx - 1) {
        pos = l + 64;  // the front guard word: >= 64 - 2 ex >= 2
        py[j] = cy - a.g.org[1];
        pz[j] = cz - a.g.org[2];
      }
    }
    px[j] = pos;
  }
  __syncthreads();
  const int wx = 2 * a.ex + 1, wy = 2 * a.ey + 1;
  const unsigned int rows = (unsigned int)(wy * (2 * a.ez + 1));
  const unsigned int items = (unsigned int)np * rows;  // <= 1024 * 945
  const unsigned long long mask = (1ull << wx) - 1ull;  // (wx <= 63)
  for (unsigned int it = threadIdx.x; it < items; it += kPsBlock) {
    const unsigned int p = it / rows, r = it - p * rows;
    const int pos = px[p];
    if (pos < 0) continue;
    const int rz = (int)(r / (unsigned int)wy), ry = (int)r - rz * wy;
    const int ly = py[p] + ry - a.ey, lz = pz[p] + rz - a.ez;
    if ((unsigned int)ly >= (unsigned int)a.g.ny || (unsigned int)lz >= (unsigned int)a.g.nz) continue;  // the row leaves the grid: nothing there
    const unsigned long long* __restrict__ row = a.grid + ((size_t)lz * a.g.ny + ly) * a.g.row_words;
    const int wi = pos >> 6, sh = pos & 63;  // wi + 1 <= ceil(nx / 64) + 1 = row_words - 1
    const unsigned long long lo = row[wi], hi = row[wi + 1];
    unsigned long long w = ((lo >> sh) | (sh ? hi << (64 - sh) : 0ull)) & mask;
    int* v = vol + r * wx;
    while (w) {
      atomicAdd(&v[__builtin_ctzll(w)], 1);
      w &= w - 1ull;
    }
  }
  __syncthreads();
  int* out = a.score + (size_t)blockIdx.y * a.n_shifts;
  for (int s = threadIdx.x; s < a.n_shifts; s += kPsBlock) {
    const int c = vol[s];
    if (c) atomicAdd(&out[s], c);
  }
}

__device__ __forceinline__ unsigned long long ps_key(int score, unsigned int entry) {
  return ((unsigned long long)(unsigned int)(0x7fffffff - score) << 32) | entry;  // (score <= n_src < 2^31 - 1: no real key is 0 or kPsNoKey)
}

// block g: out[g * top + 0 .. top) = the `top` smallest keys of entries [g * seg, min(n, (g + 1) * seg)) in ascending order, kPsNoKey where
// the segment has fewer.  SCORES: the input is the score array and entry i's key is ps_key(score[i], i); else the input holds keys.
// One round per place, as k_sc_topk: every thread scans its strided share for the smallest key above the previous winner (keys are
// distinct), the block reduces.
template <int U, bool SCORES>
__global__ void __launch_bounds__(kPsBlock) k_ps_topk(const void* __restrict__ in, unsigned int n, unsigned int seg, int top, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long wkey[kPsBlock / 64];
  const unsigned int lo = blockIdx.x * seg, hi = min(n, lo + seg);
  unsigned long long prev = 0ull;
  for (int place = 0; place < top; ++place) {
    unsigned long long best = kPsNoKey;
    for (unsigned int i = lo + threadIdx.x; i < hi; i += kPsBlock) {
      unsigned long long key;
      if constexpr (SCORES) key = ps_key(static_cast<const int*>(in)[i], i);
      else key = static_cast<const unsigned long long*>(in)[i];
      if (key > prev && key < best) best = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long ok = __shfl_xor(best, o);
      if (ok < best) best = ok;
    }
    if ((threadIdx.x & 63) == 0) wkey[threadIdx.x >> 6] = best;
    __syncthreads();
    best = wkey[0];
#pragma unroll
    for (int w = 1; w < kPsBlock / 64; ++w)
      if (wkey[w] < best) best = wkey[w];
    __syncthreads();  // (the words are rewritten in the next round)
    if (threadIdx.x == 0) out[(size_t)blockIdx.x * top + place] = best;
    if (best == kPsNoKey) {  // the segment is exhausted (uniform): the remaining places hold no key
      for (int q = place + 1 + threadIdx.x; q < top; q += kPsBlock) out[(size_t)blockIdx.x * top + q] = kPsNoKey;
      break;
    }
    prev = best;
  }
}

}  // namespace ngk

// ---- the host side ----
namespace {

using namespace ngk;

size_t ps_score_lds(int n_shifts) { return ((size_t)n_shifts + 3 * (size_t)kPsChunk) * sizeof(int); }

void ps_events(ngicp* h) {
  for (hipEvent_t& e : h->ps.ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
}

// what the last search's volume was computed against: compared when the volume is asked for
struct PsMapStamp {
  bool rolling;
  long long gen;
};
PsMapStamp ps_map_stamp(const ngicp* h) {
  const bool rolling = rolling_active(h);
  return PsMapStamp{rolling, rolling ? h->roll.gen : h->voxel_builds};
}

void pose_search_impl(ngicp* h, size_t n_poses, const float* T_colmajor, int ex, int ey, int ez, int top_k, int* pose_out, int* shift_out_xyz, int* score_out, size_t* n_out) {
  const std::string e = "ngicp_voxel_pose_search";
  ngicp::PoseSearch& ps = h->ps;
  if (!(h->voxel_res > 0.0)) throw ArgError{NGICP_ERR_STATE, e + ": the voxelized mode is off (ngicp_set_voxel_resolution)"};
  if (n_poses == 0) throw ArgError{NGICP_ERR_ARG, e + ": n_poses is 0"};
  if (!T_colmajor) throw ArgError{NGICP_ERR_ARG, e + ": null transforms"};
  if (ngps::shift_count(ex, ey, ez) < 0) throw ArgError{NGICP_ERR_ARG, e + ": the extents must satisfy 0 <= ex, ey <= 31, 0 <= ez <= 7 and (2 ex + 1)(2 ey + 1)(2 ez + 1) <= 12288"};
  if (top_k < 1 || top_k > ngps::kMaxTopK) throw ArgError{NGICP_ERR_ARG, e + ": top_k must be 1..64"};
  if (n_poses > (size_t)ngps::kMaxEntries || !ngps::entries_ok((long long)n_poses, ex, ey, ez))
    throw ArgError{NGICP_ERR_ARG, e + ": n_poses times the number of shifts must not exceed 2^24 (tile a larger window over more calls)"};
  if (!pose_out || !shift_out_xyz || !score_out || !n_out) throw ArgError{NGICP_ERR_ARG, e + ": null output"};
  ensure_slot_ready(h, h->src, "source");
  const VoxelMapView vm = ensure_voxel_map(h);
  DeviceCloud& S = *h->src.dev;
  const int np = (int)S.n;
  const int n_shifts = (int)ngps::shift_count(ex, ey, ez);
  const size_t B = n_poses, entries = B * (size_t)n_shifts;
  const float inv_res = 1.0f / (float)h->voxel_res;
  const unsigned int slots = vm.mask + 1u;
  ps_events(h);
  ps.T.ensure(B * 16 * sizeof(float));
  ps.box.ensure(12 * sizeof(int));
  const float* T_dev = ps.T.as<float>();
  int* box_dev = ps.box.as<int>();
  // ---- the two boxes, one read-back ----
  static const int kNoBox[12] = {0x7fffffff, 0x7fffffff, 0x7fffffff, (int)0x80000000, (int)0x80000000, (int)0x80000000,
                                 0x7fffffff, 0x7fffffff, 0x7fffffff, (int)0x80000000, (int)0x80000000, (int)0x80000000};
  int box[12];
  try {
    HIP_TRY(hipMemcpyAsync(ps.T.p, T_colmajor, B * 16 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(box_dev, kNoBox, sizeof(kNoBox), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(ps.ev[0], h->stream));
    hipLaunchKernelGGL((k_ps_map_box<0>), dim3((unsigned)std::min<size_t>((slots + kPsBlock - 1) / kPsBlock, (size_t)kPsBoxBlocks)), dim3(kPsBlock), 0, h->stream, vm.table, slots, box_dev);
    if (np > 0) {
      const unsigned bx = (unsigned)std::min<size_t>(((size_t)np + kPsBlock - 1) / kPsBlock, (size_t)kPsBoxBlocks);
      for (size_t at = 0; at < B; at += kPsPoseChunk) {
        const size_t m = std::min<size_t>(kPsPoseChunk, B - at);
        hipLaunchKernelGGL((k_ps_src_box<0>), dim3(bx, (unsigned)m), dim3(kPsBlock), 0, h->stream, (const float4*)S.pts(), np, T_dev + at * 16, inv_res, box_dev + 6);
      }
    }
    HIP_TRY(hipEventRecord(ps.ev[1], h->stream));
    HIP_TRY(hipMemcpyAsync(box, box_dev, sizeof(box), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
  } catch (...) {
    (void)hipStreamSynchronize(h->stream);  // the upload of the caller's poses may still be pending: it must not outlive them
    throw;
  }
  const ngps::Box map_box{{box[0], box[1], box[2]}, {box[3], box[4], box[5]}}, src_box{{box[6], box[7], box[8]}, {box[9], box[10], box[11]}};
  const ngps::Plan plan = ngps::plan_grid(map_box, src_box, ex, ey, ez);
  if (plan.too_large) throw ArgError{NGICP_ERR_ARG, e + ": the occupancy grid over the map and the window would exceed 256 MiB (search a smaller region, or a coarser map)"};
  // ---- from here on the last search's volume is replaced ----
  const int top_n = (int)std::min<size_t>((size_t)top_k, entries);
  const size_t per_seg = std::max<size_t>(1, (size_t)kPsTopSegMin / (size_t)n_shifts);  // poses per level-0 segment
  const size_t nseg0 = (B + per_seg - 1) / per_seg, nseg1 = (nseg0 + kPsTopFan - 1) / kPsTopFan;
  ps.valid = false;
  ps.score.ensure(entries * sizeof(int));
  ps.cand.ensure((nseg0 + nseg1) * (size_t)top_n * sizeof(unsigned long long));
  if (!plan.empty) ps.grid.ensure(plan.bytes);
  int* score = ps.score.as<int>();
  unsigned long long* cand[2] = {ps.cand.as<unsigned long long>(), ps.cand.as<unsigned long long>() + nseg0 * (size_t)top_n};
  HIP_TRY(hipEventRecord(ps.ev[2], h->stream));
  HIP_TRY(hipMemsetAsync(score, 0, entries * sizeof(int), h->stream));
  if (!plan.empty) {  // (an empty intersection: every score is 0 and no score kernel runs)
    PsGrid g{{plan.org[0], plan.org[1], plan.org[2]}, plan.nx, plan.ny, plan.nz, plan.row_words};
    HIP_TRY(hipMemsetAsync(ps.grid.p, 0, plan.bytes, h->stream));
    hipLaunchKernelGGL((k_ps_occ_fill<0>), dim3((slots + kPsBlock - 1) / kPsBlock), dim3(kPsBlock), 0, h->stream, vm.table, slots, g, ps.grid.as<unsigned long long>());
    PsScoreArgs a{};
    a.src = S.pts();
    a.n_src = np;
    a.inv_res = inv_res;
    a.grid = ps.grid.as<unsigned long long>();
    a.g = g;
    a.ex = ex, a.ey = ey, a.ez = ez;
    a.n_shifts = n_shifts;
    const unsigned chunks = (unsigned)((np + kPsChunk - 1) / kPsChunk);
    for (size_t at = 0; at < B && chunks; at += kPsPoseChunk) {
      const size_t m = std::min<size_t>(kPsPoseChunk, B - at);
      a.T = T_dev + at * 16;
      a.score = score + at * (size_t)n_shifts;
      hipLaunchKernelGGL((k_ps_score<0>), dim3(chunks, (unsigned)m), dim3(kPsBlock), ps_score_lds(n_shifts), h->stream, a);
    }
  }
  // ---- top-k: per group of poses, then 64 segments per block until one block is left ----
  hipLaunchKernelGGL((k_ps_topk<0, true>), dim3((unsigned)nseg0), dim3(kPsBlock), 0, h->stream, (const void*)score, (unsigned int)entries, (unsigned int)(per_seg * (size_t)n_shifts), top_n, cand[0]);
  int cur = 0;
  for (size_t nseg = nseg0; nseg > 1;) {
    const size_t next = (nseg + kPsTopFan - 1) / kPsTopFan;
    hipLaunchKernelGGL((k_ps_topk<0, false>), dim3((unsigned)next), dim3(kPsBlock), 0, h->stream, (const void*)cand[cur], (unsigned int)(nseg * (size_t)top_n), (unsigned int)(kPsTopFan * top_n), top_n,
                       cand[cur ^ 1]);
    cur ^= 1;
    nseg = next;
  }
  HIP_TRY(hipEventRecord(ps.ev[3], h->stream));
  unsigned long long keys[ngps::kMaxTopK];
  HIP_TRY(hipMemcpyAsync(keys, cand[cur], (size_t)top_n * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));  // the one read-back of the results
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  float ms_a = 0.f, ms_b = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms_a, ps.ev[0], ps.ev[1]));
  HIP_TRY(hipEventElapsedTime(&ms_b, ps.ev[2], ps.ev[3]));
  ps.kernel_ms = (double)ms_a + (double)ms_b;
  for (int i = 0; i < top_n; ++i) {
    const unsigned int entry = (unsigned int)(keys[i] & 0xffffffffull);
    if (keys[i] == kPsNoKey || entry >= entries) throw ArgError{NGICP_ERR_HIP, e + ": inconsistent top-k record"};
    pose_out[i] = (int)(entry / (unsigned int)n_shifts);
    ngps::shift_of_index((int)(entry % (unsigned int)n_shifts), ex, ey, ez, shift_out_xyz + 3 * i);
    score_out[i] = 0x7fffffff - (int)(keys[i] >> 32);
  }
  *n_out = (size_t)top_n;
  ps.entries = entries;
  ps.stamp_rolling = ps_map_stamp(h).rolling;
  ps.stamp_gen = ps_map_stamp(h).gen;
  ps.valid = true;
}

void pose_search_scores_impl(ngicp* h, int* out, size_t capacity) {
  const std::string e = "ngicp_voxel_pose_search_scores";
  ngicp::PoseSearch& ps = h->ps;
  if (!ps.valid) throw ArgError{NGICP_ERR_STATE, e + ": no search has been run"};
  const PsMapStamp now = ps_map_stamp(h);
  if (!(h->voxel_res > 0.0) || now.rolling != ps.stamp_rolling || now.gen != ps.stamp_gen || (!now.rolling && !voxel_map_current(h)))
    throw ArgError{NGICP_ERR_STATE, e + ": the voxel map has changed since the last search"};
  if (!out) throw ArgError{NGICP_ERR_ARG, e + ": null output"};
  if (capacity < ps.entries) throw ArgError{NGICP_ERR_ARG, e + ": the output holds fewer than n_poses times the number of shifts entries"};
  HIP_TRY(hipMemcpyAsync(out, ps.score.p, ps.entries * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
}

}  // namespace

extern "C" {

int ngicp_voxel_pose_search(ngicp_t* h, size_t n_poses, const float* T_n16_colmajor, int ex, int ey, int ez, int top_k, int* pose_out, int* shift_out_xyz, int* score_out, size_t* n_out) {
  return guarded(h, [&] { pose_search_impl(h, n_poses, T_n16_colmajor, ex, ey, ez, top_k, pose_out, shift_out_xyz, score_out, n_out); });
}

int ngicp_voxel_pose_search_scores(ngicp_t* h, int* out, size_t capacity) {
  return guarded(h, [&] { pose_search_scores_impl(h, out, capacity); });
}

int ngicp_voxel_pose_search_kernel_ms(const ngicp_t* h, double* ms) {
  if (!h || !ms) return NGICP_ERR_ARG;
  *ms = h->ps.kernel_ms;
  return NGICP_OK;
}

}  // extern "C"
