// Re-posing keyframes of the device-resident store after a loop closure, and reading a keyframe back (include/ngicp.h
// "moving keyframes").  The project's own definition: the reference keeps its keyframes on the host and has no counterpart.  Part of
// ngicp_api.hip's translation unit (included there behind every other kernel).
//
//   k_keyframe_move      ONE launch for a whole call, a thread per point of every listed keyframe.  The host uploads one table: per listed
//                        keyframe a KfMoveSeg {source and destination arrays, n, the float matrix, its 3x3 block in double}, per block a
//                        {segment, first point} pair - no block straddles two keyframes, so a block's segment is uniform and its 16 floats
//                        and 9 doubles come through scalar loads - and the six box words per keyframe and the flag word, initialised.
//                        A thread moves its point (transform_point_f, one 16-byte load and store, .w = the original index kept), rotates its
//                        covariance (rotate_sym, 48 bytes in and out as three 16-byte accesses) and leaves both at the SAME storage position
//                        in the destination arrays: 128 bytes of traffic per point.  The box: the coordinates' order-preserving integer
//                        images - the maxima's complemented, so that all six words are minima - reduced over the wave (shuffles) and the
//                        block (6 words of LDS per wave), then ONE atomicMin instruction per block (six lanes, the keyframe's six words).
//                        A block is 1024 threads because of that instruction: atomics execute at the memory side, about 20 ns each when
//                        they meet on one line, and with 256-thread blocks the 9,400 of a 12 x 100k store took 0.2 ms - seven times the
//                        streaming (measured).  Min and max do not depend on the order.  A coordinate that is not
//                        finite sets the flag word with an atomicOr (the box would hide a NaN).
//   k_keyframe_get_*     a keyframe's points / covariances into ORIGINAL point order by the index each stored point carries in .w: a
//                        keyframe that was moved has no permutation array (it is storage only, see DeviceCloud::storage_only).
// The kernels are templates on an unused int, as ngicp_scan_context.h's are: the compiler then emits them behind every kernel the
// library had, and the code object up to there is laid out as it was without this header.
#pragma once
#include <hip/hip_runtime.h>

#include "ngicp_cloudops.h"
#include "ngicp_math.h"

namespace ngk {

struct KfMoveSeg {
  const float4* src_pts;  // [n] {x, y, z, bitcast(original index)} in the keyframe's storage order
  float4* dst_pts;
  const double* src_cov;  // [n][6] in the same order
  double* dst_cov;
  float m[16];            // the matrix, column-major
  double R[9];            // its 3x3 block widened to double, row-major
  int n;
  int pad;
};
static_assert(sizeof(KfMoveSeg) % 16 == 0, "segments are laid out back to back in the table");

constexpr int kKfMoveBlock = 1024;

// float -> unsigned int, ascending with the float (-inf lowest, +inf highest; -0 below +0)
__host__ __device__ __forceinline__ unsigned int kf_order_key(float f) {
  unsigned int b;
  __builtin_memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ float kf_order_value(unsigned int k) {
  const unsigned int b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}

template <int>
__global__ void __launch_bounds__(kKfMoveBlock) k_keyframe_move(const KfMoveSeg* __restrict__ segs, const int2* __restrict__ blocks, unsigned int* box, unsigned int* flag) {
  __shared__ unsigned int lds[kKfMoveBlock / 64][6];
  const int2 be = blocks[blockIdx.x];
  const KfMoveSeg& sg = segs[be.x];
  const int i = be.y + (int)threadIdx.x;
  unsigned int key[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};  // min x y z, ~max x y z: neutral where the lane has no point
  bool bad = false;
  if (i < sg.n) {
    const float4 p = sg.src_pts[i];
    const float3 q = transform_point_f(sg.m, p.x, p.y, p.z);
    sg.dst_pts[i] = make_float4(q.x, q.y, q.z, p.w);
    const double2* c = reinterpret_cast<const double2*>(sg.src_cov + (size_t)i * 6);
    const double2 c0 = c[0], c1 = c[1], c2 = c[2];
    const double A[6] = {c0.x, c0.y, c1.x, c1.y, c2.x, c2.y};
    double o[6];
    rotate_sym(sg.R, A, o);
    double2* d = reinterpret_cast<double2*>(sg.dst_cov + (size_t)i * 6);
    d[0] = make_double2(o[0], o[1]);
    d[1] = make_double2(o[2], o[3]);
    d[2] = make_double2(o[4], o[5]);
    bad = !(isfinite(q.x) && isfinite(q.y) && isfinite(q.z));
    key[0] = kf_order_key(q.x); key[3] = ~key[0];
    key[1] = kf_order_key(q.y); key[4] = ~key[1];
    key[2] = kf_order_key(q.z); key[5] = ~key[2];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int d = 0; d < 6; ++d) key[d] = min(key[d], (unsigned int)__shfl_xor((int)key[d], off));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < 6; ++d) lds[wave][d] = key[d];
  }
  if (__any(bad) && lane == 0) atomicOr(flag, 1u);
  __syncthreads();
  if (threadIdx.x < 6) {
    const int d = threadIdx.x;
    unsigned int v = lds[0][d];
    for (int w = 1; w < kKfMoveBlock / 64; ++w) v = min(v, lds[w][d]);
    atomicMin(box + (size_t)be.x * 6 + d, v);
  }
}

// stored points -> packed xyz in ORIGINAL point order
template <int>
__global__ void __launch_bounds__(256) k_keyframe_get_points(const float4* __restrict__ pts, int n, float* __restrict__ out_xyz) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  float* d = out_xyz + (size_t)__float_as_int(p.w) * 3;
  d[0] = p.x; d[1] = p.y; d[2] = p.z;
}

// stored packed covariances -> N x 16 column-major 4x4 in ORIGINAL point order (k_covs_expand with the index taken from the point)
template <int>
__global__ void __launch_bounds__(256) k_keyframe_get_covs(const float4* __restrict__ pts, const double* __restrict__ covs6, int n, double* __restrict__ out16) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* c = covs6 + (size_t)i * 6;
  double* o = out16 + (size_t)__float_as_int(pts[i].w) * 16;
  o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = 0;
  o[4] = c[1]; o[5] = c[3]; o[6] = c[4]; o[7] = 0;
  o[8] = c[2]; o[9] = c[4]; o[10] = c[5]; o[11] = 0;
  o[12] = 0; o[13] = 0; o[14] = 0; o[15] = 0;
}

}  // namespace ngk

// ---- the host side ----
namespace {

using namespace ngk;

const ngicp::Keyframe& keyframe_of(const ngicp* h, int id) {
  if (id < 0 || (size_t)id >= h->keyframes.size()) throw ArgError{NGICP_ERR_ARG, "unknown keyframe id " + std::to_string(id)};
  return h->keyframes[(size_t)id];
}

// everything ngicp_keyframe_transform refuses before it enqueues anything
void check_keyframe_move_args(const ngicp* h, const int* ids, size_t n_ids, const float* T) {
  if (!ids || !T || n_ids == 0) throw ArgError{NGICP_ERR_ARG, "ngicp_keyframe_transform: null ids or transforms, or an empty list"};
  std::vector<std::pair<int, size_t>> seen(n_ids);
  for (size_t j = 0; j < n_ids; ++j) {
    (void)keyframe_of(h, ids[j]);
    seen[j] = {ids[j], j};
  }
  std::sort(seen.begin(), seen.end());
  for (size_t j = 1; j < n_ids; ++j)
    if (seen[j].first == seen[j - 1].first)
      throw ArgError{NGICP_ERR_ARG, "ngicp_keyframe_transform: keyframe " + std::to_string(seen[j].first) + " is listed twice, at positions " +
                                        std::to_string(seen[j - 1].second) + " and " + std::to_string(seen[j].second)};
  for (size_t j = 0; j < n_ids; ++j) {
    const float* m = T + j * 16;
    for (int e = 0; e < 16; ++e)
      if (!std::isfinite(m[e])) throw ArgError{NGICP_ERR_ARG, "ngicp_keyframe_transform: transform " + std::to_string(j) + " has an entry that is not finite"};
    if (m[3] != 0.f || m[7] != 0.f || m[11] != 0.f || m[15] != 1.f)
      throw ArgError{NGICP_ERR_ARG, "ngicp_keyframe_transform: the last row of transform " + std::to_string(j) + " is not (0, 0, 0, 1)"};
  }
}

}  // namespace

extern "C" {

int ngicp_keyframe_get(ngicp_t* h, int id, float* xyz_out, size_t out_stride_bytes, double* covs_n16, size_t* n_out) {
  return guarded(h, [&] {
    const ngicp::Keyframe& kf = keyframe_of(h, id);
    if (xyz_out && (out_stride_bytes < 12 || out_stride_bytes % 4)) throw ArgError{NGICP_ERR_ARG, "bad out_stride_bytes"};
    const size_t n = kf.cloud->n;
    if (n_out) *n_out = n;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (xyz_out) {
      h->out_xyz.ensure(n * 3 * sizeof(float));
      hipLaunchKernelGGL(k_keyframe_get_points<0>, grid, block, 0, h->stream, (const float4*)kf.cloud->pts(), (int)n, h->out_xyz.as<float>());
      download_xyz(h, n, xyz_out, out_stride_bytes);
    }
    if (covs_n16) {
      h->scratch16.ensure(n * 16 * sizeof(double));
      hipLaunchKernelGGL(k_keyframe_get_covs<0>, grid, block, 0, h->stream, (const float4*)kf.cloud->pts(), (const double*)kf.covs->as<double>(), (int)n, h->scratch16.as<double>());
      HIP_TRY(hipMemcpyAsync(covs_n16, h->scratch16.p, n * 16 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
      HIP_TRY(hipGetLastError());
    }
  });
}

int ngicp_keyframe_transform(ngicp_t* h, const int* ids, size_t n_ids, const float* T_colmajor_n16, int* submap_stale_out) {
  return guarded(h, [&] {
    check_keyframe_move_args(h, ids, n_ids, T_colmajor_n16);
    // fresh buffers for every listed keyframe (copy on move: the present ones may be a producer's source slot or another store's)
    struct Fresh {
      std::shared_ptr<DeviceCloud> cloud;
      std::shared_ptr<DevBuf> covs;
    };
    std::vector<Fresh> fresh(n_ids);
    size_t n_blocks = 0;
    for (size_t j = 0; j < n_ids; ++j) {
      const size_t n = h->keyframes[(size_t)ids[j]].cloud->n;
      Fresh& f = fresh[j];
      f.cloud = std::make_shared<DeviceCloud>();  // (not from the pool, and never into it: an index object there carries nine buffers, this one needs one)
      f.cloud->device = h->device;
      f.cloud->storage_only = true;  // no index is built: nothing searches a keyframe
      f.cloud->n = n;
      f.cloud->sorted.ensure((n + 2 * kSortedPad) * sizeof(float4));  // (the layout pts() expects; the pads stay unwritten, nobody walks this array)
      f.covs = acquire_buf(h, h->device, n * 6 * sizeof(double));
      n_blocks += (n + kKfMoveBlock - 1) / kKfMoveBlock;
    }
    if (n_blocks > (size_t)0x7fffffff) throw ArgError{NGICP_ERR_ARG, "ngicp_keyframe_transform: too many points in one call"};
    // the table: [n_ids] segments, [n_blocks] {segment, first point}, [n_ids][6] box words (all ones: three minima, three complemented maxima), the flag word
    const size_t off_blocks = n_ids * sizeof(KfMoveSeg), off_box = off_blocks + n_blocks * sizeof(int2), bytes = off_box + (n_ids * 6 + 1) * sizeof(unsigned int);
    h->kfm_host.resize(bytes);
    KfMoveSeg* segs = reinterpret_cast<KfMoveSeg*>(h->kfm_host.data());
    int2* blocks = reinterpret_cast<int2*>(h->kfm_host.data() + off_blocks);
    unsigned int* box = reinterpret_cast<unsigned int*>(h->kfm_host.data() + off_box);
    size_t b = 0;
    for (size_t j = 0; j < n_ids; ++j) {
      const ngicp::Keyframe& kf = h->keyframes[(size_t)ids[j]];
      const float* m = T_colmajor_n16 + j * 16;
      KfMoveSeg& s = segs[j];
      s.src_pts = kf.cloud->pts();
      s.dst_pts = fresh[j].cloud->pts();
      s.src_cov = kf.covs->as<double>();
      s.dst_cov = fresh[j].covs->as<double>();
      std::memcpy(s.m, m, sizeof(s.m));
      for (int row = 0; row < 3; ++row)
        for (int col = 0; col < 3; ++col) s.R[row * 3 + col] = (double)m[col * 4 + row];
      s.n = (int)kf.cloud->n;
      s.pad = 0;
      for (size_t first = 0; first < kf.cloud->n; first += kKfMoveBlock) blocks[b++] = make_int2((int)j, (int)first);
      for (int d = 0; d < 6; ++d) box[j * 6 + d] = 0xffffffffu;
    }
    box[n_ids * 6] = 0u;
    h->kfm_table.ensure(bytes);
    unsigned char* dev = h->kfm_table.as<unsigned char>();
    if (!h->ev_kfm_a) HIP_TRY(hipEventCreate(&h->ev_kfm_a));
    if (!h->ev_kfm_b) HIP_TRY(hipEventCreate(&h->ev_kfm_b));
    HIP_TRY(hipMemcpyAsync(dev, h->kfm_host.data(), bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->ev_kfm_a, h->stream));
    unsigned int* box_dev = reinterpret_cast<unsigned int*>(dev + off_box);
    hipLaunchKernelGGL(k_keyframe_move<0>, dim3((unsigned)n_blocks), dim3(kKfMoveBlock), 0, h->stream, reinterpret_cast<const KfMoveSeg*>(dev),
                       reinterpret_cast<const int2*>(dev + off_blocks), box_dev, box_dev + n_ids * 6);
    HIP_TRY(hipEventRecord(h->ev_kfm_b, h->stream));
    std::vector<unsigned int> back(n_ids * 6 + 1);
    HIP_TRY(hipMemcpyAsync(back.data(), box_dev, back.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // the call's one synchronisation; nothing of the store has changed yet
    HIP_TRY(hipGetLastError());
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev_kfm_a, h->ev_kfm_b) == hipSuccess) h->kfm_kernel_ms = ms;
    if (back[n_ids * 6]) throw ArgError{NGICP_ERR_ARG, "ngicp_keyframe_transform: a moved coordinate is not finite; no keyframe was changed"};
    // the swap
    bool stale = false;
    for (size_t j = 0; j < n_ids; ++j) {
      ngicp::Keyframe& kf = h->keyframes[(size_t)ids[j]];
      for (int d = 0; d < 3; ++d) {
        fresh[j].cloud->bb_min[d] = kf_order_value(back[j * 6 + d]);
        fresh[j].cloud->bb_max[d] = kf_order_value(~back[j * 6 + 3 + d]);
      }
      kf.cloud = fresh[j].cloud;
      kf.covs = fresh[j].covs;
      kf.part = nullptr;  // rebuilt lazily from the moved points and covariances
      stale = stale || std::find(h->submap_ids.begin(), h->submap_ids.end(), ids[j]) != h->submap_ids.end();
    }
    // the target keeps its buffers and stays what it was, voxel map included, but it is no longer "the submap of these keyframes": the
    // next ngicp_submap_set rebuilds, and a voxel map that has to be rebuilt meanwhile comes from the target's points, not from moved parts
    if (stale) h->submap_moved = true;
    if (submap_stale_out) *submap_stale_out = stale ? 1 : 0;
  });
}

int ngicp_keyframe_transform_kernel_ms(const ngicp_t* h, double* ms) {
  if (!h || !ms) return NGICP_ERR_ARG;
  *ms = h->kfm_kernel_ms;
  return NGICP_OK;
}

}  // extern "C"
