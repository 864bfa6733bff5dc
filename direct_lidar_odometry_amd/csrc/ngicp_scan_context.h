// Scan Context place recognition (include/ngicp.h "scan context"): a polar height descriptor of a scan in the manner of
// Kim & Kim (IROS 2018), a device-resident database of them and an exhaustive match over every column shift.  The project's own
// definition - no fidelity to any outside implementation is claimed - and a query: nothing an alignment or a hook left on the handle is
// read or written.  Part of ngicp_api.hip's translation unit (included there behind every other kernel).
//
//   k_sc_build   one thread per point (grid-stride), 256 threads.  The two tables (ring edges squared, sector boundary directions) and the
//                block's descriptor sit in LDS.  A point's cell is a pair of COUNTS (edges passed, boundaries passed), v = z + z0; an LDS
//                atomicMax on the unsigned bit pattern of v when v > 0 (non-negative floats order as unsigned integers), then one global
//                atomicMax per non-zero LDS cell.  A maximum does not depend on order: the descriptor is deterministic.
//   k_sc_norms   block d, thread j < S: the norm of column j of descriptor d, summed in double with r ascending, the root corrected to
//                the correctly rounded one (sc_sqrt_rn) so that a host restates it with an IEEE sqrt.
//   k_sc_match   one wave per candidate, blockDim.x / 64 candidates per block (the launch sizes the block so that the LDS fits).  The
//                query's floats and norms are staged once per block, a candidate's per wave.  Lane k < S owns shift k and walks j and r
//                in the defined order in plain FP64 (no MFMA: its fused accumulation is not the defined sum); it reads C[r][(j + k) mod S],
//                consecutive lanes consecutive words, and Q[r][j] as a broadcast.  The minimum over the lanes is a shuffle reduction on
//                (d, k), the tie going to the smaller k.
//   k_sc_topk    one block: the first top_k of the ascending (distance, id) ranking, one round per place - every thread scans its strided
//                share for the smallest key above the previous winner, the block reduces.  The distances are not modified.
// The kernels are templates on an unused int, as k_voxel_fitness_final is: the compiler then emits them behind every kernel the library
// had, and the code object up to there - the pass kernels among it - is laid out as it was without this header.
#pragma once
#include <hip/hip_runtime.h>

namespace ngk {

constexpr int kScMaxRings = 64, kScMaxSectors = 64, kScMaxTopK = 64;
constexpr int kScBuildBlock = 256;
constexpr int kScBuildMaxBlocks = 256;          // one per CU: a block's non-zero cells cost one global atomic each
constexpr int kScTabE2 = kScMaxRings + 1;       // floats of the device table: E2[0..R], then b[0..S/2) as (x, y) pairs at kScTabE2
constexpr int kScTabFloats = kScTabE2 + kScMaxSectors;
constexpr int kScTopBlock = 256;
constexpr int kScLdsBudget = 64 * 1024;         // what a match block may take

struct ScTopRec {  // what ngicp_scan_context_match reads back, in one copy
  double dist[kScMaxTopK];
  int id[kScMaxTopK];
  int shift[kScMaxTopK];
};

// LDS bytes of a match block of `waves` waves: (1 + waves) descriptors of R * S floats, then (1 + waves) norm rows of S doubles
__host__ __device__ inline size_t sc_match_lds(int R, int S, int waves) {
  return (size_t)(1 + waves) * ((size_t)R * S * sizeof(float) + (size_t)S * sizeof(double));
}

// the correctly rounded root of x >= 0 (0 and +inf map to themselves): the device's root, then at most two steps against the rounding
// boundaries in exact arithmetic.  With s a candidate, u the gap to its upper neighbour and e = x - s^2 (exact in an fma: a multiple of
// ulp(s)^2 below 2^53 of them), x lies above the midpoint (s + u/2) iff e > s u, and below (s - w/2), w the gap to the lower neighbour,
// iff e <= -s w: e and s u are multiples of u^2 / 4 apart from the u^2 / 4 of the square itself, and no root of a double is a midpoint.
__device__ __forceinline__ double sc_sqrt_rn(double x) {
  if (!(x > 0.0) || x > 1.7e308) return x;
  double s = sqrt(x);
#pragma unroll 1
  for (int it = 0; it < 2; ++it) {
    const double e = __fma_rn(-s, s, x);
    const double up = __longlong_as_double(__double_as_longlong(s) + 1), dn = __longlong_as_double(__double_as_longlong(s) - 1);
    if (e > __dmul_rn(s, __dsub_rn(up, s))) s = up;
    else if (e <= -__dmul_rn(s, __dsub_rn(s, dn))) s = dn;
    else break;
  }
  return s;
}

template <int U>
__global__ void __launch_bounds__(kScBuildBlock) k_sc_build(const float4* __restrict__ pts, int n, const float* __restrict__ tab, int R, int S, float z0,
                                                            unsigned int* __restrict__ desc) {
  __shared__ unsigned int cell[kScMaxRings * kScMaxSectors];
  __shared__ float t[kScTabFloats];
  const int cells = R * S, half = S / 2;
  for (int c = threadIdx.x; c < cells; c += kScBuildBlock) cell[c] = 0u;
  for (int c = threadIdx.x; c < kScTabFloats; c += kScBuildBlock) t[c] = tab[c];
  __syncthreads();
  const float E2R = t[R];
  for (long long i = (long long)blockIdx.x * kScBuildBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kScBuildBlock) {
    const float4 p = pts[i];
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;
    const float r2 = __fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y));
    if (!(r2 < E2R)) continue;
    int ring = 0;
    for (int k = 1; k < R; ++k) ring += r2 >= t[k] ? 1 : 0;
    const bool low = p.y < 0.f || (p.y == 0.f && p.x < 0.f);
    const float xs = low ? -p.x : p.x, ys = low ? -p.y : p.y;
    int sector = low ? half : 0;
    for (int k = 1; k < half; ++k) {
      const float bx = t[kScTabE2 + 2 * k], by = t[kScTabE2 + 2 * k + 1];
      sector += __fsub_rn(__fmul_rn(bx, ys), __fmul_rn(by, xs)) >= 0.f ? 1 : 0;
    }
    const float v = __fadd_rn(p.z, z0);
    if (v > 0.f) atomicMax(&cell[ring * S + sector], __float_as_uint(v));  // ring < R and sector < S: both are counts of at most R - 1 and S - 1
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cells; c += kScBuildBlock) {
    const unsigned int b = cell[c];
    if (b) atomicMax(&desc[c], b);
  }
}

// block d: norms[d][j] of desc[d][R][S]
template <int U>
__global__ void __launch_bounds__(kScMaxSectors) k_sc_norms(const float* __restrict__ desc, int R, int S, double* __restrict__ norms) {
  const int j = threadIdx.x;
  if (j >= S) return;
  const float* __restrict__ D = desc + (size_t)blockIdx.x * R * S;
  double s = 0.0;
  for (int r = 0; r < R; ++r) {
    const double a = (double)D[r * S + j];
    s = __dadd_rn(s, __dmul_rn(a, a));
  }
  norms[(size_t)blockIdx.x * S + j] = sc_sqrt_rn(s);
}

// candidates [first, first + n) of the database against the query: dist[g], shift[g] for candidate first + g
template <int U>
__global__ void __launch_bounds__(256) k_sc_match(const float* __restrict__ q_desc, const double* __restrict__ q_norm, const float* __restrict__ db_desc,
                                                  const double* __restrict__ db_norm, int first, int n, int R, int S, double* __restrict__ dist,
                                                  int* __restrict__ shift) {
  extern __shared__ double sc_lds[];  // norms first (8-byte aligned), the floats behind them
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cells = R * S;
  double* nq = sc_lds;
  double* nc = sc_lds + (size_t)(1 + wave) * S;
  float* Q = reinterpret_cast<float*>(sc_lds + (size_t)(1 + waves) * S);
  float* Cw = Q + (size_t)(1 + wave) * cells;
  for (int c = threadIdx.x; c < cells; c += blockDim.x) Q[c] = q_desc[c];
  for (int c = threadIdx.x; c < S; c += blockDim.x) nq[c] = q_norm[c];
  const int g = blockIdx.x * waves + wave;
  const bool live = g < n;  // uniform per wave
  if (live) {
    const float* __restrict__ C = db_desc + (size_t)(first + g) * cells;
    const double* __restrict__ N = db_norm + (size_t)(first + g) * S;
    for (int c = lane; c < cells; c += 64) Cw[c] = C[c];
    for (int c = lane; c < S; c += 64) nc[c] = N[c];
  }
  __syncthreads();
  if (!live) return;
  double d = __builtin_inf();
  int k = lane;
  if (lane < S) {
    double sum = 0.0;
    int m = 0, jp = lane;  // jp = (j + k) mod S
    for (int j = 0; j < S; ++j) {
      const double a = nq[j], b = nc[jp];
      if (a > 0.0 && b > 0.0) {
        double dot = 0.0;
        for (int r = 0; r < R; ++r) dot = __dadd_rn(dot, __dmul_rn((double)Q[r * S + j], (double)Cw[r * S + jp]));
        sum = __dadd_rn(sum, __ddiv_rn(dot, __dmul_rn(a, b)));
        ++m;
      }
      jp = jp + 1 == S ? 0 : jp + 1;
    }
    d = m ? __dsub_rn(1.0, __ddiv_rn(sum, (double)m)) : 1.0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // lane l takes the better of l and l + o: lane 0 ends with the scan's answer
    const double od = __shfl_down(d, o);
    const int ok = __shfl_down(k, o);
    if (lane + o < 64 && (od < d || (od == d && ok < k))) {
      d = od;
      k = ok;
    }
  }
  if (lane == 0) {
    dist[g] = d;
    shift[g] = k;
  }
}

// a double as an unsigned key of the same order (-x < +x, a NaN behind +inf)
__device__ __forceinline__ unsigned long long sc_key(double d) {
  if (d != d) return ~0ull;
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// out = the first `top` (<= n, <= kScMaxTopK) entries of dist[0..n) in ascending (distance, index) order; ids are first + index
template <int U>
__global__ void __launch_bounds__(kScTopBlock) k_sc_topk(const double* __restrict__ dist, const int* __restrict__ shift, int first, int n, int top,
                                                         ScTopRec* __restrict__ out) {
  __shared__ unsigned long long wkey[kScTopBlock / 64];
  __shared__ int widx[kScTopBlock / 64];
  unsigned long long prev_key = 0ull;
  int prev_idx = -1;  // (every real pair is above {0, -1})
  for (int place = 0; place < top; ++place) {
    unsigned long long best_key = ~0ull;
    int best_idx = 0x7fffffff;  // (no candidate; a real pair is below it: idx < n)
    for (int i = threadIdx.x; i < n; i += kScTopBlock) {
      const unsigned long long key = sc_key(dist[i]);
      const bool above = key > prev_key || (key == prev_key && i > prev_idx);
      if (above && (key < best_key || (key == best_key && i < best_idx))) {
        best_key = key;
        best_idx = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long ok = __shfl_xor(best_key, o);
      const int oi = __shfl_xor(best_idx, o);
      if (ok < best_key || (ok == best_key && oi < best_idx)) {
        best_key = ok;
        best_idx = oi;
      }
    }
    if ((threadIdx.x & 63) == 0) {
      wkey[threadIdx.x >> 6] = best_key;
      widx[threadIdx.x >> 6] = best_idx;
    }
    __syncthreads();
    best_key = wkey[0];
    best_idx = widx[0];
#pragma unroll
    for (int w = 1; w < kScTopBlock / 64; ++w) {
      if (wkey[w] < best_key || (wkey[w] == best_key && widx[w] < best_idx)) {
        best_key = wkey[w];
        best_idx = widx[w];
      }
    }
    __syncthreads();  // (the words are rewritten in the next round)
    if (best_idx >= n) break;  // cannot happen for top <= n; uniform
    if (threadIdx.x == 0) {
      out->dist[place] = dist[best_idx];
      out->id[place] = first + best_idx;
      out->shift[place] = shift[best_idx];
    }
    prev_key = best_key;
    prev_idx = best_idx;
  }
}

}  // namespace ngk

// ---- the host side: parameters and tables, the database, the entries ----
namespace {

using namespace ngk;

void sc_check_params(int R, int S, float L, float z0) {
  if (R < 1 || R > kScMaxRings) throw ArgError{NGICP_ERR_ARG, "scan context: n_rings must be 1..64"};
  if (S < 2 || S > kScMaxSectors || (S & 1)) throw ArgError{NGICP_ERR_ARG, "scan context: n_sectors must be even and 2..64"};
  if (!(L > 0.f) || !std::isfinite(L)) throw ArgError{NGICP_ERR_ARG, "scan context: max_radius must be positive and finite"};
  if (!std::isfinite(z0)) throw ArgError{NGICP_ERR_ARG, "scan context: z_offset must be finite"};
}

// the host tables of the parameters in force: tab[0..R] = E2, tab[kScTabE2 + 2 k] = b_k
void sc_make_tables(ngicp::ScanContext& sc) {
  if (sc.tab_valid) return;
  sc.tab.assign(kScTabFloats, 0.f);
  for (int k = 0; k <= sc.R; ++k) {
    const float e = (float)((double)sc.L * k / sc.R);
    sc.tab[k] = e * e;
  }
  const double two_pi = 6.283185307179586476925286766559;
  for (int k = 0; k < sc.S / 2; ++k) {
    sc.tab[kScTabE2 + 2 * k] = (float)std::cos(two_pi * k / sc.S);
    sc.tab[kScTabE2 + 2 * k + 1] = (float)std::sin(two_pi * k / sc.S);
  }
  sc.tab_valid = true;
  sc.tab_on_device = false;
}

const float* sc_device_tables(ngicp* h) {
  ngicp::ScanContext& sc = h->sc;
  sc_make_tables(sc);
  sc.tab_dev.ensure(kScTabFloats * sizeof(float));
  if (!sc.tab_on_device) {
    HIP_TRY(hipMemcpyAsync(sc.tab_dev.p, sc.tab.data(), kScTabFloats * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // (the host vector may be rebuilt by the next parameter change)
    sc.tab_on_device = true;
  }
  return sc.tab_dev.as<float>();
}

void sc_events(ngicp* h) {
  if (!h->sc.ev_a) HIP_TRY(hipEventCreate(&h->sc.ev_a));
  if (!h->sc.ev_b) HIP_TRY(hipEventCreate(&h->sc.ev_b));
}

// the cloud of a slot, as ngicp_range_select defines `which` and with its state errors
void sc_slot_cloud(ngicp* h, int which, const float4*& pts, size_t& n) {
  if (which < 0 || which > 2) throw ArgError{NGICP_ERR_ARG, "scan context: which must be 0 (source), 1 (target) or 2 (preprocessed scan)"};
  if (which == 2) {
    if (!h->filt_out || h->filt_n <= 0) throw ArgError{NGICP_ERR_STATE, "no preprocessed cloud: call ngicp_preprocess_scan first"};
    pts = h->filt_out;
    n = (size_t)h->filt_n;
  } else {
    DeviceCloud& C = query_cloud(h, which);
    pts = C.pts();
    n = C.n;
  }
  if (n == 0) throw ArgError{NGICP_ERR_STATE, "the cloud is empty"};
  if (n > (size_t)0x7fffff00) throw ArgError{NGICP_ERR_ARG, "cloud too large for int counters"};
}

void sc_check_host_descriptor(const ngicp::ScanContext& sc, const float* desc) {
  if (!desc) throw ArgError{NGICP_ERR_ARG, "scan context: null descriptor"};
  const size_t cells = (size_t)sc.R * sc.S;
  for (size_t c = 0; c < cells; ++c)
    if (!(std::isfinite(desc[c]) && desc[c] >= 0.f)) throw ArgError{NGICP_ERR_ARG, "scan context: a descriptor's cells must be finite and >= 0"};
}

// enqueue: the descriptor of a slot's cloud -> desc_dev (R * S floats) and, with norm_dev, its column norms
void sc_enqueue_build(ngicp* h, const float4* pts, size_t n, float* desc_dev, double* norm_dev) {
  ngicp::ScanContext& sc = h->sc;
  const float* tab = sc_device_tables(h);
  const size_t cells = (size_t)sc.R * sc.S;
  HIP_TRY(hipMemsetAsync(desc_dev, 0, cells * sizeof(float), h->stream));
  const int blocks = (int)std::min<size_t>((n + kScBuildBlock - 1) / kScBuildBlock, (size_t)kScBuildMaxBlocks);
  hipLaunchKernelGGL((k_sc_build<0>), dim3((unsigned)blocks), dim3(kScBuildBlock), 0, h->stream, pts, (int)n, tab, sc.R, sc.S, sc.z0, reinterpret_cast<unsigned int*>(desc_dev));
  if (norm_dev) hipLaunchKernelGGL((k_sc_norms<0>), dim3(1), dim3(kScMaxSectors), 0, h->stream, (const float*)desc_dev, sc.R, sc.S, norm_dev);
}

void sc_timing_done(ngicp* h) {  // after the stream has been synchronised behind ev_b
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->sc.ev_a, h->sc.ev_b));
  h->sc.kernel_ms = ms;
}

// room for one more entry: the per-entry arrays double, their contents kept
void sc_reserve_one(ngicp* h) {
  ngicp::ScanContext& sc = h->sc;
  if (sc.count < sc.cap) return;
  const size_t cap = std::max<size_t>(64, sc.cap * 2);
  const size_t cells = (size_t)sc.R * sc.S;
  DevBuf nd, nn;
  nd.ensure(cap * cells * sizeof(float));
  nn.ensure(cap * sc.S * sizeof(double));
  if (sc.count) {
    HIP_TRY(hipMemcpyAsync(nd.p, sc.db_desc.p, sc.count * cells * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(nn.p, sc.db_norm.p, sc.count * sc.S * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // (the old arrays are freed when nd / nn leave this scope)
  }
  std::swap(nd.p, sc.db_desc.p);
  std::swap(nd.cap, sc.db_desc.cap);
  std::swap(nn.p, sc.db_norm.p);
  std::swap(nn.cap, sc.db_norm.cap);
  sc.cap = cap;
}

void sc_add_impl(ngicp* h, int which, const float* host_desc, int* id_out) {
  ngicp::ScanContext& sc = h->sc;
  if (!id_out) throw ArgError{NGICP_ERR_ARG, "scan context: null id"};
  const float4* pts = nullptr;
  size_t n = 0;
  if (host_desc) sc_check_host_descriptor(sc, host_desc);
  else sc_slot_cloud(h, which, pts, n);
  if (sc.count >= (size_t)0x7fffffff) throw ArgError{NGICP_ERR_ARG, "scan context: the database is full"};
  sc_events(h);
  sc_reserve_one(h);
  const size_t cells = (size_t)sc.R * sc.S;
  float* d = sc.db_desc.as<float>() + sc.count * cells;
  double* nr = sc.db_norm.as<double>() + sc.count * sc.S;
  if (host_desc) {
    HIP_TRY(hipMemcpyAsync(d, host_desc, cells * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(sc.ev_a, h->stream));
    hipLaunchKernelGGL((k_sc_norms<0>), dim3(1), dim3(kScMaxSectors), 0, h->stream, (const float*)d, sc.R, sc.S, nr);
  } else {
    sc_device_tables(h);
    HIP_TRY(hipEventRecord(sc.ev_a, h->stream));
    sc_enqueue_build(h, pts, n, d, nr);
  }
  HIP_TRY(hipEventRecord(sc.ev_b, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  sc_timing_done(h);
  *id_out = (int)sc.count;
  ++sc.count;
}

void sc_compute_impl(ngicp* h, int which, float* desc_out) {
  ngicp::ScanContext& sc = h->sc;
  if (!desc_out) throw ArgError{NGICP_ERR_ARG, "scan context: null output"};
  const float4* pts = nullptr;
  size_t n = 0;
  sc_slot_cloud(h, which, pts, n);
  sc_events(h);
  const size_t cells = (size_t)sc.R * sc.S;
  sc.q_desc.ensure(cells * sizeof(float));
  sc_device_tables(h);
  HIP_TRY(hipEventRecord(sc.ev_a, h->stream));
  sc_enqueue_build(h, pts, n, sc.q_desc.as<float>(), nullptr);
  HIP_TRY(hipEventRecord(sc.ev_b, h->stream));
  HIP_TRY(hipMemcpyAsync(desc_out, sc.q_desc.p, cells * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  sc_timing_done(h);
}

// distances (top_k == 0) or match: everything passed in is checked before anything is enqueued
void sc_query_impl(ngicp* h, int which, const float* host_desc, long long id_begin, long long id_end, int top_k, int* ids_out, double* dist_out, int* shift_out,
                   size_t* n_out) {
  ngicp::ScanContext& sc = h->sc;
  const bool match = ids_out || n_out || top_k;
  if (which == -1 ? !host_desc : host_desc != nullptr) throw ArgError{NGICP_ERR_ARG, "scan context: the query is a slot (which 0..2, no descriptor) or a descriptor (which -1)"};
  if (id_begin < 0 || id_begin > id_end || id_end > (long long)sc.count) throw ArgError{NGICP_ERR_ARG, "scan context: the range must satisfy 0 <= id_begin <= id_end <= count"};
  if (match && (top_k < 1 || top_k > kScMaxTopK)) throw ArgError{NGICP_ERR_ARG, "scan context: top_k must be 1..64"};
  if (match && !n_out) throw ArgError{NGICP_ERR_ARG, "scan context: null n_out"};
  const size_t n = (size_t)(id_end - id_begin);
  if (n && (!dist_out || !shift_out || (match && !ids_out))) throw ArgError{NGICP_ERR_ARG, "scan context: null output"};
  const float4* pts = nullptr;
  size_t np = 0;
  if (host_desc) sc_check_host_descriptor(sc, host_desc);
  else sc_slot_cloud(h, which, pts, np);
  if (match) *n_out = 0;
  if (n == 0) return;
  sc_events(h);
  const size_t cells = (size_t)sc.R * sc.S;
  sc.q_desc.ensure(cells * sizeof(float));
  sc.q_norm.ensure(sc.S * sizeof(double));
  const size_t dist_bytes = n * sizeof(double);
  sc.res.ensure(dist_bytes + n * sizeof(int) + sizeof(ScTopRec) + 16);
  double* dist = sc.res.as<double>();
  int* shift = reinterpret_cast<int*>(sc.res.as<unsigned char>() + dist_bytes);
  ScTopRec* top = reinterpret_cast<ScTopRec*>(sc.res.as<unsigned char>() + ((dist_bytes + n * sizeof(int) + 7) & ~(size_t)7));
  if (host_desc) {
    HIP_TRY(hipMemcpyAsync(sc.q_desc.p, host_desc, cells * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(sc.ev_a, h->stream));
    hipLaunchKernelGGL((k_sc_norms<0>), dim3(1), dim3(kScMaxSectors), 0, h->stream, (const float*)sc.q_desc.as<float>(), sc.R, sc.S, sc.q_norm.as<double>());
  } else {
    sc_device_tables(h);
    HIP_TRY(hipEventRecord(sc.ev_a, h->stream));
    sc_enqueue_build(h, pts, np, sc.q_desc.as<float>(), sc.q_norm.as<double>());
  }
  int waves = 4;
  while (waves > 1 && sc_match_lds(sc.R, sc.S, waves) > (size_t)kScLdsBudget) --waves;  // (64 x 64: two waves, 49.5 KB)
  const unsigned grid = (unsigned)((n + waves - 1) / waves);
  hipLaunchKernelGGL((k_sc_match<0>), dim3(grid), dim3(64 * waves), sc_match_lds(sc.R, sc.S, waves), h->stream, (const float*)sc.q_desc.as<float>(),
                     (const double*)sc.q_norm.as<double>(), (const float*)sc.db_desc.as<float>(), (const double*)sc.db_norm.as<double>(), (int)id_begin, (int)n, sc.R,
                     sc.S, dist, shift);
  const int top_n = match ? (int)std::min<size_t>((size_t)top_k, n) : 0;
  if (match) hipLaunchKernelGGL((k_sc_topk<0>), dim3(1), dim3(kScTopBlock), 0, h->stream, (const double*)dist, (const int*)shift, (int)id_begin, (int)n, top_n, top);
  HIP_TRY(hipEventRecord(sc.ev_b, h->stream));
  if (match) {
    ScTopRec rec;
    HIP_TRY(hipMemcpyAsync(&rec, top, sizeof(rec), hipMemcpyDeviceToHost, h->stream));  // the one read-back
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < top_n; ++i) {
      ids_out[i] = rec.id[i];
      dist_out[i] = rec.dist[i];
      shift_out[i] = rec.shift[i];
    }
    *n_out = (size_t)top_n;
  } else {
    std::vector<unsigned char> host(dist_bytes + n * sizeof(int));
    HIP_TRY(hipMemcpyAsync(host.data(), sc.res.p, host.size(), hipMemcpyDeviceToHost, h->stream));  // the one read-back
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    std::memcpy(dist_out, host.data(), dist_bytes);
    std::memcpy(shift_out, host.data() + dist_bytes, n * sizeof(int));
  }
  sc_timing_done(h);
}

}  // namespace

extern "C" {

int ngicp_scan_context_set_params(ngicp_t* h, int n_rings, int n_sectors, float max_radius, float z_offset) {
  return guarded(h, [&] {
    sc_check_params(n_rings, n_sectors, max_radius, z_offset);
    ngicp::ScanContext& sc = h->sc;
    if (n_rings == sc.R && n_sectors == sc.S && max_radius == sc.L && z_offset == sc.z0) return;
    sc.R = n_rings;
    sc.S = n_sectors;
    sc.L = max_radius;
    sc.z0 = z_offset;
    sc.tab_valid = false;
    sc.count = 0;  // descriptors of another layout or scale cannot be compared: the database starts again
    // the arrays are kept and cut anew for the new entry size
    sc.cap = std::min(sc.db_desc.cap / ((size_t)sc.R * sc.S * sizeof(float)), sc.db_norm.cap / ((size_t)sc.S * sizeof(double)));
  });
}

int ngicp_scan_context_get_params(const ngicp_t* h, int* n_rings, int* n_sectors, float* max_radius, float* z_offset) {
  if (!h) return NGICP_ERR_ARG;
  if (n_rings) *n_rings = h->sc.R;
  if (n_sectors) *n_sectors = h->sc.S;
  if (max_radius) *max_radius = h->sc.L;
  if (z_offset) *z_offset = h->sc.z0;
  return NGICP_OK;
}

int ngicp_scan_context_tables(ngicp_t* h, float* E2_out, float* b_out) {
  return guarded(h, [&] {
    if (!E2_out || !b_out) throw ArgError{NGICP_ERR_ARG, "scan context: null output"};
    sc_make_tables(h->sc);
    std::memcpy(E2_out, h->sc.tab.data(), (size_t)(h->sc.R + 1) * sizeof(float));
    std::memcpy(b_out, h->sc.tab.data() + kScTabE2, (size_t)h->sc.S * sizeof(float));
  });
}

int ngicp_scan_context_compute(ngicp_t* h, int which, float* desc_out) {
  return guarded(h, [&] { sc_compute_impl(h, which, desc_out); });
}

int ngicp_scan_context_add(ngicp_t* h, int which, int* id) {
  return guarded(h, [&] { sc_add_impl(h, which, nullptr, id); });
}

int ngicp_scan_context_add_descriptor(ngicp_t* h, const float* desc, int* id) {
  return guarded(h, [&] {
    if (!desc) throw ArgError{NGICP_ERR_ARG, "scan context: null descriptor"};
    sc_add_impl(h, -1, desc, id);
  });
}

int ngicp_scan_context_count(const ngicp_t* h, size_t* n) {
  if (!h || !n) return NGICP_ERR_ARG;
  *n = h->sc.count;
  return NGICP_OK;
}

int ngicp_scan_context_get(ngicp_t* h, int id, float* desc_out) {
  return guarded(h, [&] {
    if (!desc_out) throw ArgError{NGICP_ERR_ARG, "scan context: null output"};
    if (id < 0 || (size_t)id >= h->sc.count) throw ArgError{NGICP_ERR_ARG, "scan context: no such entry"};
    const size_t cells = (size_t)h->sc.R * h->sc.S;
    HIP_TRY(hipMemcpyAsync(desc_out, h->sc.db_desc.as<float>() + (size_t)id * cells, cells * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  });
}

int ngicp_scan_context_clear(ngicp_t* h) {
  return guarded(h, [&] { h->sc.count = 0; });
}

int ngicp_scan_context_distances(ngicp_t* h, int which_or_minus1, const float* desc_or_null, size_t id_begin, size_t id_end, double* dist_out, int* shift_out) {
  return guarded(h, [&] {
    if (id_begin > (size_t)0x7fffffff || id_end > (size_t)0x7fffffff) throw ArgError{NGICP_ERR_ARG, "scan context: the range must satisfy 0 <= id_begin <= id_end <= count"};
    sc_query_impl(h, which_or_minus1, desc_or_null, (long long)id_begin, (long long)id_end, 0, nullptr, dist_out, shift_out, nullptr);
  });
}

int ngicp_scan_context_match(ngicp_t* h, int which_or_minus1, const float* desc_or_null, size_t id_begin, size_t id_end, int top_k, int* ids_out, double* dist_out,
                             int* shift_out, size_t* n_out) {
  return guarded(h, [&] {
    if (!n_out) throw ArgError{NGICP_ERR_ARG, "scan context: null n_out"};
    if (top_k < 1 || top_k > kScMaxTopK) throw ArgError{NGICP_ERR_ARG, "scan context: top_k must be 1..64"};
    if (id_begin > (size_t)0x7fffffff || id_end > (size_t)0x7fffffff) throw ArgError{NGICP_ERR_ARG, "scan context: the range must satisfy 0 <= id_begin <= id_end <= count"};
    sc_query_impl(h, which_or_minus1, desc_or_null, (long long)id_begin, (long long)id_end, top_k, ids_out, dist_out, shift_out, n_out);
  });
}

int ngicp_scan_context_kernel_ms(const ngicp_t* h, double* ms) {
  if (!h || !ms) return NGICP_ERR_ARG;
  *ms = h->sc.kernel_ms;
  return NGICP_OK;
}

}  // extern "C"
