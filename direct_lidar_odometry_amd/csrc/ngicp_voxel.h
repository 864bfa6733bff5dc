// Voxelized GICP: the target reduced once to one Gaussian per occupied voxel, and a pass that finds a source point's
// correspondence with one table lookup instead of an exact 1-NN search.  The project's own definition (include/ngicp.h, "voxelized
// GICP"); no bit-fidelity to any outside library is claimed.
//
//   voxel of a float point p      ijk = floorf(p * inv_res) per axis, inv_res = 1.0f / (float)resolution: one float multiply, nothing
//                                 fused (the library is built with -ffp-contract=off), then floorf.  |i| >= 2^20 on any axis: no voxel
//                                 (a target with such a point is refused, a source point there has no correspondence), so that the
//                                 63-bit key (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20) orders the voxels by (iz, iy, ix).
//   voxel map of the target       per occupied voxel v, all sums in ascending ORIGINAL target index: n_v, mean_v = (sum (double)p_j) / n_v,
//                                 cov_v = (sum C_j) / n_v.  Voxels are numbered in ascending key.  Build: keys in original order ->
//                                 the filters' stable LSD radix sort (ngk_sort_pairs_u64) -> segment heads -> exclusive scan -> one
//                                 thread per voxel adds its segment in order.  Nothing depends on the order in which threads arrive.
//   lookup                        an open-addressing hash table (linear probing, load <= 1/2) from key to voxel number.  Every key is
//                                 inserted once, so WHERE a key lands depends on the order of arrival but WHAT a lookup returns does
//                                 not.  One 16-byte load per probe (about 1.5 probes per hit at this load in theory; not yet
//                                 measured), against the log2(100k) ~ 17 dependent loads of a binary search over 100k sorted keys.
//   k_vgicp_pass                  k_gicp_pass's role in the two-launch loop with the same mode bits (bit 0: error of the trial pose under
//                                 the previous pass's correspondences, bit 1: lookup + linearisation at the trial pose, bit 2: ignore
//                                 `done`), DIRECT1 rule: the source point at the float pose, q = ((c0 x + c1 y) + c2 z) + c3, corresponds
//                                 to the voxel of q if that voxel is occupied.  max_correspondence_distance is not consulted.
//                                 Terms (FP64): e = mean_v - T a, M = (cov_v + R C_a R^T)^-1; the matrix stored and used is n_v M, so the
//                                 tail and k_lm_solve are the exact path's.  A block takes 256 consecutive source points in the index's
//                                 sorted order and writes one row of 32 sums, reduced in a fixed order.
//   k_vgicp_pass_n<K>             the same pass for the neighbourhoods DIRECT7 (K = 7) and DIRECT27 (K = 27): slot s of a point whose voxel is
//                                 c corresponds to voxel c + off[s] if every component stays below 2^20 in magnitude (tested on the
//                                 integers, before a key is formed) and the voxel is occupied.  A point's terms are added in ascending slot.
//                                 K = 7: (0,0,0) (+1,0,0) (-1,0,0) (0,+1,0) (0,-1,0) (0,0,+1) (0,0,-1); K = 27: {-1,0,1}^3 in the key's order
//                                 (dx fastest, dz slowest; the centre is slot 13).  State is slot-major: corr[K][n_src], mahal[K][n_src][6].
//                                 k_vgicp_pass itself serves DIRECT1 and is not touched by any of this.
//   vgicp_pass_body / vgicp_pass_n_body<K>   what the two kernels do once they hold the state's pose and flags, as inlined functions:
//                                 k_vgicp_pass_batch<K> (ngicp_voxel_batch.h) runs the same bodies on a lane's record.
//   shared pieces, each defined once   voxel_cell / voxel_pack (-> voxel_key), voxel_probe_from (-> voxel_lookup, and the neighbourhoods'
//                                 probe continuation), voxel_segment_sums, voxel_table_insert and voxel_record_from_sums (every map's fill kernels), voxel_pass_begin
//                                 (the single kernels' head), voxel_block_row (a pass block's row); through ngicp_pass.h: load_pose (ngicp_lm.h),
//                                 transform_point_rowmajor_f (ngicp_search.h), lin_terms / err_term (ngicp_terms.h: the exact pass's K3 and its error leg).
//   merged voxel map              (a setting, off by default) the map of a submap from sums its keyframes carry:
//                                 k_voxel_part_fill (one keyframe's per-voxel sums, no division), k_voxel_part_gather (the parts' keys in
//                                 the order of the id list, value = global record position), the same stable sort and numbering, and
//                                 k_voxel_merge_fill (one thread per voxel adds its parts in list order and divides once).  The record
//                                 format, the numbering and the table are the map's above; the passes do not know the difference.
#pragma once
#include "ngicp_pass.h"

namespace ngk {

constexpr int kVoxBias = 1 << 20;       // |i| < 2^20 per axis
constexpr int kVoxKeyBits = 63;
constexpr unsigned long long kVoxEmpty = ~0ull;  // (no key has bit 63)
constexpr int kVoxBlock = 256;          // source points per block of k_vgicp_pass
constexpr int kVoxRec = 10;             // doubles per voxel record: mean 3, covariance {xx, xy, xz, yy, yz, zz}, count

// the cell of a float point; false when it has none (a component at or beyond 2^20 in magnitude, or a NaN coordinate)
__device__ __forceinline__ bool voxel_cell(float x, float y, float z, float inv_res, int& ix, int& iy, int& iz) {
  const float fx = floorf(x * inv_res), fy = floorf(y * inv_res), fz = floorf(z * inv_res);
  const float lim = 1048576.f;
  if (!(fx > -lim && fx < lim && fy > -lim && fy < lim && fz > -lim && fz < lim)) return false;  // (a NaN coordinate ends here too)
  ix = (int)fx, iy = (int)fy, iz = (int)fz;
  return true;
}

// the key of a cell whose components are all below 2^20 in magnitude
__device__ __forceinline__ unsigned long long voxel_pack(int ix, int iy, int iz) {
  return ((unsigned long long)(iz + kVoxBias) << 42) | ((unsigned long long)(iy + kVoxBias) << 21) | (unsigned long long)(ix + kVoxBias);
}

__device__ __forceinline__ bool voxel_key(float x, float y, float z, float inv_res, unsigned long long& key) {
  int ix, iy, iz;
  if (!voxel_cell(x, y, z, inv_res, ix, iy, iz)) return false;
  key = voxel_pack(ix, iy, iz);
  return true;
}

__device__ __forceinline__ unsigned int voxel_hash(unsigned long long k, unsigned int mask) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (unsigned int)k & mask;
}

// voxel number of `key`, or -1, probing from `slot` on.  The table always has empty slots (load <= 1/2): the probe sequence ends at a
// hit or at an empty slot, never at the loop's bound, which is there for form (mask + 1 slots from wherever the probe starts - the
// neighbourhoods' continuation, which starts one slot on, used to stop one slot sooner).  `table` is not __restrict__ here: the
// continuation never had it, and its caller stores to corr / LDS between probes.
__device__ __forceinline__ int voxel_probe_from(const ulonglong2* table, unsigned int mask, unsigned int slot, unsigned long long key, unsigned int& probes) {
  int v = -1;
  for (unsigned int t = 0; t <= mask; ++t) {
    const ulonglong2 e = table[slot];
    ++probes;
    if (e.x == key) { v = (int)e.y; break; }
    if (e.x == kVoxEmpty) break;
    slot = (slot + 1) & mask;
  }
  return v;
}

__device__ __forceinline__ int voxel_lookup(const ulonglong2* __restrict__ table, unsigned int mask, unsigned long long key, unsigned int& probes) {
  return voxel_probe_from(table, mask, voxel_hash(key, mask), key, probes);
}

// m, c = the sums of the points order[s .. e) and of their covariances, each started at 0.0 and added in segment order
__device__ __forceinline__ void voxel_segment_sums(const int* __restrict__ order, int s, int e, const float4* __restrict__ pts, const double* __restrict__ covs, double (&m)[3],
                                                   double (&c)[6]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) m[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = 0.0;
  for (int j = s; j < e; ++j) {
    const int p = order[j];
    const float4 q = pts[p];
    m[0] += (double)q.x;
    m[1] += (double)q.y;
    m[2] += (double)q.z;
    const double* C = covs + (size_t)p * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] += C[k];
  }
}

// {key, v} into the first free slot of key's probe sequence (keys are distinct and the table is at most half full: a free slot comes)
__device__ __forceinline__ void voxel_table_insert(ulonglong2* __restrict__ table, unsigned int mask, unsigned long long key, int v) {
  unsigned int slot = voxel_hash(key, mask);
  for (unsigned int t = 0; t <= mask; ++t) {
    const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long*>(&table[slot]), kVoxEmpty, key);
    if (prev == kVoxEmpty) {
      table[slot].y = (unsigned long long)v;
      break;
    }
    slot = (slot + 1) & mask;
  }
}

// the record of a voxel from its ten sums {S 3, C 6, n}: one division per entry, the count kept
__device__ __forceinline__ void voxel_record_from_sums(const double (&S)[kVoxRec], double* __restrict__ r) {
  const double cnt = S[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) r[k] = S[k] / cnt;
  r[9] = cnt;
}

// keys[o] / vals[o] for ORIGINAL target index o (the sort is stable: a voxel's points stay in ascending original index); vals = the
// point's position in the cell-sorted cloud, where its coordinates and covariance are.  *bad != 0: a point without a voxel.
__global__ void __launch_bounds__(256) k_voxel_map_keys(const float4* __restrict__ pts, int n, float inv_res, unsigned long long* __restrict__ keys, int* __restrict__ vals,
                                                         int* __restrict__ bad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const float4 p = pts[s];
  const int o = __float_as_int(p.w);
  unsigned long long key = 0;
  if (!voxel_key(p.x, p.y, p.z, inv_res, key)) atomicOr(bad, 1);
  keys[o] = key;
  vals[o] = s;
}

__global__ void __launch_bounds__(256) k_voxel_map_heads(const unsigned long long* __restrict__ keys, int n, int* __restrict__ head) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  head[j] = (j == 0 || keys[j] != keys[j - 1]) ? 1 : 0;
}

// seg_start[v] = first sorted position of voxel v (vox_of: the exclusive prefix of head, n + 1 entries); seg_start[n_vox] = n
__global__ void __launch_bounds__(256) k_voxel_map_starts(const int* __restrict__ head, const int* __restrict__ vox_of, int n, int* __restrict__ seg_start) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  if (head[j]) seg_start[vox_of[j]] = j;
  if (j == n - 1) seg_start[vox_of[n]] = n;
}

// one thread per voxel: its record (sums in segment order = ascending original index), its key, its entry in the hash table
__global__ void __launch_bounds__(256) k_voxel_map_fill(const unsigned long long* __restrict__ keys, const int* __restrict__ order, const int* __restrict__ seg_start, int n_vox,
                                                         const float4* __restrict__ pts, const double* __restrict__ covs, double* __restrict__ rec,
                                                         unsigned long long* __restrict__ vkeys, ulonglong2* __restrict__ table, unsigned int mask) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_vox) return;
  const int s = seg_start[v], e = seg_start[v + 1];
  double m[3], c[6];
  voxel_segment_sums(order, s, e, pts, covs, m, c);
  const double S[kVoxRec] = {m[0], m[1], m[2], c[0], c[1], c[2], c[3], c[4], c[5], (double)(e - s)};
  voxel_record_from_sums(S, rec + (size_t)v * kVoxRec);
  const unsigned long long key = keys[s];
  vkeys[v] = key;
  voxel_table_insert(table, mask, key, v);
}

// ---- a submap's map merged from per-keyframe voxel sums (include/ngicp.h "merged voxel map") -------------------------
// The voxel part of ONE keyframe: k_voxel_map_fill without the division and without the table.  A record holds the sums themselves,
// {sum (double)p 3, sum C 6, count}, each started at 0.0 and added in segment order = ascending original index inside the keyframe;
// the sorted key of voxel v goes to pkeys[v].
__global__ void __launch_bounds__(256) k_voxel_part_fill(const unsigned long long* __restrict__ keys, const int* __restrict__ order, const int* __restrict__ seg_start, int n_vox,
                                                          const float4* __restrict__ pts, const double* __restrict__ covs, double* __restrict__ rec,
                                                          unsigned long long* __restrict__ pkeys) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_vox) return;
  const int s = seg_start[v], e = seg_start[v + 1];
  double m[3], c[6];
  voxel_segment_sums(order, s, e, pts, covs, m, c);
  double* r = rec + (size_t)v * kVoxRec;
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = m[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) r[3 + k] = c[k];
  r[9] = (double)(e - s);
  pkeys[v] = keys[s];
}

// One listed keyframe's part keys into the gathered list at `offset`; the value is the GLOBAL part-record position offset + j (the
// stable sort then keeps a voxel's parts in the order of the id list).
__global__ void __launch_bounds__(256) k_voxel_part_gather(const unsigned long long* __restrict__ pkeys, int n, int offset, unsigned long long* __restrict__ keys,
                                                            int* __restrict__ vals) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  keys[offset + j] = pkeys[j];
  vals[offset + j] = offset + j;
}

// One thread per merged voxel: S = the first part record of its segment, then S + the next ones in segment order (ten doubles each,
// the count among them: exact), one division, the record, the key and the table entry exactly as k_voxel_map_fill writes them.
// part_off[0..m]: where each listed keyframe's records start in the gathered numbering (ascending, part_off[m] = the total);
// part_rec[i]: that keyframe's records.  An id listed twice has two entries.
__global__ void __launch_bounds__(256) k_voxel_merge_fill(const unsigned long long* __restrict__ keys, const int* __restrict__ order, const int* __restrict__ seg_start, int n_vox,
                                                           const int* __restrict__ part_off, const double* const* __restrict__ part_rec, int m, double* __restrict__ rec,
                                                           unsigned long long* __restrict__ vkeys, ulonglong2* __restrict__ table, unsigned int mask) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_vox) return;
  const int s = seg_start[v], e = seg_start[v + 1];
  double S[kVoxRec];
  for (int j = s; j < e; ++j) {
    const int g = order[j];
    int lo = 0, hi = m;  // the last i with part_off[i] <= g (parts are never empty: the offsets are strictly ascending)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (part_off[mid] <= g) lo = mid;
      else hi = mid;
    }
    const double* r = part_rec[lo] + (size_t)(g - part_off[lo]) * kVoxRec;
    if (j == s) {
#pragma unroll
      for (int k = 0; k < kVoxRec; ++k) S[k] = r[k];
    } else {
#pragma unroll
      for (int k = 0; k < kVoxRec; ++k) S[k] = S[k] + r[k];
    }
  }
  voxel_record_from_sums(S, rec + (size_t)v * kVoxRec);
  const unsigned long long key = keys[s];
  vkeys[v] = key;
  voxel_table_insert(table, mask, key, v);
}

struct VoxelPassArgs {
  const float4* src;        // source points in the index's sorted order, w = original index
  const double* cov_src;    // [n_src][6], the same order
  int n_src;
  const ulonglong2* table;  // {key, voxel number}; kVoxEmpty in free slots
  unsigned int mask;
  const double* rec;        // [n_vox][kVoxRec]
  int n_vox;
  float inv_res;
  int* corr[2];             // [n_src] voxel number or -1 (ping-pong halves, as PassArgs::tpt)
  double* mahal[2];         // [n_src][6] n_v (cov_v + R C_a R^T)^-1
  LmState* st;
  double* partials;         // [blocks][kNumSlots]
  int mode;                 // bit0: error part, bit1: linearise part, bit2: ignore st->done (test hooks)
  unsigned long long* t_first;  // device word: stamped by the first pass of an alignment (block 0), or null
  int nbr;                  // slots per source point (1, 7 or 27); k_vgicp_pass reads neither this nor slot_stride
  int slot_stride;          // k_vgicp_pass_n: corr / mahal are slot-major, slot s of point i at [s * slot_stride + i]
  // robust kernel (robust_term, ngicp_terms.h): read by the ROBUST instantiations only, which the host launches exactly when kind != NONE
  int robust_kind;
  double robust_c, robust_c2;
};

// The shared-memory arrays of a voxelized pass block (K = 1 has no `vs`).
struct VoxelPassLds {
  double red[4][16 * 30];
  double lds[4][kNumSlots];
  unsigned int cnt[4][2][64];
};

// A voxelized pass block's row of kNumSlots sums from its threads' sums and counters, in a fixed order: sixteen lanes at a time write a
// [16][30] tile, lane v adds column v top to bottom (the exact pass's R0); lanes 29 and 30 add the two counter columns; then the four
// waves in order.
__device__ __forceinline__ void voxel_block_row(const double (&acc)[kNumSums], const unsigned int nprobes, const unsigned int nvalid, VoxelPassLds& sh, double* partials) {
  double (&lds)[4][kNumSlots] = sh.lds;
  unsigned int (&cnt)[4][2][64] = sh.cnt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {
    double* rw = sh.red[wave];
    double out = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      wave_lds_sync();
      if ((lane >> 4) == q) {
#pragma unroll
        for (int v = 0; v < kNumSums; ++v) rw[(lane & 15) * 30 + v] = acc[v];
      }
      wave_lds_sync();
      if (lane < kNumSums)
        for (int l = 0; l < 16; ++l) out += rw[l * 30 + lane];
    }
    cnt[wave][0][lane] = nprobes;
    cnt[wave][1][lane] = nvalid;
    wave_lds_sync();
    if (lane >= kNumSums && lane < kNumSums + 2) {
      unsigned int sum = 0;
      for (int l = 0; l < 64; ++l) sum += cnt[wave][lane - kNumSums][l];
      out = (double)sum;
    }
    if (lane < kNumSlots) lds[wave][lane] = lane < kNumSums + 2 ? out : 0.0;
  }
  __syncthreads();
  if (threadIdx.x < kNumSlots) {
    const int v = threadIdx.x;
    partials[(size_t)blockIdx.x * kNumSlots + v] = ((lds[0][v] + lds[1][v]) + lds[2][v]) + lds[3][v];
  }
}

// One block of one DIRECT1 pass, from the pose on: everything k_vgicp_pass does once it holds the state's trial pose and flags.  The
// single kernel and k_vgicp_pass_batch<1> (ngicp_voxel_batch.h) both inline it: the same per-point statements, the same reduction, the
// same row - a lane of the batch comes out bit for bit as the single alignment.  A: VoxelPassArgs (the kernel's argument) or the same
// record seen through the constant address space (KernelVoxelPassArgs: a lane's record in device memory, read with scalar loads).
template <bool ROBUST = false, class A>
__device__ __forceinline__ void vgicp_pass_body(A& a, const PassPose& p, VoxelPassLds& sh) {
  const double (&R)[9] = p.R;
  const double (&t)[3] = p.t;
  const float (&Tf)[12] = p.Tf;
  const int cur = p.cur;
  const int nxt = cur ^ 1;
  const bool do_err = (a.mode & 1) && p.have_lin;
  const bool do_lin = (a.mode & 2);
  const int i = blockIdx.x * kVoxBlock + threadIdx.x;
  const bool mine = i < a.n_src;

  double acc[kNumSums];
#pragma unroll
  for (int v = 0; v < kNumSums; ++v) acc[v] = 0.0;
  unsigned int nprobes = 0, nvalid = 0;
  if (mine) {
    const float4 sp = a.src[i];
    const double ax = (double)sp.x, ay = (double)sp.y, az = (double)sp.z;
    const double tax = R[0] * ax + R[1] * ay + R[2] * az + t[0];  // T * a in FP64, as the exact pass
    const double tay = R[3] * ax + R[4] * ay + R[5] * az + t[1];
    const double taz = R[6] * ax + R[7] * ay + R[8] * az + t[2];
    if (do_err) {  // error of the trial pose under the previous pass's correspondences
      const int v_old = a.corr[cur][i];
      if ((unsigned int)v_old < (unsigned int)a.n_vox) {  // (-1: none)
        const double* mv = a.rec + (size_t)v_old * kVoxRec;
        if constexpr (ROBUST) acc[28] += err_term_robust(a.robust_kind, a.robust_c, a.robust_c2, mv[0] - tax, mv[1] - tay, mv[2] - taz, a.mahal[cur] + (size_t)i * 6);
        else acc[28] += err_term(mv[0] - tax, mv[1] - tay, mv[2] - taz, a.mahal[cur] + (size_t)i * 6);
      }
    }
    if (do_lin) {
      const float3 q = transform_point_rowmajor_f(Tf, sp.x, sp.y, sp.z);  // the float pose times the point, as the exact pass
      unsigned long long key = 0;
      int v = -1;
      if (voxel_key(q.x, q.y, q.z, a.inv_res, key)) v = voxel_lookup(a.table, a.mask, key, nprobes);
      a.corr[nxt][i] = v;
      if (v >= 0) {
        ++nvalid;
        const double* rv = a.rec + (size_t)v * kVoxRec;
        const double* CA = a.cov_src + (size_t)i * 6;
        double ca[6], rcr[6], M[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) ca[e] = CA[e];
        const double bx = rv[0], by = rv[1], bz = rv[2], nv = rv[9];
        rotate_sym(R, ca, rcr);
#pragma unroll
        for (int e = 0; e < 6; ++e) rcr[e] = rv[3 + e] + rcr[e];
        inv3_sym(rcr, M);
#pragma unroll
        for (int e = 0; e < 6; ++e) M[e] = nv * M[e];
        double* Mo = a.mahal[nxt] + (size_t)i * 6;
#pragma unroll
        for (int e = 0; e < 6; ++e) Mo[e] = M[e];
        // residual, Jacobian, normal equations: the exact pass's K3 with mean_v for the target point and n_v M for M
        if constexpr (ROBUST) lin_terms_robust(acc, a.robust_kind, a.robust_c, a.robust_c2, tax, tay, taz, bx - tax, by - tay, bz - taz, M);
        else lin_terms(acc, tax, tay, taz, bx - tax, by - tay, bz - taz, M);
      }
    }
  }
  voxel_block_row(acc, nprobes, nvalid, sh, a.partials);
}

typedef const VoxelPassArgs __attribute__((address_space(4))) KernelVoxelPassArgs;

// The head of the two single kernels: the state's pose and flags; false when the block has nothing to do (the alignment is done and
// mode bit 2 is not set); the first pass of an alignment stamps t_first.
__device__ __forceinline__ bool voxel_pass_begin(const VoxelPassArgs& a, PassPose& p) {
  const LmState* __restrict__ st = a.st;
  const int done_now = st->hot.done;
  load_pose(st, p);
  if (!(a.mode & 4) && done_now) return false;
  if (a.t_first && blockIdx.x == 0 && threadIdx.x == 0 && !p.have_lin) *a.t_first = __builtin_amdgcn_s_memrealtime();
  return true;
}

template <bool ROBUST = false>
__global__ void __launch_bounds__(kVoxBlock) k_vgicp_pass(VoxelPassArgs a) {
  __shared__ VoxelPassLds sh;
  PassPose p;
  if (!voxel_pass_begin(a, p)) return;
  vgicp_pass_body<ROBUST>(a, p, sh);
}

// voxel numbers (and float squared distances to (float)mean_v at the pose of the linearisation) back in ORIGINAL source order
__global__ void __launch_bounds__(256) k_voxel_corr_to_original(const int* __restrict__ corr, const float4* __restrict__ src, int n, const double* __restrict__ rec,
                                                                 int* __restrict__ out_corr, float* __restrict__ out_sqd, const float* __restrict__ lin_f) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 sp = src[i];
  const int o = __float_as_int(sp.w);
  const int v = corr[i];
  out_corr[o] = v;
  if (out_sqd) {
    float d = __builtin_inff();
    if (v >= 0) {
      const float3 q = transform_point_rowmajor_f(lin_f, sp.x, sp.y, sp.z);
      const double* mv = rec + (size_t)v * kVoxRec;
      d = sqdist(q.x, q.y, q.z, Xyz{(float)mv[0], (float)mv[1], (float)mv[2]});
    }
    out_sqd[o] = d;
  }
}

// ---- neighbourhoods (DIRECT7 / DIRECT27) ------------------------------------------------------------------------------------------
// component `axis` (0: x, 1: y, 2: z) of the offset of slot s
template <int K>
__host__ __device__ constexpr int vox_nbr_off(int s, int axis) {
  static_assert(K == 7 || K == 27, "DIRECT7 or DIRECT27");
  if (K == 27) return axis == 0 ? s % 3 - 1 : axis == 1 ? (s / 3) % 3 - 1 : s / 9 - 1;
  if (s == 0) return 0;
  return (s - 1) / 2 == axis ? (((s - 1) & 1) ? -1 : 1) : 0;  // slots 1..6: +x -x +y -y +z -z
}
template <int K>
__host__ __device__ constexpr int vox_nbr_centre() { return K == 27 ? 13 : 0; }

template <int K>
struct VoxelPassLdsN : VoxelPassLds {
  int vs[K][kVoxBlock];  // a thread's K voxel numbers between the lookups (unrolled) and the terms (a rolled loop): its own column
};

// vgicp_pass_body for the neighbourhoods: one block of one DIRECT7 / DIRECT27 pass from the pose on, inlined into k_vgicp_pass_n<K> and
// k_vgicp_pass_batch<K>.
template <int K, bool ROBUST = false, class A>
__device__ __forceinline__ void vgicp_pass_n_body(A& a, const PassPose& p, VoxelPassLdsN<K>& sh) {
  const double (&R)[9] = p.R;
  const double (&t)[3] = p.t;
  const float (&Tf)[12] = p.Tf;
  const int cur = p.cur;
  int (&vs)[K][kVoxBlock] = sh.vs;
  const int nxt = cur ^ 1;
  const bool do_err = (a.mode & 1) && p.have_lin;
  const bool do_lin = (a.mode & 2);
  const int i = blockIdx.x * kVoxBlock + threadIdx.x;
  const bool mine = i < a.n_src;
  const size_t stride = (size_t)a.slot_stride;

  double acc[kNumSums];
#pragma unroll
  for (int v = 0; v < kNumSums; ++v) acc[v] = 0.0;
  unsigned int nprobes = 0, nvalid = 0;
  if (mine) {
    const float4 sp = a.src[i];
    const double ax = (double)sp.x, ay = (double)sp.y, az = (double)sp.z;
    const double tax = R[0] * ax + R[1] * ay + R[2] * az + t[0];  // T * a in FP64, as the exact pass
    const double tay = R[3] * ax + R[4] * ay + R[5] * az + t[1];
    const double taz = R[6] * ax + R[7] * ay + R[8] * az + t[2];
    if (do_err) {  // error of the trial pose under the previous linearisation's voxels and matrices, slot after slot
      const int* __restrict__ co = a.corr[cur] + i;
      int vo[K];
#pragma unroll
      for (int s = 0; s < K; ++s) vo[s] = co[(size_t)s * stride];
#pragma unroll
      for (int s = 0; s < K; ++s) {
        if ((unsigned int)vo[s] < (unsigned int)a.n_vox) {  // (-1: none)
          const double* mv = a.rec + (size_t)vo[s] * kVoxRec;
          if constexpr (ROBUST) acc[28] += err_term_robust(a.robust_kind, a.robust_c, a.robust_c2, mv[0] - tax, mv[1] - tay, mv[2] - taz, a.mahal[cur] + ((size_t)s * stride + i) * 6);
          else acc[28] += err_term(mv[0] - tax, mv[1] - tay, mv[2] - taz, a.mahal[cur] + ((size_t)s * stride + i) * 6);
        }
      }
    }
    if (do_lin) {
      const float3 q = transform_point_rowmajor_f(Tf, sp.x, sp.y, sp.z);
      int cx, cy, cz;
      int* __restrict__ cn = a.corr[nxt] + i;
      if (!voxel_cell(q.x, q.y, q.z, a.inv_res, cx, cy, cz)) {  // (the centre has no cell: no slot has a voxel)
#pragma unroll
        for (int s = 0; s < K; ++s) cn[(size_t)s * stride] = -1;
      } else {
        // ---- the K lookups: every key first, and the first probe of each in flight before any is looked at ----
        unsigned long long key[K];
        ulonglong2 first[K];
        unsigned int in_range = 0;
#pragma unroll
        for (int s = 0; s < K; ++s) {
          const int nx = cx + vox_nbr_off<K>(s, 0), ny = cy + vox_nbr_off<K>(s, 1), nz = cz + vox_nbr_off<K>(s, 2);
          const bool ok = nx > -kVoxBias && nx < kVoxBias && ny > -kVoxBias && ny < kVoxBias && nz > -kVoxBias && nz < kVoxBias;
          key[s] = voxel_pack(nx, ny, nz);
          in_range |= ok ? (1u << s) : 0u;
          first[s] = a.table[ok ? voxel_hash(key[s], a.mask) : 0u];  // (a neighbour beyond the range: the load is neither used nor counted)
        }
#pragma unroll
        for (int s = 0; s < K; ++s) {
          int v = -1;
          if (in_range & (1u << s)) {
            ++nprobes;
            if (first[s].x == key[s]) {
              v = (int)first[s].y;
            } else if (first[s].x != kVoxEmpty) {  // the probe sequence goes on (the table always has empty slots: it ends)
              v = voxel_probe_from(a.table, a.mask, (voxel_hash(key[s], a.mask) + 1) & a.mask, key[s], nprobes);  // (rare: hashed again, not kept in a register for every slot)
            }
          }
          cn[(size_t)s * stride] = v;
          vs[s][threadIdx.x] = v;
        }
        // ---- the terms, slot after slot; R C_a R^T once per point ----
        const double* CA = a.cov_src + (size_t)i * 6;
        double ca[6], rcr[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) ca[e] = CA[e];
        rotate_sym(R, ca, rcr);
#pragma unroll 1
        for (int s = 0; s < K; ++s) {
          const int v = vs[s][threadIdx.x];
          if (v < 0) continue;
          ++nvalid;
          const double* rv = a.rec + (size_t)v * kVoxRec;
          double S[6], M[6];
          const double bx = rv[0], by = rv[1], bz = rv[2], nv = rv[9];
#pragma unroll
          for (int e = 0; e < 6; ++e) S[e] = rv[3 + e] + rcr[e];
          inv3_sym(S, M);
#pragma unroll
          for (int e = 0; e < 6; ++e) M[e] = nv * M[e];
          double* Mo = a.mahal[nxt] + ((size_t)s * stride + i) * 6;
#pragma unroll
          for (int e = 0; e < 6; ++e) Mo[e] = M[e];
          if constexpr (ROBUST) lin_terms_robust(acc, a.robust_kind, a.robust_c, a.robust_c2, tax, tay, taz, bx - tax, by - tay, bz - taz, M);
          else lin_terms(acc, tax, tay, taz, bx - tax, by - tay, bz - taz, M);
        }
      }
    }
  }
  voxel_block_row(acc, nprobes, nvalid, sh, a.partials);
}

template <int K, bool ROBUST = false>
__global__ void __launch_bounds__(kVoxBlock, 2) k_vgicp_pass_n(VoxelPassArgs a) {
  __shared__ VoxelPassLdsN<K> sh;
  PassPose p;
  if (!voxel_pass_begin(a, p)) return;
  vgicp_pass_n_body<K, ROBUST>(a, p, sh);
}

// the K voxel numbers of every source point, slot-major in sorted order -> row-major [n][K] in ORIGINAL source order
__global__ void __launch_bounds__(256) k_voxel_corr_n_to_original(const int* __restrict__ corr, const float4* __restrict__ src, int n, int K, int slot_stride,
                                                                   int* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int o = __float_as_int(src[i].w);
  for (int s = 0; s < K; ++s) out[(size_t)o * K + s] = corr[(size_t)s * slot_stride + i];
}

}  // namespace ngk
