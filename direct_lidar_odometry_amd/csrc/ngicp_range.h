// The range median of a cloud on the device: dlo::OdomNode::computeSpaciousness (src/dlo/odom.cc:990-1010) without the download.
//
//   range      d = (float) sqrt((double)x * x + (double)y * y + (double)z * z), the sum taken left to right in double: what odom.cc:996
//              computes (pow(float, 2) promotes to double, the square of a float is exact in double, std::sqrt(double) is correctly
//              rounded, the result is narrowed to float).  d >= 0, so the float bit patterns order like unsigned integers; a NaN range
//              takes the key 0xffffffff and so sorts after +inf.
//   select     the element of 0-based rank r of the n ranges in ascending order, by an exact radix select over the 32-bit key in three
//              rounds of 11 + 11 + 10 bits.  Per round k_range_hist recomputes every point's key from its float4 (no key buffer), drops
//              the points whose higher bits differ from the prefix chosen so far, counts the digit of the others in a per-block LDS
//              histogram and adds the block's non-zero bins to one global histogram; k_range_pick (one block) finds the bin that holds
//              the remaining rank and writes {prefix, remaining rank} for the next round.  After the third round the prefix is the answer.
//
// Everything accumulated is a 32-bit integer count (one bin can hold the whole cloud), so the result does not depend on the order of
// the atomics: no floating-point reduction anywhere in this path.
//
// Exactness of d (range_key).  Nothing is assumed about the device's FP64 sqrt beyond "within a float step of the root": the candidate
// (float)sqrt(s) is corrected against the float rounding boundaries in exact double arithmetic.  Between two neighbouring floats
// g < g' lies the midpoint m (25 significant bits, never a power of two except 2^-150, which no root comes near: s is 0 or >= 2^-298),
// and with u = ulp_double(m), t = m u, e = s - m^2:
//     e >   t   <=>  the correctly rounded double root is above m   ->  d >= g'
//     e <= -t   <=>  it is below m                                  ->  d <= g
//     otherwise      it IS m (the double rounding of the reference) ->  the tie goes to the even one of g, g'
// because RN(sqrt(s)) = m  <=>  (m - u/2)^2 < s < (m + u/2)^2  <=>  -t + u^2/4 < e < t + u^2/4, and e and t are multiples of u^2.
// m^2 has 50 bits and is exact; e is exact by Sterbenz' lemma (m^2 is within a factor (1 + 2^-22)^2 of s); t is a power-of-two scaling.
#pragma once
#include <hip/hip_runtime.h>

namespace ngk {

constexpr int kRangeBins = 2048;    // 11 bits; the last round uses the lower 1024
constexpr int kRangeBlock = 256;
constexpr int kRangeMaxBlocks = 256;  // one per CU: a block's non-zero bins cost one global atomic each
constexpr unsigned int kRangeNanKey = 0xffffffffu;

struct RangeRec {
  unsigned int prefix;  // the key bits chosen so far (the lower ones 0)
  int rank;             // rank of the answer among the points that share the prefix
  unsigned int value;   // after the third round: the answer's float bit pattern
  int pad;
};

// s against the midpoint of the floats with bit patterns g and g + 1 (g finite): +1 above, -1 below, 0 the reference's double root is the midpoint
__device__ __forceinline__ int range_side(double s, unsigned int g) {
  const unsigned int ef = (g >> 23) ? (g >> 23) : 1u;  // subnormals step like the lowest normal binade
  const double half_step = __longlong_as_double((long long)(ef + 872u) << 52);  // 2^(ef - 127 - 24)
  const double m = (double)__uint_as_float(g) + half_step;
  const double u = __longlong_as_double(((__double_as_longlong(m) >> 52) - 52) << 52);  // ulp_double(m)
  const double e = __dsub_rn(s, __dmul_rn(m, m));
  const double t = __dmul_rn(m, u);
  return e > t ? 1 : (e <= -t ? -1 : 0);
}

__device__ __forceinline__ unsigned int range_key(const float4 p) {
  const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  const double s = __dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z));
  if (s != s) return kRangeNanKey;
  if (s > 1.7e308) return 0x7f800000u;  // an infinite coordinate (finite floats give s < 2^258)
  unsigned int f = __float_as_uint((float)sqrt(s));
  if (f > 0x7f800000u) f = 0x7f800000u;
#pragma unroll 1
  for (int it = 0; it < 4; ++it) {  // (a candidate within a float step of the answer needs one)
    if (f < 0x7f800000u) {
      const int c = range_side(s, f);
      if (c > 0 || (c == 0 && (f & 1u))) {
        ++f;
        continue;
      }
    }
    if (f > 0u) {
      const int c = range_side(s, f - 1u);
      if (c < 0 || (c == 0 && (f & 1u))) {
        --f;
        continue;
      }
    }
    break;
  }
  return f;
}

// round 0: digit = key >> 21; round 1: (key >> 10) & 2047 of the keys with key >> 21 == prefix >> 21; round 2: key & 1023 of the keys with
// key >> 10 == prefix >> 10.  hist: this round's 2048 bins, zero on entry.
__global__ void __launch_bounds__(kRangeBlock) k_range_hist(const float4* __restrict__ pts, int n, int round, const RangeRec* __restrict__ rec, int* __restrict__ hist) {
  __shared__ int h[kRangeBins];
  for (int b = threadIdx.x; b < kRangeBins; b += kRangeBlock) h[b] = 0;
  const unsigned int prefix = round ? rec->prefix : 0u;
  const int keep_shift = round == 0 ? 32 : (round == 1 ? 21 : 10);  // the bits above it must equal the prefix's
  const int digit_shift = round == 0 ? 21 : (round == 1 ? 10 : 0);
  const unsigned int digit_mask = round == 2 ? 1023u : 2047u;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * kRangeBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kRangeBlock) {
    const unsigned int key = range_key(pts[i]);
    if (keep_shift < 32 && (key >> keep_shift) != (prefix >> keep_shift)) continue;
    atomicAdd(&h[(key >> digit_shift) & digit_mask], 1);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kRangeBins; b += kRangeBlock) {
    const int c = h[b];
    if (c) atomicAdd(&hist[b], c);
  }
}

// One block: the bin that holds rank r (round 0: `rank0`, later rounds: rec->rank) of this round's histogram -> rec.
__global__ void __launch_bounds__(kRangeBlock) k_range_pick(const int* __restrict__ hist, int round, int rank0, RangeRec* __restrict__ rec) {
  constexpr int kPer = kRangeBins / kRangeBlock;  // consecutive bins per thread
  __shared__ int sums[kRangeBlock];
  const int t = threadIdx.x;
  int c[kPer];
  int s = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    c[j] = hist[t * kPer + j];
    s += c[j];
  }
  sums[t] = s;
  __syncthreads();
  const int rank = round ? rec->rank : rank0;
  const unsigned int prefix = round ? rec->prefix : 0u;
  int below = 0;  // points in the bins of the threads before this one (n <= 2^31 - 256: the counts fit an int)
  for (int k = 0; k < t; ++k) below += sums[k];
  __syncthreads();  // (every thread has read rec before one writes it)
  if (rank >= below && rank < below + s) {  // exactly one thread: the bins partition the points that share the prefix
    int r = rank - below;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (r >= 0 && r < c[j]) {
        const int digit_shift = round == 0 ? 21 : (round == 1 ? 10 : 0);
        const unsigned int p = prefix | ((unsigned int)(t * kPer + j) << digit_shift);
        rec->prefix = p;
        rec->rank = r;
        if (round == 2) rec->value = p == kRangeNanKey ? 0x7fc00000u : p;
        r = -1;
      } else if (r >= 0) {
        r -= c[j];
      }
    }
  }
}

}  // namespace ngk
