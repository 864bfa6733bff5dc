// The host arithmetic of the correlative pose search (csrc/ngicp_pose_search.h; include/ngicp.h "voxel pose search"):
// the caps of a window, the index of a shift and the plan of the dense occupancy bit grid the score kernel reads.  Plain C++ with
// nothing of HIP in it: tests/cpp/pose_search_plan.cpp compiles it into a program of its own and holds it to the numpy model.
//
//   the grid     covers  map box  INTERSECTED WITH  (source box dilated by the extents), cell-aligned, inclusive on both ends.  A cell
//                outside the map box holds no voxel, and a cell outside the dilated source box is no c_b(p) + s of any point: bits
//                outside the grid are never asked for by a window that counts.
//   its layout   bit (x - org[0]) of row (z - org[2]) * ny + (y - org[1]); a row is `row_words` 64-bit words: one guard word, then
//                ceil(nx / 64) data words (x along the bits, bit 0 first), then one guard word.  Guards and the bits past nx stay 0.
//   a window     of a point whose cell is c, for the shift row (sy, sz): the 2 ex + 1 bits from local x  l = c.x - ex - org[0]  on.  It
//                touches the grid iff l + 2 ex >= 0 and l <= nx - 1; then its first bit is bit 64 + l >= 1 of the row, and because
//                2 ex + 1 <= 63 the two words at (64 + l) / 64 and the next one hold all of it: the last of them is at most word
//                ceil(nx / 64) + 1, the rear guard.  A window that touches nothing is skipped on the integers, before an address is formed.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ngps {

constexpr int kMaxExtentXY = 31;          // a row of shifts is at most 63 bits wide
constexpr int kMaxExtentZ = 7;
constexpr int kMaxShifts = 12288;         // 48 KB of int32 in LDS
constexpr long long kMaxEntries = 1ll << 24;  // B * |S|
constexpr int kMaxTopK = 64;
constexpr size_t kMaxGridBytes = (size_t)256 << 20;  // the bit grid's cap: 256 MiB
constexpr int kCellLimit = 1 << 20;       // |i| < 2^20 per axis (ngk::kVoxBias)

// inclusive cell box; empty when lo > hi on any axis (what the device leaves when nothing was seen: INT_MAX / INT_MIN)
struct Box {
  int lo[3], hi[3];
  bool empty() const { return lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]; }
};

struct Plan {
  bool empty;        // nothing can score: every score is 0 and no grid is built
  bool too_large;    // bytes > kMaxGridBytes: the call is refused
  int org[3];        // the cell of bit 0 of row 0
  int nx, ny, nz;    // cells per axis
  int row_words;     // 64-bit words per row, the two guards included
  size_t words, bytes;
};

// number of shifts of a window, or -1 when an extent or the product is beyond its cap
inline long long shift_count(int ex, int ey, int ez) {
  if (ex < 0 || ey < 0 || ez < 0 || ex > kMaxExtentXY || ey > kMaxExtentXY || ez > kMaxExtentZ) return -1;
  const long long s = (long long)(2 * ex + 1) * (2 * ey + 1) * (2 * ez + 1);
  return s > kMaxShifts ? -1 : s;
}

// B >= 1 poses, a window inside its caps, B * |S| <= 2^24
inline bool entries_ok(long long n_poses, int ex, int ey, int ez) {
  const long long s = shift_count(ex, ey, ez);
  if (s < 0 || n_poses < 1) return false;
  return n_poses <= kMaxEntries / s;
}

inline int shift_index(int sx, int sy, int sz, int ex, int ey, int ez) { return ((sz + ez) * (2 * ey + 1) + (sy + ey)) * (2 * ex + 1) + (sx + ex); }

inline void shift_of_index(int idx, int ex, int ey, int ez, int s[3]) {
  const int wx = 2 * ex + 1, wy = 2 * ey + 1;
  s[0] = idx % wx - ex;
  s[1] = (idx / wx) % wy - ey;
  s[2] = idx / (wx * wy) - ez;
}

inline Plan plan_grid(const Box& map, const Box& src, int ex, int ey, int ez) {
  Plan p{};
  const int e[3] = {ex, ey, ez};
  if (map.empty() || src.empty()) {
    p.empty = true;
    return p;
  }
  int n[3];
  for (int a = 0; a < 3; ++a) {
    // (boxes lie inside (-2^20, 2^20) and extents are at most 31: nothing overflows)
    const int lo = map.lo[a] > src.lo[a] - e[a] ? map.lo[a] : src.lo[a] - e[a];
    const int hi = map.hi[a] < src.hi[a] + e[a] ? map.hi[a] : src.hi[a] + e[a];
    if (lo > hi) {
      p.empty = true;
      return p;
    }
    p.org[a] = lo;
    n[a] = hi - lo + 1;
  }
  p.nx = n[0], p.ny = n[1], p.nz = n[2];
  p.row_words = (p.nx + 63) / 64 + 2;
  p.words = (size_t)p.row_words * (size_t)p.ny * (size_t)p.nz;  // < 2^15 * 2^21 * 2^21 = 2^57
  p.bytes = p.words * sizeof(uint64_t);
  p.too_large = p.bytes > kMaxGridBytes;
  return p;
}

// the candidate pose's translation on one axis: (float)((double)t + (double)s * res)
inline float shifted_translation(float t, int s, double res) { return (float)((double)t + (double)s * res); }

}  // namespace ngps
