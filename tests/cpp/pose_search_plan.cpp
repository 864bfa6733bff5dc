// The pose search's host arithmetic (direct_lidar_odometry_amd/csrc/ngicp_pose_search_plan.h) as a program of its own: no library, no GPU.
//   pose_search_plan <cases.txt>   each line: map lo xyz, map hi xyz, source lo xyz, source hi xyz, ex ey ez (15 integers).  Prints one
//                                  line per case: "empty" or "plan ox oy oz nx ny nz row_words bytes too_large"
// and then the self-checks: the caps, the shift index and its inverse over whole windows, the candidate translation, and - for every grid
// width up to 300 cells and every extent - that the two words a window reads lie inside its row and that a skipped window holds no cell
// of the grid.  Ends with "checks N failures F".
#include <cstdio>
#include <cstdlib>

#include "../../direct_lidar_odometry_amd/csrc/ngicp_pose_search_plan.h"

static long long checks = 0, failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    ++checks;                                                      \
    if (!(c)) {                                                    \
      ++failures;                                                  \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);         \
    }                                                              \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int v[15];
  for (;;) {
    int got = 0;
    for (; got < 15; ++got)
      if (std::fscanf(f, "%d", &v[got]) != 1) break;
    if (got != 15) break;
    const ngps::Box map{{v[0], v[1], v[2]}, {v[3], v[4], v[5]}}, src{{v[6], v[7], v[8]}, {v[9], v[10], v[11]}};
    const ngps::Plan p = ngps::plan_grid(map, src, v[12], v[13], v[14]);
    if (p.empty) std::printf("empty\n");
    else std::printf("plan %d %d %d %d %d %d %d %zu %d\n", p.org[0], p.org[1], p.org[2], p.nx, p.ny, p.nz, p.row_words, p.bytes, (int)p.too_large);
  }
  std::fclose(f);

  // ---- the caps ----
  CHECK(ngps::shift_count(0, 0, 0) == 1);
  CHECK(ngps::shift_count(31, 31, 0) == 63 * 63);
  CHECK(ngps::shift_count(31, 31, 1) == 63 * 63 * 3);  // 11907
  CHECK(ngps::shift_count(31, 31, 2) == -1);           // 19845 > 12288
  CHECK(ngps::shift_count(32, 0, 0) == -1 && ngps::shift_count(0, 32, 0) == -1 && ngps::shift_count(0, 0, 8) == -1);
  CHECK(ngps::shift_count(-1, 0, 0) == -1 && ngps::shift_count(0, -1, 0) == -1 && ngps::shift_count(0, 0, -1) == -1);
  CHECK(ngps::shift_count(31, 6, 7) == 63 * 13 * 15);  // 12285: the largest window with ez = 7
  CHECK(ngps::shift_count(31, 7, 7) == -1);            // 14175 > 12288
  CHECK(ngps::entries_ok(1, 0, 0, 0) && ngps::entries_ok(1ll << 24, 0, 0, 0));
  CHECK(!ngps::entries_ok((1ll << 24) + 1, 0, 0, 0) && !ngps::entries_ok(0, 0, 0, 0) && !ngps::entries_ok(1, 32, 0, 0));
  CHECK(ngps::entries_ok(1409, 31, 31, 1) && !ngps::entries_ok(1410, 31, 31, 1));  // 2^24 / 11907 = 1409.02

  // ---- the shift index and its inverse ----
  const int windows[][3] = {{0, 0, 0}, {1, 0, 0}, {3, 2, 1}, {31, 1, 0}, {0, 31, 7}, {12, 12, 1}};
  for (const auto& w : windows) {
    int next = 0;
    for (int sz = -w[2]; sz <= w[2]; ++sz)
      for (int sy = -w[1]; sy <= w[1]; ++sy)
        for (int sx = -w[0]; sx <= w[0]; ++sx) {
          const int i = ngps::shift_index(sx, sy, sz, w[0], w[1], w[2]);
          int s[3];
          ngps::shift_of_index(i, w[0], w[1], w[2], s);
          CHECK(i == next++ && s[0] == sx && s[1] == sy && s[2] == sz);
        }
    CHECK(next == ngps::shift_count(w[0], w[1], w[2]));
  }

  // ---- the candidate translation ----
  CHECK(ngps::shifted_translation(0.25f, 3, 0.5) == 1.75f);
  CHECK(ngps::shifted_translation(-1.0f, -31, 0.1) == (float)(-1.0 + -31.0 * 0.1));
  CHECK(ngps::shifted_translation(7.0f, 0, 0.3) == 7.0f);

  // ---- a window's two words lie in its row; a skipped window holds nothing of the grid ----
  for (int nx = 1; nx <= 300; ++nx) {
    const ngps::Box map{{-5, 0, 0}, {-5 + nx - 1, 0, 0}}, src{{-1000, 0, 0}, {1000, 0, 0}};
    for (int ex = 0; ex <= 31; ++ex) {
      const ngps::Plan p = ngps::plan_grid(map, src, ex, 0, 0);
      CHECK(!p.empty && p.nx == nx && p.org[0] == -5 && p.row_words == (nx + 63) / 64 + 2);
      for (int cx = -5 - 70; cx <= -5 + nx + 70; ++cx) {
        const int l = cx - ex - p.org[0];
        const bool touches = l + 2 * ex >= 0 && l <= p.nx - 1;
        bool any = false;  // does some cx + sx lie in the grid?
        for (int sx = -ex; sx <= ex; ++sx) any = any || (cx + sx >= p.org[0] && cx + sx < p.org[0] + p.nx);
        CHECK(touches == any);
        if (touches) {
          const int pos = l + 64;
          CHECK(pos >= 1 && (pos >> 6) + 1 <= p.row_words - 1);
          // every bit of the window that is a cell of the grid sits in a data word, at the cell's own bit
          for (int sx = -ex; sx <= ex; ++sx) {
            const int lx = cx + sx - p.org[0], bit = pos + (sx + ex);
            if (lx >= 0 && lx < p.nx) CHECK(bit == 64 + lx && (bit >> 6) >= 1 && (bit >> 6) <= p.row_words - 2);
          }
        }
      }
    }
  }
  std::printf("checks %lld failures %lld\n", checks, failures);
  return failures ? 1 : 0;
}
