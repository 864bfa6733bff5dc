// Scan context through the shim, spelled as INTEGRATION.md's loop-closure recipe: every keyframe scan's descriptor is added to the
// database while the scan is the source, a later scan is matched against all of them, and the best entry's shift becomes the yaw guess
// of an align() against that keyframe.  Prints the results (doubles as C99 hex, bit-exact) for tests/test_gpu_scan_context.py to
// compare with the Python API on the same clouds.
//   usage: scan_context_shim <top_k> <query_scan.bin> <keyframe_scan.bin>...   (scans: N x 3 float32)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nano_gicp/nano_gicp.hpp"

using PointType = pcl::PointXYZI;
using Gicp = nano_gicp::NanoGICP<PointType, PointType>;

static pcl::PointCloud<PointType>::Ptr load(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<float> raw(bytes / 4);
  if (std::fread(raw.data(), 4, raw.size(), f) != raw.size()) std::exit(2);
  std::fclose(f);
  pcl::PointCloud<PointType>::Ptr c(new pcl::PointCloud<PointType>);
  for (size_t i = 0; i + 2 < raw.size(); i += 3) c->push_back(PointType(raw[i], raw[i + 1], raw[i + 2]));
  return c;
}

static void print_matches(const char* tag, const std::vector<Gicp::ScanContextMatch>& m) {
  std::printf("%s %zu", tag, m.size());
  for (const Gicp::ScanContextMatch& e : m) std::printf(" %d %a %d", e.id, e.distance, e.shift);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int top_k = std::atoi(argv[1]);
  Gicp gicp;
  if (!gicp.valid()) return 3;

  const Gicp::ScanContextParams p = gicp.getScanContextParams();
  std::printf("params %d %d %a %a\n", p.n_rings, p.n_sectors, (double)p.max_radius, (double)p.z_offset);
  std::printf("refused %d\n", (int)gicp.setScanContextParams(20, 61, 80.f, 2.f));  // (an odd sector count: a line on stderr)
  std::vector<float> e2, b;
  const bool have_tables = gicp.scanContextTables(e2, b);  // (filled before anything of them is read: a call's arguments are evaluated in no fixed order)
  if (!have_tables || e2.empty() || b.size() < 3) return 6;
  std::printf("tables %d %zu %zu %a %a\n", (int)have_tables, e2.size(), b.size(), (double)e2.back(), (double)b[2]);
  std::fflush(stdout);

  std::vector<pcl::PointCloud<PointType>::Ptr> keyframes;
  for (int i = 3; i < argc; ++i) {
    keyframes.push_back(load(argv[i]));
    gicp.setInputSource(keyframes.back());
    std::printf("added %d\n", gicp.addScanContext());  // (where DLO's updateKeyframes pushes the keyframe)
  }
  std::printf("count %zu\n", gicp.numScanContexts());

  gicp.setInputSource(load(argv[2]));
  const size_t n = gicp.numScanContexts();
  const std::vector<Gicp::ScanContextMatch> best = gicp.matchScanContext(0, 0, n, top_k);
  print_matches("match", best);
  print_matches("distances", gicp.scanContextDistances(0, 0, n));
  print_matches("tail", gicp.matchScanContext(0, n / 2, n, top_k));

  const std::vector<float> desc = gicp.computeScanContext(0);
  print_matches("match_desc", gicp.matchScanContext(desc, 0, n, top_k));
  const int id = gicp.addScanContextDescriptor(desc);
  std::printf("added_desc %d same %d\n", id, (int)(gicp.scanContext(id) == desc));
  print_matches("self", gicp.matchScanContext(desc, (size_t)id, (size_t)id + 1));
  print_matches("bad_range", gicp.matchScanContext(0, 0, n + 5));  // (refused)
  if (best.empty()) return 4;

  gicp.setInputTarget(keyframes[(size_t)best[0].id]);
  pcl::PointCloud<PointType> aligned;
  gicp.align(aligned, gicp.scanContextGuess(best[0].shift));
  const Eigen::Matrix4f T = gicp.getFinalTransformation();
  std::printf("aligned %d", (int)gicp.hasConverged());
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) std::printf(" %a", (double)T(r, c));
  std::printf("\n");
  gicp.clearScanContexts();
  std::printf("cleared %zu\n", gicp.numScanContexts());
  return 0;
}
