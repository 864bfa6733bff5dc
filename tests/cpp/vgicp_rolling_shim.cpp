// The rolling voxel map through the shim, spelled the way an odometry loop would use it: setVoxelResolution() and setVoxelRolling(true)
// once, no target at all, then per scan align() and insertIntoVoxelMap() at the result, evictVoxelMap() now and then.  Prints the results
// (floats as C99 hex, bit-exact) for tests/test_vgicp_rolling_shim.py to compare with the Python API on the same clouds.
//   usage: vgicp_rolling_shim <resolution> <scan0.bin> <scan1.bin> [<scan2.bin> ...]   (each file: N x 3 float32, sensor frame)
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

static void print_T(const char* tag, const Eigen::Matrix4f& T) {
  std::printf("%s", tag);
  for (int i = 0; i < 16; ++i) std::printf(" %a", (double)T.data()[i]);
  std::printf("\n");
}

static void print_stats(const char* tag, const Gicp& g) {
  const Gicp::VoxelRollingStats s = g.voxelRollingStats();
  std::printf("%s %lld %zu %zu %zu %d %d\n", tag, s.inserts, s.n_vox, s.capacity_vox, s.table_slots, (int)(s.last_insert_ms >= 0.0), (int)(s.last_evict_ms >= 0.0));
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const double res = std::atof(argv[1]);

  Gicp gicp;
  if (!gicp.valid()) return 3;
  std::printf("rolling_default %d\n", (int)gicp.getVoxelRolling());
  gicp.setVoxelResolution(res);
  gicp.setVoxelRolling(true);
  std::printf("rolling %d\n", (int)gicp.getVoxelRolling());
  print_stats("stats_empty", gicp);
  Eigen::Matrix4f T = Eigen::Matrix4f::Identity();
  pcl::PointCloud<PointType> aligned;
  for (int a = 2; a < argc; ++a) {
    gicp.setInputSource(load(argv[a]));
    if (a > 2) {  // (the first scan founds the map at identity; no target is ever set)
      gicp.align(aligned, T);
      T = gicp.getFinalTransformation();
      print_T("T", T);
      std::printf("converged %d iterations %d\n", (int)gicp.hasConverged(), gicp.getNrIterations());
    }
    const Gicp::VoxelMapInsert ins = gicp.insertIntoVoxelMap(gicp, T);
    std::printf("insert %d %zu %zu\n", (int)ins.ok, ins.n_new, ins.n_touched);
  }
  print_stats("stats_full", gicp);
  std::printf("voxels %zu\n", gicp.getVoxelMapSize());
  const float centre[3] = {T(0, 3), T(1, 3), T(2, 3)};
  std::printf("evicted %zu\n", gicp.evictVoxelMap(centre, 10.0, 0));
  const Gicp::RollingVoxelMap m = gicp.rollingVoxelMap();
  long long points = 0, stamps = 0;
  for (int c : m.count) points += c;
  for (long long s : m.stamp) stamps += s;
  std::printf("map %zu %lld %lld %d %a %a\n", m.size(), points, stamps, m.size() ? m.ijk[0] : 0, m.size() ? m.sum[0] : 0.0, m.size() ? m.covsum[5] : 0.0);
  print_stats("stats_evicted", gicp);
  gicp.clearVoxelMap();
  print_stats("stats_cleared", gicp);
  return 0;
}
