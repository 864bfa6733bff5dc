// Clearing the rolling voxel map along a scan's rays through the shim, the way an odometry loop would use it: the first scan founds the
// map at identity, the second one - at the pose given - first counts (a dry run), then clears the map, and is inserted behind that.
// Prints the results (floats as C99 hex, bit-exact) for tests/test_vgicp_ray_shim.py to compare with the Python API on the same clouds.
//   usage: vgicp_ray_shim <resolution> <tx> <ty> <tz> <scan0.bin> <scan1.bin>   (each file: N x 3 float32, sensor frame)
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

static void print_result(const char* tag, const Gicp::RayClearResult& r) {
  std::printf("%s %d %zu %lld %lld %lld %d\n", tag, (int)r.ok, r.n_removed, r.steps, r.occupied, r.misses, (int)(r.kernel_ms >= 0.0));
}

static void print_counts(const char* tag, Gicp& g) {
  std::vector<uint32_t> miss, hit;
  const bool ok = g.voxelMapRayCounts(miss, hit);
  std::printf("%s_ok %d %zu\n", tag, (int)ok, miss.size());
  std::printf("%s_miss", tag);
  for (uint32_t v : miss) std::printf(" %u", v);
  std::printf("\n%s_hit", tag);
  for (uint32_t v : hit) std::printf(" %u", v);
  std::printf("\n");
}

static void print_map(const char* tag, Gicp& g) {
  const Gicp::RollingVoxelMap m = g.rollingVoxelMap();
  std::printf("%s_n %zu %lld\n", tag, m.size(), g.voxelRollingStats().inserts);
  std::printf("%s_ijk", tag);
  for (int v : m.ijk) std::printf(" %d", v);
  std::printf("\n%s_count", tag);
  for (int v : m.count) std::printf(" %d", v);
  std::printf("\n%s_stamp", tag);
  for (long long v : m.stamp) std::printf(" %lld", v);
  std::printf("\n%s_sum", tag);
  for (double v : m.sum) std::printf(" %a", v);
  std::printf("\n%s_covsum", tag);
  for (double v : m.covsum) std::printf(" %a", v);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const double res = std::atof(argv[1]);

  Gicp gicp;
  if (!gicp.valid()) return 3;
  gicp.setVoxelResolution(res);
  gicp.setVoxelRolling(true);
  print_counts("before", gicp);  // (no call yet: refused, a line on stderr)
  Eigen::Matrix4f T = Eigen::Matrix4f::Identity();
  gicp.setInputSource(load(argv[5]));
  const Gicp::VoxelMapInsert first = gicp.insertIntoVoxelMap(gicp, T);
  std::printf("insert %d %zu %zu\n", (int)first.ok, first.n_new, first.n_touched);

  gicp.setInputSource(load(argv[6]));
  T(0, 3) = (float)std::atof(argv[2]);
  T(1, 3) = (float)std::atof(argv[3]);
  T(2, 3) = (float)std::atof(argv[4]);
  Gicp::RayClearOptions opt;
  opt.dry_run = true;
  print_result("dry", gicp.clearVoxelMapAlongRays(gicp, T, nullptr, opt));
  print_counts("dry", gicp);
  Gicp::RayClearOptions bad;
  bad.near_cells = 0;
  print_result("refused", gicp.clearVoxelMapAlongRays(gicp, T, nullptr, bad));  // (a line on stderr; nothing changes)
  print_counts("refused", gicp);
  print_map("kept", gicp);
  opt = Gicp::RayClearOptions();
  opt.radius_cells = 0.5;
  opt.min_miss = 1;
  const float origin[3] = {T(0, 3), T(1, 3), T(2, 3) + 0.25f};
  print_result("clear", gicp.clearVoxelMapAlongRays(gicp, T, origin, opt));
  print_counts("clear", gicp);
  print_map("cleared", gicp);
  const Gicp::VoxelMapInsert second = gicp.insertIntoVoxelMap(gicp, T);
  std::printf("insert %d %zu %zu\n", (int)second.ok, second.n_new, second.n_touched);
  print_counts("stale", gicp);  // (the insert changed the map: refused)
  return 0;
}
