// The gated insert of the rolling voxel map through the shim, the way an odometry loop would use it: the first scan founds the map at
// identity, ungated; the second one - at the pose given - is first classified (a dry run), then refused once (a bad option), then inserted
// through the gate.  Prints the results (floats as C99 hex, bit-exact) for tests/test_vgicp_gate_shim.py to compare with the Python API on
// the same clouds.
//   usage: vgicp_gate_shim <resolution> <max_mahalanobis> <tx> <ty> <tz> <scan0.bin> <scan1.bin>   (each file: N x 3 float32, sensor frame)
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

static void print_result(const char* tag, const Gicp::GatedInsert& r) {
  std::printf("%s %d %zu %zu %zu %zu %zu %zu %zu %zu %d\n", tag, (int)r.ok, r.n_points, r.n_class[Gicp::INSERT_NEW], r.n_class[Gicp::INSERT_EXPLAINED],
              r.n_class[Gicp::INSERT_CONFLICT], r.n_class[Gicp::INSERT_UNJUDGED], r.n_kept, r.n_new, r.n_touched, (int)(r.kernel_ms >= 0.0));
}

static void print_classes(const char* tag, Gicp& g) {
  std::vector<uint8_t> cls;
  const bool ok = g.voxelMapInsertClasses(cls);
  std::printf("%s_ok %d %zu\n", tag, (int)ok, cls.size());
  std::printf("%s_cls", tag);
  for (uint8_t v : cls) std::printf(" %d", (int)v);
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
  if (argc != 8) return 2;
  const double res = std::atof(argv[1]);

  Gicp gicp;
  if (!gicp.valid()) return 3;
  gicp.setVoxelResolution(res);
  gicp.setNeighborSearchMethod(nano_gicp::NeighborSearchMethod::DIRECT7);
  gicp.setVoxelRolling(true);
  print_classes("before", gicp);  // (no call yet: refused, a line on stderr)
  Eigen::Matrix4f T = Eigen::Matrix4f::Identity();
  gicp.setInputSource(load(argv[6]));
  const Gicp::VoxelMapInsert first = gicp.insertIntoVoxelMap(gicp, T);
  std::printf("insert %d %zu %zu\n", (int)first.ok, first.n_new, first.n_touched);

  gicp.setInputSource(load(argv[7]));
  T(0, 3) = (float)std::atof(argv[3]);
  T(1, 3) = (float)std::atof(argv[4]);
  T(2, 3) = (float)std::atof(argv[5]);
  Gicp::GatedInsertOptions opt;
  opt.max_mahalanobis = std::atof(argv[2]);
  opt.dry_run = true;
  print_result("dry", gicp.insertIntoVoxelMapGated(gicp, T, opt));
  print_classes("dry", gicp);
  Gicp::GatedInsertOptions bad = opt;
  bad.min_voxel_count = 0;
  print_result("refused", gicp.insertIntoVoxelMapGated(gicp, T, bad));  // (a line on stderr; nothing changes)
  print_classes("refused", gicp);
  print_map("kept", gicp);
  opt.dry_run = false;
  opt.min_voxel_count = 2;
  opt.insert_unjudged = false;
  print_result("gated", gicp.insertIntoVoxelMapGated(gicp, T, opt));
  print_classes("gated", gicp);
  print_map("inserted", gicp);
  return 0;
}
