// The rolling voxel map's record routes through the shim: a map built from scans on one object is saved (rollingVoxelMap), restored on
// a second (setRollingVoxelMap), merged into a third at another resolution from the device (insertVoxelMapFrom) and from the saved
// arrays (insertVoxelsIntoVoxelMap), and moved in place (transformVoxelMap).  Every resulting map is written to <out_dir>/<tag>.bin
// for tests/test_vgicp_rollmap_shim.py to compare, byte for byte, with the Python API on the same clouds.
//   usage: vgicp_rollmap_shim <resolution> <out_dir> <scan0.bin> <scan1.bin> [...]   (each scan: N x 3 float32, sensor frame)
#include <cstdio>
#include <cstdlib>
#include <string>
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

// <n as int64> ijk (n x 3 int32) sum (n x 3 f64) covsum (n x 6 f64) count (n int32) stamp (n int64); then the insert counter
static void dump(const std::string& dir, const char* tag, Gicp& g) {
  const Gicp::RollingVoxelMap m = g.rollingVoxelMap();
  const long long n = (long long)m.size(), inserts = g.voxelRollingStats().inserts;
  FILE* f = std::fopen((dir + "/" + tag + ".bin").c_str(), "wb");
  if (!f) std::exit(2);
  std::fwrite(&n, sizeof(n), 1, f);
  std::fwrite(m.ijk.data(), sizeof(int), m.ijk.size(), f);
  std::fwrite(m.sum.data(), sizeof(double), m.sum.size(), f);
  std::fwrite(m.covsum.data(), sizeof(double), m.covsum.size(), f);
  std::fwrite(m.count.data(), sizeof(int), m.count.size(), f);
  std::fwrite(m.stamp.data(), sizeof(long long), m.stamp.size(), f);
  std::fwrite(&inserts, sizeof(inserts), 1, f);
  std::fclose(f);
  std::printf("%s %lld %lld\n", tag, n, inserts);
}

// a yaw given by its cosine and sine as decimal literals (3-4-5 and 7-24-25 triangles), so that the test spells the same float bits
static Eigen::Matrix4f pose(float x, float y, float c, float s) {
  Eigen::Matrix4f T = Eigen::Matrix4f::Identity();
  T(0, 0) = c; T(0, 1) = -s; T(1, 0) = s; T(1, 1) = c;
  T(0, 3) = x; T(1, 3) = y;
  return T;
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const double res = std::atof(argv[1]);
  const std::string dir = argv[2];

  Gicp a, b, c;
  if (!a.valid() || !b.valid() || !c.valid()) return 3;
  for (Gicp* g : {&a, &b}) g->setVoxelResolution(res);
  c.setVoxelResolution(2.0 * res);
  for (Gicp* g : {&a, &b, &c}) g->setVoxelRolling(true);

  for (int k = 3; k < argc; ++k) {  // scan i at a pose of its own (no alignment here: tests/cpp/vgicp_rolling_shim.cpp drives that loop)
    const int i = k - 3;
    a.setInputSource(load(argv[k]));
    const Gicp::VoxelMapInsert ins = a.insertIntoVoxelMap(a, pose(0.5f * i, 0.125f * i, i % 2 ? 0.96f : 1.f, i % 2 ? 0.28f : 0.f));
    std::printf("scan %d %zu %zu\n", (int)ins.ok, ins.n_new, ins.n_touched);
  }
  const float origin[3] = {0.f, 0.f, 0.f};
  std::printf("evicted %zu\n", a.evictVoxelMap(origin, 14.0, 0));
  dump(dir, "built", a);

  // save / load
  const Gicp::RollingVoxelMap saved = a.rollingVoxelMap();
  std::printf("set %d\n", (int)b.setRollingVoxelMap(saved, a.voxelRollingStats().inserts));
  dump(dir, "restored", b);
  Gicp::RollingVoxelMap twice = saved;  // the first row again at the end: refused, and b stays as it is
  for (int k = 0; k < 3; ++k) twice.ijk.push_back(saved.ijk[k]);
  for (int k = 0; k < 3; ++k) twice.sum.push_back(saved.sum[k]);
  for (int k = 0; k < 6; ++k) twice.covsum.push_back(saved.covsum[k]);
  twice.count.push_back(saved.count[0]);
  twice.stamp.push_back(saved.stamp[0]);
  std::printf("set_duplicate %d\n", (int)b.setRollingVoxelMap(twice, a.voxelRollingStats().inserts));
  dump(dir, "after_refusal", b);

  // merge two handles' maps, at another resolution: from the device, then from the saved arrays at a second pose
  Gicp::VoxelMapInsert ins = c.insertVoxelMapFrom(a, pose(0.25f, -0.5f, 0.8f, 0.6f));
  std::printf("insert_map %d %zu %zu\n", (int)ins.ok, ins.n_new, ins.n_touched);
  ins = c.insertVoxelsIntoVoxelMap(saved, pose(-1.5f, 0.75f, 0.96f, -0.28f));
  std::printf("insert_voxels %d %zu %zu\n", (int)ins.ok, ins.n_new, ins.n_touched);
  dump(dir, "merged", c);
  ins = c.insertVoxelMapFrom(c, Eigen::Matrix4f::Identity());  // a map cannot be inserted into itself
  std::printf("insert_self %d\n", (int)ins.ok);

  // move in place (a loop closure's correction)
  bool ok = false;
  const size_t left = b.transformVoxelMap(pose(0.375f, 0.25f, 0.6f, -0.8f), &ok);
  std::printf("transform %d %zu\n", (int)ok, left);
  dump(dir, "moved", b);
  return 0;
}
