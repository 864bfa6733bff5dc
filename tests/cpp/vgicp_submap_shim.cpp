// The merged voxel map through the shim, spelled the way DLO would use it: setVoxelResolution() and setVoxelSubmapMerge(true) once, then
// the keyframe store and setSubmapKeyframes() as before.  Prints the results (floats as C99 hex, bit-exact) for
// tests/test_vgicp_submap_shim.py to compare with the Python API on the same clouds.
//   usage: vgicp_submap_shim <resolution> <source.bin> <keyframe0.bin> [<keyframe1.bin> ...]   (each file: N x 3 float32, world frame)
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
  const Gicp::VoxelMapMergeStats s = g.voxelMapMergeStats();
  std::printf("%s %lld %lld %d %d\n", tag, s.merged_builds, s.parts_built, (int)(s.last_parts_ms >= 0.0), (int)(s.last_merge_ms >= 0.0));
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const double res = std::atof(argv[1]);
  auto src = load(argv[2]);

  Gicp producer, gicp;
  if (!producer.valid() || !gicp.valid()) return 3;
  std::printf("merge_default %d\n", (int)gicp.getVoxelSubmapMerge());
  gicp.setVoxelResolution(res);
  gicp.setVoxelSubmapMerge(true);
  std::printf("merge %d\n", (int)gicp.getVoxelSubmapMerge());
  Eigen::Matrix4f I = Eigen::Matrix4f::Identity();
  std::vector<int> ids;
  for (int a = 3; a < argc; ++a) {
    producer.setInputSource(load(argv[a]));
    ids.push_back(gicp.addKeyframeTransformed(producer, I));
  }
  gicp.setSubmapKeyframes(ids);
  print_stats("stats_before", gicp);
  std::printf("voxels %zu\n", gicp.getVoxelMapSize());
  print_stats("stats_merged", gicp);
  const Gicp::KeyframeVoxelMap part = gicp.keyframeVoxelMap(ids.back());
  long long points = 0;
  for (int c : part.count) points += c;
  std::printf("part %zu %lld %a\n", part.size(), points, part.size() ? part.sum[0] : 0.0);
  gicp.setInputSource(src);
  pcl::PointCloud<PointType> aligned;
  gicp.align(aligned);
  print_T("T", gicp.getFinalTransformation());
  std::printf("converged %d iterations %d\n", (int)gicp.hasConverged(), gicp.getNrIterations());
  gicp.setVoxelSubmapMerge(false);  // back to the map summed over the submap's points, on the same object
  std::printf("voxels_off %zu\n", gicp.getVoxelMapSize());
  print_stats("stats_off", gicp);
  gicp.align(aligned);
  print_T("T_off", gicp.getFinalTransformation());
  return 0;
}
