// The voxel pose search through the shim, spelled as INTEGRATION.md's relocalisation recipe: a rolling voxel map from keyframe scans,
// a lattice of base poses, voxelPoseSearch() for the best candidates.  Prints the results (floats as C99 hex, bit-exact) for
// tests/test_gpu_pose_search.py to compare with the Python API on the same clouds and poses.
//   usage: pose_search_shim <resolution> <ex> <ey> <ez> <top_k> <poses.bin> <query.bin> <map_scan.bin>...
//          (poses: B x 16 float32, each 4x4 column-major; scans: N x 3 float32; the map scans are inserted at identity)
//   pose_search_shim candidate <resolution> <sx> <sy> <sz> <16 floats, column-major, as C99 hex>   prints the candidate pose and exits:
//          needs no GPU (tests/test_pose_search_shim.py)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nano_gicp/nano_gicp.hpp"

using PointType = pcl::PointXYZI;
using Gicp = nano_gicp::NanoGICP<PointType, PointType>;

static std::vector<float> read_floats(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<float> raw(bytes / 4);
  if (std::fread(raw.data(), 4, raw.size(), f) != raw.size()) std::exit(2);
  std::fclose(f);
  return raw;
}

static pcl::PointCloud<PointType>::Ptr load(const char* path) {
  const std::vector<float> raw = read_floats(path);
  pcl::PointCloud<PointType>::Ptr c(new pcl::PointCloud<PointType>);
  for (size_t i = 0; i + 2 < raw.size(); i += 3) c->push_back(PointType(raw[i], raw[i + 1], raw[i + 2]));
  return c;
}

static void print_T(const Eigen::Matrix4f& T) {
  for (int i = 0; i < 16; ++i) std::printf(" %a", (double)T.data()[i]);
}

int main(int argc, char** argv) {
  if (argc == 22 && !std::strcmp(argv[1], "candidate")) {
    const double res = std::strtod(argv[2], nullptr);
    const int shift[3] = {std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5])};
    Eigen::Matrix4f T;
    for (int i = 0; i < 16; ++i) T.data()[i] = (float)std::strtod(argv[6 + i], nullptr);
    std::printf("candidate");
    print_T(Gicp::poseSearchCandidate(T, shift, res));
    std::printf("\n");
    return 0;
  }
  if (argc < 9) return 2;
  const double res = std::atof(argv[1]);
  const int ex = std::atoi(argv[2]), ey = std::atoi(argv[3]), ez = std::atoi(argv[4]), top_k = std::atoi(argv[5]);
  const std::vector<float> raw = read_floats(argv[6]);
  std::vector<Eigen::Matrix4f> poses(raw.size() / 16);
  for (size_t b = 0; b < poses.size(); ++b) std::memcpy(poses[b].data(), &raw[b * 16], 16 * sizeof(float));

  Gicp gicp;
  if (!gicp.valid()) return 3;
  gicp.setVoxelResolution(res);
  gicp.setVoxelRolling(true);
  gicp.setInputSource(load(argv[8]));
  std::printf("empty_map %zu\n", gicp.voxelPoseSearch(poses, ex, ey, ez, top_k).size());  // (refused: a line on stderr)
  for (int a = 8; a < argc; ++a) {
    gicp.setInputSource(load(argv[a]));
    if (!gicp.insertIntoVoxelMap(gicp, Eigen::Matrix4f::Identity()).ok) return 4;
  }
  std::printf("voxels %zu\n", gicp.getVoxelMapSize());
  gicp.setInputSource(load(argv[7]));
  std::printf("no_search %zu\n", gicp.voxelPoseSearchScores().size());  // (refused: the map has changed since - there never was one)
  const std::vector<Gicp::PoseSearchCandidate> best = gicp.voxelPoseSearch(poses, ex, ey, ez, top_k);
  std::printf("found %zu\n", best.size());
  for (const Gicp::PoseSearchCandidate& c : best) {
    std::printf("cand %d %d %d %d %d", c.pose, c.shift[0], c.shift[1], c.shift[2], c.score);
    print_T(c.T);
    std::printf("\n");
  }
  const std::vector<int> vol = gicp.voxelPoseSearchScores();
  long long sum = 0, weighted = 0;
  for (size_t i = 0; i < vol.size(); ++i) sum += vol[i], weighted += (long long)(i % 9973) * vol[i];
  std::printf("volume %zu %lld %lld\n", vol.size(), sum, weighted);
  std::printf("bad_extent %zu\n", gicp.voxelPoseSearch(poses, 32, 0, 0, top_k).size());  // (refused)
  std::printf("kept %zu\n", gicp.voxelPoseSearchScores().size());                          // (a refused call changes nothing)
  std::printf("timed %d\n", (int)(gicp.voxelPoseSearchKernelMs() > 0.0));
  const std::vector<Eigen::Matrix4f> lat = Gicp::yawLattice(Eigen::Matrix4f::Identity(), 4, 1.5707963267948966);
  std::printf("lattice %zu %a %a\n", lat.size(), (double)lat[1](1, 0), (double)lat[2](0, 0));
  return 0;
}
