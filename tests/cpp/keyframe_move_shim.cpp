// Moving keyframes through the shim, spelled the way a loop-closing DLO fork would use it: the keyframes go into the store as they are
// made, a pose-graph correction moves some of them with transformKeyframes(), setSubmapKeyframes() rebuilds the submap, getKeyframe()
// hands one back.  Writes every keyframe after the move to <out_dir>/kf<i>.bin ({int64 n, n x 3 float32, n x 16 float64}) and prints
// the flags for tests/test_keyframe_move_shim.py to compare with the Python API on the same clouds.
//   usage: keyframe_move_shim <out_dir> <transforms.bin> <keyframe0.bin> [<keyframe1.bin> ...]
//          transforms.bin: one column-major float 4x4 per keyframe, applied to the keyframes in REVERSE order in one call, the first left out
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
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

static void dump(Gicp& g, int id, const std::string& dir) {
  pcl::PointCloud<PointType> cloud;
  Gicp::CovVector covs;
  if (!g.getKeyframe(id, cloud, covs)) std::exit(4);
  FILE* f = std::fopen((dir + "/kf" + std::to_string(id) + ".bin").c_str(), "wb");
  if (!f) std::exit(2);
  const int64_t n = (int64_t)cloud.size();
  std::fwrite(&n, 8, 1, f);
  for (size_t i = 0; i < cloud.size(); ++i) std::fwrite(cloud.points[i].data, 4, 3, f);
  if (n) std::fwrite(covs.data(), 16 * sizeof(double), covs.size(), f);
  std::fclose(f);
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const std::string dir = argv[1];
  const std::vector<float> tf = read_floats(argv[2]);
  const int n_kf = argc - 3;
  if ((int)tf.size() != n_kf * 16) return 2;

  Gicp producer, gicp;
  if (!producer.valid() || !gicp.valid()) return 3;
  std::vector<int> all;
  for (int a = 3; a < argc; ++a) {
    producer.setInputSource(load(argv[a]));
    producer.calculateSourceCovariances();
    all.push_back(gicp.addKeyframe(producer));
  }
  std::vector<int> submap(all.begin(), all.begin() + 2);
  std::printf("submap %d\n", (int)gicp.setSubmapKeyframes(submap));

  std::vector<int> ids;
  std::vector<Gicp::Matrix4> Ts;
  for (int k = n_kf - 1; k >= 1; --k) {
    Gicp::Matrix4 T;
    for (int e = 0; e < 16; ++e) T.data()[e] = tf[(size_t)k * 16 + e];
    ids.push_back(all[k]);
    Ts.push_back(T);
  }
  bool stale = false;
  std::printf("moved %d", (int)gicp.transformKeyframes(ids, Ts, &stale));
  std::printf(" %d %d\n", (int)stale, (int)(gicp.keyframeTransformKernelMs() > 0.0));
  std::printf("submap_again %d\n", (int)gicp.setSubmapKeyframes(submap));
  std::vector<int> twice = {all[0], all[0]};
  std::vector<Gicp::Matrix4> two = {Ts[0], Ts[0]};
  std::printf("refused %d", (int)gicp.transformKeyframes(twice, two, &stale));
  std::printf(" %d\n", (int)stale);
  std::printf("submap_after_refusal %d\n", (int)gicp.setSubmapKeyframes(submap));
  for (int id : all) dump(gicp, id, dir);
  return 0;
}
