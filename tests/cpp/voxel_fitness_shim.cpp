// The voxel fitness through the shim, spelled as INTEGRATION.md's relocalisation recipe: a rolling map saved in one handle and restored in
// another that never sees a target cloud, alignBatchVoxel() from several guesses, getVoxelFitnessScores() of the results, the per-point
// values of the best one.  Prints the results (floats as C99 hex, bit-exact) and writes the per-point arrays for
// tests/test_gpu_voxel_fitness.py to compare with the Python API on the same clouds.
//   usage: voxel_fitness_shim <resolution> <gate> <points_out.bin> <map_scan.bin> <query_scan.bin>   (scans: N x 3 float32)
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

static void print_fitness(const char* tag, const Gicp::VoxelFitness& f) {
  std::printf("%s %d %a %a %zu %zu\n", tag, (int)f.ok, f.mahalanobis, f.sqdist, f.n_inliers, f.n_matched);
}

static Eigen::Matrix4f shifted(float x, float y) {
  Eigen::Matrix4f T = Eigen::Matrix4f::Identity();
  T(0, 3) = x;
  T(1, 3) = y;
  return T;
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const double res = std::atof(argv[1]), gate = std::atof(argv[2]);

  Gicp mapper, gicp;
  if (!mapper.valid() || !gicp.valid()) return 3;
  print_fitness("mode_off", gicp.getVoxelFitness());  // (refused: a line on stderr, ok false)
  for (Gicp* g : {&mapper, &gicp}) {
    g->setVoxelResolution(res);
    g->setVoxelRolling(true);
  }
  mapper.setInputSource(load(argv[4]));
  const Gicp::VoxelMapInsert ins = mapper.insertIntoVoxelMap(mapper, Eigen::Matrix4f::Identity());
  std::printf("insert %d %zu\n", (int)ins.ok, ins.n_new);

  gicp.setInputSource(load(argv[5]));
  print_fitness("empty_map", gicp.getVoxelFitness());  // (refused)
  std::printf("restored %d\n", (int)gicp.setRollingVoxelMap(mapper.rollingVoxelMap(), mapper.voxelRollingStats().inserts));  // (no target, ever)

  const std::vector<Eigen::Matrix4f> guesses = {Eigen::Matrix4f::Identity(), shifted(0.3f, -0.2f), shifted(25.f, 0.f)};
  const std::vector<Gicp::BatchResult> lanes = gicp.alignBatchVoxel(guesses);
  std::printf("lanes %zu\n", lanes.size());
  std::vector<Eigen::Matrix4f> finals;
  for (const Gicp::BatchResult& r : lanes) finals.push_back(r.transformation);
  const std::vector<Gicp::VoxelFitness> scores = gicp.getVoxelFitnessScores(finals, gate);
  size_t best = 0;
  for (size_t i = 0; i < scores.size(); ++i) {
    print_fitness("lane", scores[i]);
    if (2 * scores[i].n_matched >= gicp.getInputSource()->size() && scores[i].mahalanobis < scores[best].mahalanobis) best = i;  // an overlap, then the lowest score
  }
  std::printf("best %zu\n", best);
  if (finals.empty()) return 4;

  pcl::PointCloud<PointType> aligned;
  gicp.align(aligned, guesses[best]);
  print_fitness("final", gicp.getVoxelFitness(gate));
  print_fitness("final_ungated", gicp.getVoxelFitness());

  std::vector<double> m, sqd;
  std::vector<int> voxel;
  const bool have_points = gicp.voxelFitnessPoints(finals[best], m, sqd, voxel);
  std::printf("points %d %zu\n", (int)have_points, m.size());
  FILE* f = std::fopen(argv[3], "wb");
  if (!f) return 5;
  std::fwrite(m.data(), sizeof(double), m.size(), f);
  std::fwrite(sqd.data(), sizeof(double), sqd.size(), f);
  std::fwrite(voxel.data(), sizeof(int), voxel.size(), f);
  std::fclose(f);
  return 0;
}
