// The batch surface of the shim (include/nano_gicp/nano_gicp.hpp): alignBatch(guesses) and getFitnessScores(transforms) beside the
// reference's own calls.  Prints, per guess, the batch's result and the result of align(guess) / getFitnessScore() on the same object
// (floats as C99 hex, bit-exact) for tests/test_batch_shim.py to compare.
//   usage: batch_shim <source.bin> <target.bin> <guesses.bin> <max_corr_dist> <max_range>
//   (clouds: N x 3 float32; guesses: B x 16 float32, column-major 4x4 each)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nano_gicp/nano_gicp.hpp"

using PointType = pcl::PointXYZI;

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

static void print_result(const char* tag, size_t lane, const Eigen::Matrix4f& T, bool converged, int iterations, const nano_gicp::types::Matrix6d& H, double fitness,
                         double fitness_range) {
  std::printf("%s %zu %d %d", tag, lane, (int)converged, iterations);
  for (int i = 0; i < 16; ++i) std::printf(" %a", (double)T.data()[i]);
  for (int i = 0; i < 36; ++i) std::printf(" %a", H.data()[i]);
  std::printf(" %a %a\n", fitness, fitness_range);
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  auto src = load(argv[1]), tgt = load(argv[2]);
  const std::vector<float> graw = read_floats(argv[3]);
  const double max_corr_dist = std::atof(argv[4]), max_range = std::atof(argv[5]);
  std::vector<Eigen::Matrix4f> guesses(graw.size() / 16);
  for (size_t g = 0; g < guesses.size(); ++g)
    for (int i = 0; i < 16; ++i) guesses[g].data()[i] = graw[g * 16 + i];

  nano_gicp::NanoGICP<PointType, PointType> gicp;
  if (!gicp.valid()) return 3;
  gicp.setMaxCorrespondenceDistance(max_corr_dist);
  gicp.setInputSource(src);
  gicp.setInputTarget(tgt);

  const auto batch = gicp.alignBatch(guesses);
  if (batch.size() != guesses.size()) return 4;
  std::vector<Eigen::Matrix4f> finals;
  for (const auto& r : batch) finals.push_back(r.transformation);
  const std::vector<double> fit = gicp.getFitnessScores(finals), fit_range = gicp.getFitnessScores(finals, max_range);
  if (fit.size() != guesses.size() || fit_range.size() != guesses.size()) return 5;
  // the getters keep the results of the last align(): none yet
  std::printf("untouched %d\n", (int)(!gicp.hasConverged()));
  for (size_t g = 0; g < guesses.size(); ++g) print_result("batch", g, batch[g].transformation, batch[g].converged, batch[g].nr_iterations, batch[g].hessian, fit[g], fit_range[g]);
  pcl::PointCloud<PointType> aligned;
  for (size_t g = 0; g < guesses.size(); ++g) {
    gicp.align(aligned, guesses[g]);
    print_result("loop", g, gicp.getFinalTransformation(), gicp.hasConverged(), gicp.getNrIterations(), gicp.getFinalHessian(), gicp.getFitnessScore(),
                 gicp.getFitnessScore(max_range));
  }
  return 0;
}
