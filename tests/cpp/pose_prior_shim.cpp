// The pose prior through the C++ shim (include/nano_gicp/nano_gicp.hpp): setPosePrior / getPosePrior / posePriorTerms / clearPosePrior
// around one exact-route align.  tests/test_pose_prior_shim.py runs the same calls through the Python host and compares bit for bit.
// usage: pose_prior_shim source.bin target.bin params.bin out.bin
//   source / target: float32 xyz;  params: doubles, column-major - T_prior 16, info 36, guess 16, the pose for posePriorTerms 16
//   out: doubles - final transform 16 (column-major), Hessian 36 (column-major), iterations, converged, | set, T_prior 16, info 36 as
//   the getter returns them | r 6, cost, H_p 36 (column-major), b_p 6 | a bad prior: setPosePrior's result, the getter's result
//   afterwards, | posePriorTerms after clearPosePrior: its result, getPosePrior's result
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "nano_gicp/nano_gicp.hpp"

using PointType = pcl::PointXYZI;
using nano_gicp::types::Matrix4d;
using nano_gicp::types::Matrix6d;

static std::vector<char> slurp(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<char> raw(bytes);
  if (std::fread(raw.data(), 1, raw.size(), f) != raw.size()) std::exit(2);
  std::fclose(f);
  return raw;
}

static pcl::PointCloud<PointType>::Ptr load(const char* path) {
  const std::vector<char> raw = slurp(path);
  const float* v = reinterpret_cast<const float*>(raw.data());
  pcl::PointCloud<PointType>::Ptr c(new pcl::PointCloud<PointType>);
  for (size_t i = 0; i + 2 < raw.size() / 4; i += 3) c->push_back(PointType(v[i], v[i + 1], v[i + 2]));
  return c;
}

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const auto source = load(argv[1]), target = load(argv[2]);
  const std::vector<char> raw = slurp(argv[3]);
  if (raw.size() != (16 + 36 + 16 + 16) * sizeof(double)) return 2;
  const double* p = reinterpret_cast<const double*>(raw.data());
  Matrix4d T_prior, T_eval;
  Matrix6d info;
  Eigen::Matrix4f guess;
  for (int i = 0; i < 16; ++i) T_prior.data()[i] = p[i], guess.data()[i] = (float)p[52 + i], T_eval.data()[i] = p[68 + i];
  for (int i = 0; i < 36; ++i) info.data()[i] = p[16 + i];

  nano_gicp::NanoGICP<PointType, PointType> gicp;
  if (!gicp.valid()) return 3;
  gicp.setMaxCorrespondenceDistance(1.0);
  gicp.setInputSource(source);
  gicp.setInputTarget(target);
  std::vector<double> out;
  if (!gicp.setPosePrior(T_prior, info)) return 4;
  gicp.alignPoseOnly(guess);
  const Eigen::Matrix4f T = gicp.getFinalTransformation();
  for (int i = 0; i < 16; ++i) out.push_back((double)T.data()[i]);
  for (int i = 0; i < 36; ++i) out.push_back(gicp.getFinalHessian().data()[i]);
  out.push_back(gicp.getNrIterations());
  out.push_back(gicp.hasConverged() ? 1.0 : 0.0);

  Matrix4d Tg;
  Matrix6d Ig;
  out.push_back(gicp.getPosePrior(&Tg, &Ig) ? 1.0 : 0.0);
  for (int i = 0; i < 16; ++i) out.push_back(Tg.data()[i]);
  for (int i = 0; i < 36; ++i) out.push_back(Ig.data()[i]);

  double r[6], b[6], cost = -1.0;
  Matrix6d Hp;
  if (!gicp.posePriorTerms(T_eval, r, &cost, &Hp, b)) return 5;
  for (int i = 0; i < 6; ++i) out.push_back(r[i]);
  out.push_back(cost);
  for (int i = 0; i < 36; ++i) out.push_back(Hp.data()[i]);
  for (int i = 0; i < 6; ++i) out.push_back(b[i]);

  Matrix6d bad = info;
  bad(0, 1) = std::numeric_limits<double>::quiet_NaN();
  out.push_back(gicp.setPosePrior(T_prior, bad) ? 1.0 : 0.0);  // (reported on stderr, changes nothing)
  out.push_back(gicp.getPosePrior(&Tg, &Ig) && Ig(0, 1) == info(0, 1) ? 1.0 : 0.0);

  gicp.clearPosePrior();
  out.push_back(gicp.posePriorTerms(T_eval, r, &cost, &Hp, b) ? 1.0 : 0.0);
  out.push_back(gicp.getPosePrior() ? 1.0 : 0.0);

  FILE* f = std::fopen(argv[4], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 6;
  std::fclose(f);
  return 0;
}
