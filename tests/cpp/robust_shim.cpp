// The robust kernel through the shim, spelled the way a user of a GICP class with robust kernels would: setRobustKernel() next to the
// other settings, align() as before, then robustTerms() to see what was down-weighted.  Prints the results (floats as C99 hex,
// bit-exact) for tests/test_robust_shim.py to compare with the Python API on the same clouds.
//   usage: robust_shim <source.bin> <target.bin> <resolution> <width> <terms_out.bin>   (each cloud file: N x 3 float32)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nano_gicp/nano_gicp.hpp"

using PointType = pcl::PointXYZI;

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

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  auto src = load(argv[1]), tgt = load(argv[2]);
  const double res = std::atof(argv[3]), width = std::atof(argv[4]);

  nano_gicp::NanoGICP<PointType, PointType> gicp;
  if (!gicp.valid()) return 3;
  double w0 = 0.0;
  const nano_gicp::RobustKernel k0 = gicp.getRobustKernel(&w0);
  std::printf("kernel_default %d %a\n", static_cast<int>(k0), w0);
  gicp.setVoxelResolution(res);
  gicp.setNeighborSearchMethod(nano_gicp::NeighborSearchMethod::DIRECT7);
  gicp.setRobustKernel(nano_gicp::RobustKernel::CAUCHY, width);
  double w1 = 0.0;
  const nano_gicp::RobustKernel k1 = gicp.getRobustKernel(&w1);
  std::printf("kernel %d %a\n", static_cast<int>(k1), w1);
  gicp.setInputSource(src);
  gicp.setInputTarget(tgt);
  pcl::PointCloud<PointType> aligned;
  gicp.align(aligned);
  const auto T = gicp.getFinalTransformation();
  std::printf("T");
  for (int i = 0; i < 16; ++i) std::printf(" %a", (double)T.data()[i]);
  std::printf("\nconverged %d iterations %d\n", (int)gicp.hasConverged(), gicp.getNrIterations());
  std::vector<double> s, w;
  if (!gicp.robustTerms(T.template cast<double>(), s, w)) return 4;
  std::printf("terms %zu %zu\n", s.size(), w.size());
  FILE* f = std::fopen(argv[5], "wb");
  if (!f || std::fwrite(s.data(), sizeof(double), s.size(), f) != s.size() || std::fwrite(w.data(), sizeof(double), w.size(), f) != w.size()) return 5;
  std::fclose(f);
  return 0;
}
