// Voxelized GICP through the shim, spelled the way a user of the reference class would add it: one setVoxelResolution() call next to
// the other setters, then align() as before.  Prints the results (floats as C99 hex, bit-exact) for tests/test_vgicp_shim.py to compare
// with the Python API on the same clouds.
//   usage: vgicp_shim <source.bin> <target.bin> <resolution>   (each file: N x 3 float32)
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

static void print_T(const char* tag, const Eigen::Matrix4f& T) {
  std::printf("%s", tag);
  for (int i = 0; i < 16; ++i) std::printf(" %a", (double)T.data()[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  auto src = load(argv[1]), tgt = load(argv[2]);
  const double res = std::atof(argv[3]);

  nano_gicp::NanoGICP<PointType, PointType> gicp;
  if (!gicp.valid()) return 3;
  std::printf("resolution_default %a\n", gicp.getVoxelResolution());
  gicp.setVoxelResolution(res);
  std::printf("resolution %a\n", gicp.getVoxelResolution());
  gicp.setInputSource(src);
  gicp.setInputTarget(tgt);
  std::printf("voxels %zu\n", gicp.getVoxelMapSize());
  pcl::PointCloud<PointType> aligned;
  gicp.align(aligned);
  print_T("T", gicp.getFinalTransformation());
  std::printf("converged %d iterations %d\n", (int)gicp.hasConverged(), gicp.getNrIterations());
  gicp.setVoxelResolution(0.0);  // back to exact GICP on the same object
  gicp.align(aligned);
  print_T("T_exact", gicp.getFinalTransformation());
  return 0;
}
