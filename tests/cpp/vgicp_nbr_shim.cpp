// The DIRECT7 / DIRECT27 neighbourhoods of voxelized GICP through the shim, spelled the way a user of a voxelized-GICP class would:
// setNeighborSearchMethod() next to setVoxelResolution(), then align() as before.  Prints the results (floats as C99 hex, bit-exact) for
// tests/test_vgicp_nbr_shim.py to compare with the Python API on the same clouds.
//   usage: vgicp_nbr_shim <source.bin> <target.bin> <resolution> <corr_out.bin>   (each cloud file: N x 3 float32)
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
  if (argc != 5) return 2;
  auto src = load(argv[1]), tgt = load(argv[2]);
  const double res = std::atof(argv[3]);

  nano_gicp::NanoGICP<PointType, PointType> gicp;
  if (!gicp.valid()) return 3;
  std::printf("neighbors_default %d\n", static_cast<int>(gicp.getNeighborSearchMethod()));
  gicp.setVoxelResolution(res);
  gicp.setNeighborSearchMethod(nano_gicp::NeighborSearchMethod::DIRECT7);
  std::printf("neighbors %d\n", static_cast<int>(gicp.getNeighborSearchMethod()));
  gicp.setInputSource(src);
  gicp.setInputTarget(tgt);
  pcl::PointCloud<PointType> aligned;
  gicp.align(aligned);
  print_T("T", gicp.getFinalTransformation());
  std::printf("converged %d iterations %d\n", (int)gicp.hasConverged(), gicp.getNrIterations());
  const std::vector<int> corr = gicp.voxelCorrespondences();
  std::printf("corr_ints %zu\n", corr.size());
  FILE* f = std::fopen(argv[4], "wb");
  if (!f || std::fwrite(corr.data(), sizeof(int), corr.size(), f) != corr.size()) return 4;
  std::fclose(f);
  gicp.setNeighborSearchMethod(nano_gicp::NeighborSearchMethod::DIRECT27);
  gicp.align(aligned);
  print_T("T27", gicp.getFinalTransformation());
  std::printf("corr27_ints %zu\n", gicp.voxelCorrespondences().size());
  return 0;
}
