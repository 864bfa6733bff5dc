// Several initial guesses at once against a voxelized target through the shim: alignBatchVoxel() next to setVoxelResolution() and
// setNeighborSearchMethod(DIRECT7), on a small synthetic pair made here.  Every lane is compared with alignPoseOnly(guess) on the same
// object by memcmp; tests/test_vgicp_batch_shim.py builds this with g++ -Wall -Werror and, on the GPU, runs it.
//   usage: vgicp_batch_shim      exit status 0 and a line "lanes_equal N" when every lane is the single alignment bit for bit
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nano_gicp/nano_gicp.hpp"

using PointType = pcl::PointXYZI;
using GICP = nano_gicp::NanoGICP<PointType, PointType>;

// a floor, two walls and a slanted board, sampled by a fixed linear congruential sequence
static pcl::PointCloud<PointType>::Ptr room(int n, unsigned seed, float dx, float dy, float yaw) {
  pcl::PointCloud<PointType>::Ptr c(new pcl::PointCloud<PointType>);
  unsigned s = seed;
  auto u = [&s]() {
    s = s * 1664525u + 1013904223u;
    return (float)(s >> 8) / 16777216.0f;
  };
  const float cy = std::cos(yaw), sy = std::sin(yaw);
  for (int i = 0; i < n; ++i) {
    const float a = 10.0f * u() - 5.0f, b = 10.0f * u() - 5.0f, h = 3.0f * u();
    float x, y, z;
    switch (i % 4) {
      case 0: x = a; y = b; z = 0.0f; break;
      case 1: x = 5.0f; y = b; z = h; break;
      case 2: x = a; y = -5.0f; z = h; break;
      default: x = 0.4f * a; y = 0.4f * b + 1.0f; z = 0.5f + 0.1f * a; break;
    }
    c->push_back(PointType(cy * x - sy * y + dx, sy * x + cy * y + dy, z));
  }
  return c;
}

static GICP::Matrix4 pose(float x, float y, float z, float yaw) {
  GICP::Matrix4 T = GICP::Matrix4::Identity();
  T(0, 0) = std::cos(yaw); T(0, 1) = -std::sin(yaw);
  T(1, 0) = std::sin(yaw); T(1, 1) = std::cos(yaw);
  T(0, 3) = x; T(1, 3) = y; T(2, 3) = z;
  return T;
}

int main() {
  GICP gicp;
  if (!gicp.valid()) return 3;
  gicp.setInputSource(room(1500, 1u, 0.0f, 0.0f, 0.0f));
  gicp.setInputTarget(room(6000, 2u, 0.25f, -0.15f, 0.03f));
  const std::vector<GICP::Matrix4> guesses = {GICP::Matrix4::Identity(), pose(0.25f, -0.15f, 0.0f, 0.03f), pose(0.6f, 0.3f, 0.05f, -0.1f), pose(-1.0f, 0.5f, 0.0f, 0.3f),
                                              pose(400.0f, 0.0f, 0.0f, 0.0f)};
  if (!gicp.alignBatchVoxel(guesses).empty()) {  // the voxel mode is off: refused
    std::fprintf(stderr, "alignBatchVoxel ran with the voxel mode off\n");
    return 4;
  }
  gicp.setVoxelResolution(1.0);
  gicp.setNeighborSearchMethod(nano_gicp::NeighborSearchMethod::DIRECT7);
  const std::vector<GICP::BatchResult> lanes = gicp.alignBatchVoxel(guesses);
  if (lanes.size() != guesses.size()) return 5;
  bool moved = false;
  for (size_t g = 0; g < guesses.size(); ++g) {
    gicp.alignPoseOnly(guesses[g]);
    const GICP::Matrix4 T = gicp.getFinalTransformation();
    const auto& H = gicp.getFinalHessian();
    std::printf("lane %zu converged %d iterations %d t %a %a %a\n", g, (int)lanes[g].converged, lanes[g].nr_iterations, (double)T(0, 3), (double)T(1, 3), (double)T(2, 3));
    if (std::memcmp(lanes[g].transformation.data(), T.data(), 16 * sizeof(float)) != 0 || std::memcmp(lanes[g].hessian.data(), H.data(), 36 * sizeof(double)) != 0 ||
        lanes[g].converged != gicp.hasConverged() || lanes[g].nr_iterations != gicp.getNrIterations()) {
      std::fprintf(stderr, "lane %zu differs from alignPoseOnly(guess)\n", g);
      return 6;
    }
    if (std::memcmp(T.data(), guesses[g].data(), 16 * sizeof(float)) != 0) moved = true;
  }
  if (!moved) {
    std::fprintf(stderr, "no lane left its guess\n");
    return 7;
  }
  std::printf("lanes_equal %zu\n", guesses.size());
  return 0;
}
