// Motion deskew the way a DLIO-style callback built on the shim spells it: a DeskewTrajectory filled pose by pose, the point times
// once in an array of their own (deskewCloud) and once inside the point records (preprocessScanDeskewed, whose result becomes the
// input source on the device).  Prints every output coordinate as C99 hex (bit-exact) for tests/test_deskew_shim.py to compare with
// the Python API.
//   usage: deskew_shim <scan.bin> <times.bin> <traj.bin>   (N x 3 float32; N float32 seconds; M x 17 float64 {time, pose column-major})
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nano_gicp/nano_gicp.hpp"

using PointType = pcl::PointXYZI;

template <class T>
static std::vector<T> load(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<T> raw(bytes / sizeof(T));
  if (std::fread(raw.data(), sizeof(T), raw.size(), f) != raw.size()) std::exit(2);
  std::fclose(f);
  return raw;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::vector<float> xyz = load<float>(argv[1]), times = load<float>(argv[2]);
  const std::vector<double> traj_raw = load<double>(argv[3]);
  const size_t n = times.size(), M = traj_raw.size() / 17;
  if (xyz.size() != n * 3 || M < 2) return 2;
  nano_gicp::NanoGICP<PointType, PointType> gicp;
  if (!gicp.valid()) return 3;

  nano_gicp::DeskewTrajectory traj;
  nano_gicp::types::Matrix4d T;
  for (size_t k = 0; k < M; ++k) {
    for (int e = 0; e < 16; ++e) T.data()[e] = traj_raw[k * 17 + 1 + e];
    traj.addPose(traj_raw[k * 17], T);
  }
  traj.setReference(T);  // the frame at the end of the sweep

  pcl::PointCloud<PointType> scan, out;
  for (size_t i = 0; i < n; ++i) {
    PointType p(xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], (float)i);
    p.data_c[1] = times[i];  // a driver's per-point time, in the record's padding
    scan.push_back(p);
  }
  // 1. the times in an array of their own, host to host
  traj.setTimes(times.data());
  if (!gicp.deskewCloud(scan, traj, out) || out.size() != n) return 4;
  for (size_t i = 0; i < n; ++i) std::printf("cloud %a %a %a %a\n", (double)out[i].data[0], (double)out[i].data[1], (double)out[i].data[2], (double)out[i].intensity);
  // 2. the times inside the records; the deskewed scan becomes the input source without a download
  traj.setTimesInRecord((long)((const char*)&scan.points[0].data_c[1] - (const char*)scan.points[0].data), NGICP_TIME_F32_S);
  pcl::PointCloud<PointType> pre = scan;
  if (!gicp.preprocessScanDeskewed(pre, traj, true, 0.f, 0.f, /*set_as_source=*/true)) return 5;
  for (size_t i = 0; i < pre.size(); ++i) std::printf("scan %a %a %a %a\n", (double)pre[i].data[0], (double)pre[i].data[1], (double)pre[i].data[2], (double)pre[i].intensity);
  std::printf("median %a\n", (double)gicp.medianRange());
  // 3. a refused trajectory (one pose) is reported, changes nothing and throws nothing
  nano_gicp::DeskewTrajectory one;
  one.addPose(0.0, T);
  one.setTimes(times.data());
  pcl::PointCloud<PointType> kept = scan;
  const bool a = gicp.deskewCloud(scan, one, out), b = gicp.preprocessScanDeskewed(kept, one, true, 0.f, 0.f);
  std::printf("refused %d %d %zu\n", (int)!a, (int)!b, kept.size());
  return 0;
}
