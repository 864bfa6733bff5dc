// computeSpaciousness (src/dlo/odom.cc:990-1010 of the reference) the way a DLO built on the shim spells it: the scan is
// preprocessed on the device and becomes the input source without a download, medianRange() takes the median of its ranges there,
// and SpaciousnessFilter holds the low-pass state.  Prints every median and filtered value as C99 hex (bit-exact) for
// tests/test_metrics_shim.py to compare with the Python API and a float32 restatement of the filter.
//   usage: metrics_shim <crop> <leaf> <scan.bin>...   (each file: N x 3 float32)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nano_gicp/nano_gicp.hpp"

using PointType = pcl::PointXYZI;

static pcl::PointCloud<PointType> load(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<float> raw(bytes / 4);
  if (std::fread(raw.data(), 4, raw.size(), f) != raw.size()) std::exit(2);
  std::fclose(f);
  pcl::PointCloud<PointType> c;
  for (size_t i = 0; i + 2 < raw.size(); i += 3) c.push_back(PointType(raw[i], raw[i + 1], raw[i + 2]));
  return c;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const float crop = (float)std::atof(argv[1]), leaf = (float)std::atof(argv[2]);
  nano_gicp::NanoGICP<PointType, PointType> gicp_s2s;
  if (!gicp_s2s.valid()) return 3;
  nano_gicp::SpaciousnessFilter spaciousness_lpf;
  for (int i = 3; i < argc; ++i) {
    pcl::PointCloud<PointType> scan = load(argv[i]);
    gicp_s2s.preprocessPoints(scan, true, crop, leaf, /*set_as_source=*/true);
    // the two lines computeSpaciousness() becomes
    const float median_curr = gicp_s2s.medianRange();
    const float median_lpf = spaciousness_lpf.update(median_curr);
    std::printf("scan %zu %a %a %a %a\n", scan.size(), (double)median_curr, (double)median_lpf, (double)gicp_s2s.medianRange(2),
                (double)gicp_s2s.rangeSelect(scan.size() - 1));
  }
  std::printf("bad_rank %d\n", (int)(gicp_s2s.rangeSelect((size_t)1 << 40) != gicp_s2s.rangeSelect((size_t)1 << 40)));  // NaN on failure
  return 0;
}
