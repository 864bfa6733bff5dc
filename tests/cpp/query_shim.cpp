// The query surface of the shim, spelled the way users of the reference class spell it: the public kd-tree members searched
// through `->` (KdTreeFLANN::nearestKSearch / radiusSearch, include/nano_gicp/nanoflann.hpp:141-175 of the reference) and
// pcl::Registration::getFitnessScore.  Prints every result (floats as C99 hex, bit-exact) for tests/test_query_shim.py to compare
// with the Python API on the same clouds.
//   usage: query_shim <source.bin> <target.bin> <queries.bin> <k> <radius> <max_range>   (each file: N x 3 float32)
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

static void print_hits(const char* tag, int n, const std::vector<int>& idx, const std::vector<float>& d2) {
  std::printf("%s %d", tag, n);
  for (int i : idx) std::printf(" %d", i);
  for (float d : d2) std::printf(" %a", (double)d);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  auto src = load(argv[1]), tgt = load(argv[2]), queries = load(argv[3]);
  const int k = std::atoi(argv[4]);
  const double radius = std::atof(argv[5]), max_range = std::atof(argv[6]);

  nano_gicp::NanoGICP<PointType, PointType> gicp;
  if (!gicp.valid()) return 3;
  gicp.setInputSource(src);
  gicp.setInputTarget(tgt);
  std::printf("fitness_before_align %a\n", gicp.getFitnessScore());
  pcl::PointCloud<PointType> aligned;
  gicp.align(aligned);
  const Eigen::Matrix4f T = gicp.getFinalTransformation();
  std::printf("T");
  for (int i = 0; i < 16; ++i) std::printf(" %a", (double)T.data()[i]);
  std::printf("\n");
  std::printf("fitness %a\n", gicp.getFitnessScore());
  std::printf("fitness_range %a\n", gicp.getFitnessScore(max_range));

  std::vector<int> idx, all_knn_idx, all_rad_idx;
  std::vector<float> d2, all_knn_d2, all_rad_d2;
  for (const PointType& q : queries->points) {
    int n = gicp.target_kdtree_->nearestKSearch(q, k, idx, d2);
    print_hits("tknn", n, idx, d2);
    all_knn_idx.insert(all_knn_idx.end(), idx.begin(), idx.end());
    all_knn_d2.insert(all_knn_d2.end(), d2.begin(), d2.end());
    n = gicp.source_kdtree_->nearestKSearch(q, k, idx, d2);
    print_hits("sknn", n, idx, d2);
    n = gicp.target_kdtree_->radiusSearch(q, radius, idx, d2);
    print_hits("trad", n, idx, d2);
    all_rad_idx.insert(all_rad_idx.end(), idx.begin(), idx.end());
    all_rad_d2.insert(all_rad_d2.end(), d2.begin(), d2.end());
    n = gicp.source_kdtree_->radiusSearch(q, radius, idx, d2);
    print_hits("srad", n, idx, d2);
  }

  // the batched forms give what the single-point calls gave, concatenated
  std::vector<size_t> offsets;
  const size_t m = gicp.target_kdtree_->nearestKSearch(*queries, k, idx, d2);
  std::printf("batched_knn %zu %d\n", m, (int)(idx == all_knn_idx && d2 == all_knn_d2));
  const size_t total = gicp.target_kdtree_->radiusSearch(*queries, radius, offsets, idx, d2);
  std::printf("batched_radius %zu %d %zu\n", total, (int)(idx == all_rad_idx && d2 == all_rad_d2), offsets.size());
  std::printf("offsets");
  for (size_t o : offsets) std::printf(" %zu", o);
  std::printf("\n");
  return 0;
}
