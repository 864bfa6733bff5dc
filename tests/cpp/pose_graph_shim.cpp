// Compile-and-run check of the pose-graph surface of the C++ shim (include/nano_gicp/nano_gicp.hpp) without PCL or Eigen:
//   pose_graph_shim <out dir> <graph.bin>
// graph.bin: int64 n, int64 m, n x 16 doubles (poses, column-major), n bytes (fixed), m x 2 int32, m x 16 doubles (Z), m x 36 doubles
// (information), m bytes (robust flags).  The program loads the graph through the matrix forms, optimises it, writes the poses and the
// corrections (out dir/poses.bin, corrections.bin) and prints what tests/test_pose_graph_shim.py compares with the Python API.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include <nano_gicp/nano_gicp.hpp>

using Gicp = nano_gicp::NanoGICP<pcl::PointXYZI, pcl::PointXYZI>;
namespace types = nano_gicp::types;

static bool read_all(const std::string& path, std::vector<unsigned char>& out) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  out.resize((size_t)n);
  const bool ok = std::fread(out.data(), 1, (size_t)n, f) == (size_t)n;
  std::fclose(f);
  return ok;
}

template <class T>
static bool write_all(const std::string& path, const std::vector<T>& v) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
  std::fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string dir = argv[1];
  std::vector<unsigned char> raw;
  if (!read_all(argv[2], raw)) return 3;
  const unsigned char* p = raw.data();
  const int64_t n = reinterpret_cast<const int64_t*>(p)[0], m = reinterpret_cast<const int64_t*>(p)[1];
  p += 16;
  const double* poses = reinterpret_cast<const double*>(p);
  p += n * 128;
  const unsigned char* fixed = p;
  p += n;
  p += (8 - (n % 8)) % 8;
  const int* ij = reinterpret_cast<const int*>(p);
  p += m * 8;
  const double* Z = reinterpret_cast<const double*>(p);
  p += m * 128;
  const double* info = reinterpret_cast<const double*>(p);
  p += m * 288;
  const unsigned char* robust = p;

  Gicp g;
  std::vector<types::Matrix4d> T((size_t)n);
  for (int64_t k = 0; k < n; ++k)
    for (int e = 0; e < 16; ++e) T[(size_t)k].data()[e] = poses[k * 16 + e];
  const int first = g.poseGraphAddNodes(T, std::vector<unsigned char>(fixed, fixed + n));
  std::vector<Gicp::PoseGraphEdge> edges((size_t)m);
  for (int64_t e = 0; e < m; ++e) {
    Gicp::PoseGraphEdge& ed = edges[(size_t)e];
    ed.i = ij[2 * e], ed.j = ij[2 * e + 1];
    for (int q = 0; q < 16; ++q) ed.Z.data()[q] = Z[e * 16 + q];
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) ed.info(a, b) = info[e * 36 + a * 6 + b];
    ed.robust = robust[e] != 0;
  }
  const int first_edge = g.poseGraphAddEdges(edges);
  size_t nn = 0, mm = 0;
  g.poseGraphSize(&nn, &mm);
  std::printf("added %d %d %zu %zu\n", first, first_edge, nn, mm);
  // a refused add: a self-edge; nothing changes
  Gicp::PoseGraphEdge bad = edges[0];
  bad.j = bad.i;
  const int refused = g.poseGraphAddEdges(std::vector<Gicp::PoseGraphEdge>(1, bad));
  g.poseGraphSize(&nn, &mm);
  std::printf("refused %d %zu %zu\n", refused, nn, mm);
  g.poseGraphSetRobust(NGICP_ROBUST_CAUCHY, 3.0);
  double chi2 = 0.0;
  g.poseGraphLinearize(&chi2, nullptr, nullptr, nullptr, nullptr);
  ngicp_pg_options opt = {40, 1e-4, 1e-4, 1e-8, 30000};
  ngicp_pg_result res;
  const bool ok = g.poseGraphOptimize(&opt, &res);
  std::printf("optimize %d %d %d %lld %d %d %.17g %.17g %.17g\n", ok ? 1 : 0, res.iterations, res.accepted, res.cg_iterations, res.converged, res.n_trace, chi2,
              res.initial_chi2, res.final_chi2);
  std::vector<types::Matrix4d> out;
  g.poseGraphPoses(out);
  std::vector<double> flat(out.size() * 16);
  for (size_t k = 0; k < out.size(); ++k)
    for (int e = 0; e < 16; ++e) flat[k * 16 + e] = out[k].data()[e];
  std::vector<int> ids((size_t)n);
  for (int64_t k = 0; k < n; ++k) ids[(size_t)k] = (int)k;
  std::vector<Gicp::Matrix4> Cs;
  const bool okc = g.poseGraphCorrections(ids, Cs);
  std::vector<float> cflat(Cs.size() * 16);
  for (size_t k = 0; k < Cs.size(); ++k)
    for (int e = 0; e < 16; ++e) cflat[k * 16 + e] = Cs[k].data()[e];
  std::printf("corrections %d %zu %d\n", okc ? 1 : 0, Cs.size(), g.poseGraphKernelMs() > 0.0 ? 1 : 0);
  if (!write_all(dir + "/poses.bin", flat) || !write_all(dir + "/corrections.bin", cflat)) return 4;
  // edgeFromAlignment on the first edge's ends
  types::Matrix6d H = types::Matrix6d::Identity(), Lam;
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) H(a, b) = (a == b ? 50.0 + 7.0 * a : 0.0) + 0.5 * (a + b);
  types::Matrix4d Zm;
  Gicp::edgeFromAlignment(T[0], T[1], H, Zm, Lam);
  std::printf("edge");
  for (int e = 0; e < 16; ++e) std::printf(" %.17g", Zm.data()[e]);
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) std::printf(" %.17g", Lam(a, b));
  std::printf("\n");
  g.poseGraphClear();
  g.poseGraphSize(&nn, &mm);
  std::printf("cleared %zu %zu\n", nn, mm);
  return 0;
}
