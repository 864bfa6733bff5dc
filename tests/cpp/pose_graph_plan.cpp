// Stand-alone driver of csrc/ngicp_pose_graph_plan.h (no library, no GPU): reads cases from the file named on the command line and prints,
// per case, what the header answers.  tests/test_pose_graph_plan_cpu.py compares the lines with the numpy model's answers.
//   graph n m  f_0 .. f_{n-1}  i_0 j_0 .. i_{m-1} j_{m-1}     -> csr <offsets> ; <entries> ; ungauged <k>
//   nodes n_now count listed  [bad]*listed                     -> ok | refused        bad: 0 fine, 1 a NaN, 2 a last row
//   edges n_nodes m_now count listed  [i j zbad ibad]*listed   -> ok | refused        zbad as above; ibad: 0 fine, 1 asymmetric, 2 a NaN
// `count` is what the call claims; only the first `listed` items exist (a call beyond a cap must be refused before anything is read).
#include <cstdio>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>

#include "../../direct_lidar_odometry_amd/csrc/ngicp_pose_graph_plan.h"

static void identity16(double* T, int bad) {
  for (int e = 0; e < 16; ++e) T[e] = (e % 5 == 0) ? 1.0 : 0.0;
  T[12] = 3.0, T[13] = -2.0, T[14] = 0.5;
  if (bad == 1) T[9] = std::numeric_limits<double>::quiet_NaN();
  if (bad == 2) T[7] = 1e-300;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  long cases = 0;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string kind;
    if (!(ss >> kind)) continue;
    ++cases;
    if (kind == "graph") {
      size_t n, m;
      ss >> n >> m;
      std::vector<unsigned char> fixed(n);
      for (size_t k = 0; k < n; ++k) {
        int f;
        ss >> f;
        fixed[k] = (unsigned char)f;
      }
      std::vector<int> ij(2 * m);
      for (size_t e = 0; e < 2 * m; ++e) ss >> ij[e];
      std::vector<int> off, ent;
      ngpg::build_csr(n, ij.data(), m, off, ent);
      std::printf("csr");
      for (int v : off) std::printf(" %d", v);
      std::printf(" ;");
      for (int v : ent) std::printf(" %d", v);
      std::printf(" ; ungauged %zu\n", ngpg::ungauged_components(n, ij.data(), m, fixed.data()));
    } else if (kind == "nodes") {
      size_t n_now, count, listed;
      ss >> n_now >> count >> listed;
      std::vector<double> T(listed * 16 + 16);
      for (size_t k = 0; k < listed; ++k) {
        int bad;
        ss >> bad;
        identity16(T.data() + k * 16, bad);
      }
      size_t where = 0;
      const ngpg::Refusal r = ngpg::check_add_nodes(n_now, T.data(), count, &where);
      std::printf("%s\n", r == ngpg::kOk ? "ok" : "refused");
    } else if (kind == "edges") {
      size_t n_nodes, m_now, count, listed;
      ss >> n_nodes >> m_now >> count >> listed;
      std::vector<int> ij(2 * listed + 2);
      std::vector<double> Z(listed * 16 + 16), L(listed * 36 + 36, 0.0);
      for (size_t e = 0; e < listed; ++e) {
        int zbad, ibad;
        ss >> ij[2 * e] >> ij[2 * e + 1] >> zbad >> ibad;
        identity16(Z.data() + e * 16, zbad);
        double* l = L.data() + e * 36;
        for (int a = 0; a < 6; ++a)
          for (int b = 0; b < 6; ++b) l[a * 6 + b] = (a == b ? 4.0 : 0.0) + 0.125 * (a + b);
        if (ibad == 1) l[2 * 6 + 4] += 1e-15;
        if (ibad == 2) l[5 * 6 + 5] = std::numeric_limits<double>::infinity();
      }
      size_t where = 0;
      const ngpg::Refusal r = ngpg::check_add_edges(n_nodes, m_now, ij.data(), Z.data(), L.data(), count, &where);
      std::printf("%s\n", r == ngpg::kOk ? "ok" : "refused");
    } else {
      return 3;
    }
  }
  std::printf("cases %ld\n", cases);
  return 0;
}
