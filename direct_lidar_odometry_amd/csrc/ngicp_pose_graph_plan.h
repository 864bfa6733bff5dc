// The host arithmetic of the pose graph (csrc/ngicp_pose_graph.h; include/ngicp.h "pose graph"): the caps, what an add
// refuses, the union-find that finds a connected component without a fixed node, and the per-node incidence lists the kernels walk.
// Plain C++ with nothing of HIP in it: tests/cpp/pose_graph_plan.cpp compiles it into a program of its own and holds it to the numpy
// model (tests/_pose_graph_model.py).
//
//   ids          dense, in order of insertion, for nodes and for edges
//   an edge      (i, j), i != j, both known; several edges may join one pair, and (j, i) with j > i is as good as (i, j)
//   the lists    node k's incident edges as entries 2 * edge + side (side 0: k is the edge's i; 1: its j), ascending in the edge id -
//                the written order of every per-node sum.  offsets[n + 1], entries[2 m].
//   the gauge    every connected component needs a fixed node; a node without edges is a component of its own
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ngpg {

constexpr size_t kMaxNodes = (size_t)1 << 20;
constexpr size_t kMaxEdges = (size_t)1 << 22;
constexpr int kTraceCap = 256;  // rows of ngicp_pg_result::trace
constexpr int kTraceCols = 5;   // chi2 of the try, lambda, gain ratio, CG iterations, accepted

// bytes of the device arrays, in size_t (2^22 edges x 288 bytes is beyond 2^30)
constexpr size_t kNodeDoubles = 12;   // a pose: R row-major (9), t (3)
constexpr size_t kEdgeLinDoubles = 36;  // a linearised edge: M upper triangle (21), g (6), r (6), s, w, rho
inline size_t pose_bytes(size_t n) { return n * kNodeDoubles * sizeof(double); }
inline size_t edge_lin_bytes(size_t m) { return m * kEdgeLinDoubles * sizeof(double); }
inline size_t edge_const_bytes(size_t m) { return m * (12 + 36) * sizeof(double); }  // Z as a pose, Lambda row-major

enum Refusal { kOk = 0, kEmpty, kNull, kCap, kUnknownId, kSelfEdge, kNotFinite, kLastRow, kAsymmetric };

inline const char* refusal_text(Refusal r) {
  switch (r) {
    case kOk: return "ok";
    case kEmpty: return "n == 0";
    case kNull: return "a null array";
    case kCap: return "beyond the cap (2^20 nodes, 2^22 edges)";
    case kUnknownId: return "an unknown node id";
    case kSelfEdge: return "a self-edge";
    case kNotFinite: return "an entry that is not finite";
    case kLastRow: return "a last row other than (0, 0, 0, 1)";
    case kAsymmetric: return "an information matrix whose mirrored entries are not equal";
  }
  return "?";
}

// a column-major 4x4: every entry finite, last row exactly (0, 0, 0, 1)
inline Refusal check_pose16(const double* T) {
  for (int e = 0; e < 16; ++e)
    if (!std::isfinite(T[e])) return kNotFinite;
  if (T[3] != 0.0 || T[7] != 0.0 || T[11] != 0.0 || T[15] != 1.0) return kLastRow;
  return kOk;
}

// a 6x6: every entry finite, and Lambda[a][b] == Lambda[b][a] exactly
inline Refusal check_info36(const double* L) {
  for (int e = 0; e < 36; ++e)
    if (!std::isfinite(L[e])) return kNotFinite;
  for (int a = 0; a < 6; ++a)
    for (int b = a + 1; b < 6; ++b)
      if (L[a * 6 + b] != L[b * 6 + a]) return kAsymmetric;
  return kOk;
}

// everything ngicp_pose_graph_add_nodes refuses; *bad receives the index of the offending node
inline Refusal check_add_nodes(size_t n_now, const double* T_n16, size_t n, size_t* bad) {
  *bad = 0;
  if (n == 0) return kEmpty;
  if (!T_n16) return kNull;
  if (n > kMaxNodes || n_now > kMaxNodes - n) return kCap;
  for (size_t k = 0; k < n; ++k) {
    const Refusal r = check_pose16(T_n16 + k * 16);
    if (r != kOk) {
      *bad = k;
      return r;
    }
  }
  return kOk;
}

// everything ngicp_pose_graph_add_edges refuses; *bad receives the index of the offending edge
inline Refusal check_add_edges(size_t n_nodes, size_t m_now, const int* ij_n2, const double* Z_n16, const double* info_n36, size_t n, size_t* bad) {
  *bad = 0;
  if (n == 0) return kEmpty;
  if (!ij_n2 || !Z_n16 || !info_n36) return kNull;
  if (n > kMaxEdges || m_now > kMaxEdges - n) return kCap;
  for (size_t e = 0; e < n; ++e) {
    *bad = e;
    const int i = ij_n2[2 * e], j = ij_n2[2 * e + 1];
    if (i < 0 || j < 0 || (size_t)i >= n_nodes || (size_t)j >= n_nodes) return kUnknownId;
    if (i == j) return kSelfEdge;
    Refusal r = check_pose16(Z_n16 + e * 16);
    if (r != kOk) return r;
    r = check_info36(info_n36 + e * 36);
    if (r != kOk) return r;
  }
  *bad = 0;
  return kOk;
}

// union-find over the edges: union by the smaller root id, full path compression
struct UnionFind {
  std::vector<int> parent;
  explicit UnionFind(size_t n) : parent(n) {
    for (size_t k = 0; k < n; ++k) parent[k] = (int)k;
  }
  int find(int a) {
    int r = a;
    while (parent[(size_t)r] != r) r = parent[(size_t)r];
    while (parent[(size_t)a] != r) {
      const int next = parent[(size_t)a];
      parent[(size_t)a] = r;
      a = next;
    }
    return r;
  }
  void unite(int a, int b) {
    const int ra = find(a), rb = find(b);
    if (ra == rb) return;
    if (ra < rb) parent[(size_t)rb] = ra;
    else parent[(size_t)ra] = rb;
  }
};

// the number of connected components that hold no fixed node (0: the gauge is fixed everywhere)
inline size_t ungauged_components(size_t n, const int* ij_m2, size_t m, const unsigned char* fixed) {
  UnionFind uf(n);
  for (size_t e = 0; e < m; ++e) uf.unite(ij_m2[2 * e], ij_m2[2 * e + 1]);
  std::vector<unsigned char> has(n, 0);
  for (size_t k = 0; k < n; ++k)
    if (fixed[k]) has[(size_t)uf.find((int)k)] = 1;
  size_t bad = 0;
  for (size_t k = 0; k < n; ++k)
    if (uf.find((int)k) == (int)k && !has[k]) ++bad;
  return bad;
}

// the incidence lists: a counting sort by node, stable in the edge id.  offsets: n + 1 entries; entries: 2 m
inline void build_csr(size_t n, const int* ij_m2, size_t m, std::vector<int>& offsets, std::vector<int>& entries) {
  offsets.assign(n + 1, 0);
  entries.assign(2 * m, 0);
  for (size_t e = 0; e < m; ++e) {
    offsets[(size_t)ij_m2[2 * e] + 1] += 1;
    offsets[(size_t)ij_m2[2 * e + 1] + 1] += 1;
  }
  for (size_t k = 0; k < n; ++k) offsets[k + 1] += offsets[k];  // at most 2 * 2^22
  std::vector<int> fill(offsets.begin(), offsets.end() - 1);
  for (size_t e = 0; e < m; ++e)
    for (int side = 0; side < 2; ++side) entries[(size_t)fill[(size_t)ij_m2[2 * e + (size_t)side]]++] = (int)(2 * e) + side;
}

}  // namespace ngpg
