// Index structure of one pose graph solve (pose_graph.hip): which tangent columns exist, the constraints grouped by
// pose, and the (constraint, constraint) pairs of the node elimination sorted by block pair.  Host code on indices only,
// without HIP, so that it compiles alone (tests/cpp/pose_graph_structure_check.cc runs it under sanitisers).
//
// What leaves the reduced problem is Ceres' behaviour (Program::RemoveFixedBlocks of Ceres 1.13), restated, not in the
// reference's tree: constant parameter blocks, parameter blocks that no remaining residual block uses, and residual
// blocks all of whose parameter blocks are constant (their cost is the summary's fixed cost).
#ifndef DLIOM_CSRC_POSE_GRAPH_STRUCTURE_H_
#define DLIOM_CSRC_POSE_GRAPH_STRUCTURE_H_

#include <algorithm>
#include <cstdint>
#include <vector>

namespace dliom {
namespace pose_graph {

constexpr int kStructureOk = 0, kStructureBadIndex = 1, kStructureTooLarge = 2;
// tangent slots of a pose: 0..2 translation, 3..5 rotation (bit i of a mask = slot i is a column of the problem)
constexpr unsigned kTranslationBits = 7u, kRotationBits = 56u;

struct Structure {
  int num_submaps = 0, num_nodes = 0;
  int64_t num_constraints = 0;
  int reduced_dimension = 0;          // columns of the submaps' system
  std::vector<int32_t> mask;          // per pose (submaps, then nodes): the slots that are columns
  std::vector<int32_t> column;        // 6 per submap: the slot's column in the reduced system, or -1
  std::vector<int32_t> fixed;         // per constraint: 1 = all four blocks constant
  std::vector<int32_t> pose_start;    // CSR over poses (num_submaps + num_nodes + 1) ...
  std::vector<int32_t> pose_constraints;  // ... of the constraints that stay, in input order
  // block pairs (a >= b, both with columns) in (a, b) order, every (a, a) among them; their (c, c') pairs -- c on a,
  // c' on b, both on one eliminated node -- in (node, c, c') order
  std::vector<int32_t> pair_a, pair_b, pair_start, pair_c, pair_c2;
};

// submap / node: the constraints' indices (stride in int32 words).  *_constant may be null.
inline int build_structure(int num_submaps, const unsigned char* submap_constant, int gravity_aligned_submap, int num_nodes,
                           const unsigned char* node_constant, int64_t num_constraints, const int32_t* submap,
                           const int32_t* node, int64_t stride, bool fix_z, int max_reduced_dimension, Structure* out) {
  Structure& s = *out;
  s = Structure();
  s.num_submaps = num_submaps;
  s.num_nodes = num_nodes;
  s.num_constraints = num_constraints;
  if (num_constraints > INT32_MAX / 2) return kStructureTooLarge;
  for (int64_t c = 0; c < num_constraints; ++c) {
    const int32_t a = submap[c * stride], n = node[c * stride];
    if (a < 0 || a >= num_submaps || n < 0 || n >= num_nodes) return kStructureBadIndex;
  }
  const int num_poses = num_submaps + num_nodes;
  const unsigned translation = fix_z ? 3u : 7u;
  s.mask.assign(num_poses, 0);
  for (int p = 0; p < num_poses; ++p) {
    const bool is_submap = p < num_submaps;
    const unsigned char* constant = is_submap ? submap_constant : node_constant;
    if (constant != nullptr && constant[is_submap ? p : p - num_submaps] != 0) continue;
    s.mask[p] = is_submap && p == gravity_aligned_submap ? 24 : static_cast<int32_t>(translation | kRotationBits);
  }
  // constraints that stay, and the poses they use
  s.fixed.assign(num_constraints, 0);
  std::vector<int32_t> degree(num_poses + 1, 0);
  for (int64_t c = 0; c < num_constraints; ++c) {
    const int a = submap[c * stride], n = num_submaps + node[c * stride];
    if (s.mask[a] == 0 && s.mask[n] == 0) {
      s.fixed[c] = 1;
      continue;
    }
    ++degree[a];
    ++degree[n];
  }
  s.pose_start.assign(num_poses + 1, 0);
  for (int p = 0; p < num_poses; ++p) {
    s.pose_start[p + 1] = s.pose_start[p] + degree[p];
    if (degree[p] == 0) s.mask[p] = 0;  // a block that nothing uses
  }
  s.pose_constraints.assign(s.pose_start[num_poses], 0);
  std::vector<int32_t> fill(s.pose_start.begin(), s.pose_start.end() - 1);
  for (int64_t c = 0; c < num_constraints; ++c) {
    if (s.fixed[c]) continue;
    s.pose_constraints[fill[submap[c * stride]]++] = static_cast<int32_t>(c);
    s.pose_constraints[fill[num_submaps + node[c * stride]]++] = static_cast<int32_t>(c);
  }
  s.column.assign(static_cast<size_t>(num_submaps) * 6, -1);
  int64_t columns = 0;
  for (int a = 0; a < num_submaps; ++a)
    for (int i = 0; i < 6; ++i)
      if ((s.mask[a] >> i) & 1) s.column[a * 6 + i] = static_cast<int32_t>(columns++);
  s.reduced_dimension = static_cast<int>(columns);
  if (columns > max_reduced_dimension) return kStructureTooLarge;
  // the elimination's pairs
  struct Triple {
    int32_t a, b, n, c, c2;
  };
  std::vector<Triple> triples;
  for (int a = 0; a < num_submaps; ++a)
    if (s.mask[a] != 0) triples.push_back(Triple{a, a, -1, -1, -1});  // every diagonal block exists
  for (int n = 0; n < num_nodes; ++n) {
    const int p = num_submaps + n;
    if (s.mask[p] == 0) continue;
    for (int i = s.pose_start[p]; i < s.pose_start[p + 1]; ++i) {
      const int32_t c = s.pose_constraints[i];
      const int32_t a = submap[c * stride];
      if (s.mask[a] == 0) continue;
      for (int j = s.pose_start[p]; j < s.pose_start[p + 1]; ++j) {
        const int32_t c2 = s.pose_constraints[j];
        const int32_t b = submap[c2 * stride];
        if (s.mask[b] == 0 || b > a) continue;
        if (triples.size() >= static_cast<size_t>(INT32_MAX / 2)) return kStructureTooLarge;
        triples.push_back(Triple{a, b, n, c, c2});
      }
    }
  }
  std::sort(triples.begin(), triples.end(), [](const Triple& x, const Triple& y) {
    if (x.a != y.a) return x.a < y.a;
    if (x.b != y.b) return x.b < y.b;
    if (x.n != y.n) return x.n < y.n;
    if (x.c != y.c) return x.c < y.c;
    return x.c2 < y.c2;
  });
  for (size_t i = 0; i < triples.size(); ++i) {
    const Triple& t = triples[i];
    if (i == 0 || t.a != triples[i - 1].a || t.b != triples[i - 1].b) {
      s.pair_a.push_back(t.a);
      s.pair_b.push_back(t.b);
      s.pair_start.push_back(static_cast<int32_t>(s.pair_c.size()));
    }
    if (t.n < 0) continue;  // the diagonal block's marker
    s.pair_c.push_back(t.c);
    s.pair_c2.push_back(t.c2);
  }
  s.pair_start.push_back(static_cast<int32_t>(s.pair_c.size()));
  return kStructureOk;
}

}  // namespace pose_graph
}  // namespace dliom

#endif  // DLIOM_CSRC_POSE_GRAPH_STRUCTURE_H_
