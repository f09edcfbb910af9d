// Index structure of one pose graph solve (pose_graph.hip): which tangent columns exist, the residual blocks grouped by
// pose, the (constraint, constraint) pairs of the node elimination sorted by block pair, the nodes that landmark
// observations move into the reduced system and the block pairs' direct terms.  Host code on indices only, without HIP,
// so that it compiles alone (tests/cpp/pose_graph_structure_check.cc runs it under sanitisers).
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

// Parameterisation of a submap's or a fixed frame's rotation (rotation_parameterization.h): QuaternionParameterization,
// the gravity-aligned submap's ConstantYawQuaternionPlus (two columns), a fixed frame's YawOnlyQuaternionPlus (one
// column, slot 3).
constexpr int kKindQuaternion = 0, kKindConstantYaw = 1, kKindYawOnly = 2;
// a fixed frame: the translation has no parameterisation (three columns even under fix_z), the yaw is slot 3
constexpr int kFixedFrameMask = 15;

// The graph's indices.  The poses are the submaps, the fixed frames, the nodes and the landmarks, in that order; the
// residual blocks are the constraints, the fixed-frame constraints and the landmark observations, in that order, and
// that is the input order of every list of a Structure.  Every index array is read with its stride, in int32 words; an
// array of no entries and a *_constant may be null.  A fixed frame is never constant.  Observation o couples the nodes
// observation_prev[o] and observation_next[o] (different) with observation_landmark[o] (optimization_problem_3d.cc:
// 124-186).
struct Indices {
  int num_submaps = 0;
  const unsigned char* submap_constant = nullptr;
  int gravity_aligned_submap = -1;
  int num_fixed_frames = 0;
  int num_nodes = 0;
  const unsigned char* node_constant = nullptr;
  int64_t num_constraints = 0;
  const int32_t *constraint_submap = nullptr, *constraint_node = nullptr;
  int64_t constraint_stride = 1;
  int64_t num_frame_constraints = 0;
  const int32_t *frame_constraint_frame = nullptr, *frame_constraint_node = nullptr;
  int64_t frame_constraint_stride = 1;
  int num_landmarks = 0;
  const unsigned char* landmark_constant = nullptr;
  int64_t num_observations = 0;
  const int32_t *observation_landmark = nullptr, *observation_prev = nullptr, *observation_next = nullptr;
  int64_t observation_stride = 1;
  bool fix_z = false;
  int max_reduced_dimension = 0;
};

// The kept blocks -- the poses with columns in the reduced system -- are the submaps, the fixed frames, the promoted
// nodes and the non-constant landmarks, in the poses' order; every other node is eliminated.
struct Structure {
  int num_submaps = 0, num_fixed_frames = 0, num_nodes = 0, num_landmarks = 0;
  int64_t num_constraints = 0;        // the constraints and the fixed-frame constraints
  int64_t num_observations = 0;
  int reduced_dimension = 0;          // columns of the kept blocks' system
  std::vector<int32_t> kind;          // per submap and fixed frame: kKind*
  std::vector<int32_t> mask;          // per pose: the slots that are columns
  // 6 per pose: the slot's column in the reduced system, or -1.  The submaps and the fixed frames come first, so without
  // promoted nodes and landmarks the first 6 * (num_submaps + num_fixed_frames) entries hold every column.
  std::vector<int32_t> column;
  std::vector<int32_t> node_promoted;      // per node: 1 = kept (non-constant and named by a remaining observation)
  std::vector<int32_t> fixed;              // per constraint: 1 = all four blocks constant
  std::vector<int32_t> observation_fixed;  // per observation: 1 = all six blocks constant
  std::vector<int32_t> pose_start;         // CSR over poses (their count + 1) ...
  std::vector<int32_t> pose_constraints;   // ... of the constraints that stay, in input order
  // CSR over the poses of the remaining observations' blocks, 3 * observation + slot (0 prev, 1 next, 2 landmark), in
  // input order
  std::vector<int32_t> pose_observation_start, pose_observations;
  // block pairs (a >= b, pose indices of kept blocks with columns) in (a, b) order, every (a, a) among them; their
  // (c, c') pairs -- c on a, c' on b, both on one eliminated node -- in (node, c, c') order
  std::vector<int32_t> pair_a, pair_b, pair_start, pair_c, pair_c2;
  // per block pair a > b: the direct terms J_a^T J_b of the residual blocks that never enter the elimination, in residual
  // order, as indices of 6 x 6 Jacobian blocks: 2 c (kept side) and 2 c + 1 (node) of constraint c, 2 C + 3 o + slot of
  // observation o
  std::vector<int32_t> pair_direct_start, pair_direct_a, pair_direct_b;
};

// A landmark block has six columns also under fix_z (its translation has no parameterisation).
inline int build_structure(const Indices& in, Structure* out) {
  const int num_submaps = in.num_submaps, num_fixed_frames = in.num_fixed_frames, num_nodes = in.num_nodes,
            num_landmarks = in.num_landmarks;
  const int64_t num_submap_constraints = in.num_constraints, num_frame_constraints = in.num_frame_constraints,
                num_observations = in.num_observations;
  Structure& s = *out;
  s = Structure();
  s.num_submaps = num_submaps;
  s.num_fixed_frames = num_fixed_frames;
  s.num_nodes = num_nodes;
  s.num_landmarks = num_landmarks;
  s.num_observations = num_observations;
  if (num_submap_constraints > INT32_MAX / 2 || num_frame_constraints > INT32_MAX / 2 - num_submap_constraints) return kStructureTooLarge;
  const int64_t num_constraints = num_submap_constraints + num_frame_constraints;
  if (num_observations > (INT32_MAX - 2 * num_constraints) / 3) return kStructureTooLarge;
  s.num_constraints = num_constraints;
  for (int64_t c = 0; c < num_submap_constraints; ++c) {
    const int32_t a = in.constraint_submap[c * in.constraint_stride], n = in.constraint_node[c * in.constraint_stride];
    if (a < 0 || a >= num_submaps || n < 0 || n >= num_nodes) return kStructureBadIndex;
  }
  for (int64_t c = 0; c < num_frame_constraints; ++c) {
    const int32_t f = in.frame_constraint_frame[c * in.frame_constraint_stride], n = in.frame_constraint_node[c * in.frame_constraint_stride];
    if (f < 0 || f >= num_fixed_frames || n < 0 || n >= num_nodes) return kStructureBadIndex;
  }
  for (int64_t o = 0; o < num_observations; ++o) {
    const int32_t l = in.observation_landmark[o * in.observation_stride], p = in.observation_prev[o * in.observation_stride],
                  n = in.observation_next[o * in.observation_stride];
    if (l < 0 || l >= num_landmarks || p < 0 || p >= num_nodes || n < 0 || n >= num_nodes || p == n) return kStructureBadIndex;
  }
  // from here on in pose indices: the submap or fixed frame and the node of residual block c
  const int first_node = num_submaps + num_fixed_frames;
  const int first_landmark = first_node + num_nodes;
  if (num_landmarks > INT32_MAX / 72 - first_landmark) return kStructureTooLarge;
  const int num_poses = first_landmark + num_landmarks;
  auto kept = [&](int64_t c) -> int32_t {
    return c < num_submap_constraints ? in.constraint_submap[c * in.constraint_stride]
                                      : num_submaps + in.frame_constraint_frame[(c - num_submap_constraints) * in.frame_constraint_stride];
  };
  auto node = [&](int64_t c) -> int32_t {
    return first_node + (c < num_submap_constraints ? in.constraint_node[c * in.constraint_stride]
                                                    : in.frame_constraint_node[(c - num_submap_constraints) * in.frame_constraint_stride]);
  };
  // the pose of an observation's slot
  auto observed = [&](int64_t o, int slot) -> int32_t {
    if (slot == 2) return first_landmark + in.observation_landmark[o * in.observation_stride];
    return first_node + (slot == 0 ? in.observation_prev : in.observation_next)[o * in.observation_stride];
  };
  s.kind.assign(first_node, kKindQuaternion);
  if (in.gravity_aligned_submap >= 0 && in.gravity_aligned_submap < num_submaps) s.kind[in.gravity_aligned_submap] = kKindConstantYaw;
  for (int f = 0; f < num_fixed_frames; ++f) s.kind[num_submaps + f] = kKindYawOnly;
  const unsigned translation = in.fix_z ? 3u : 7u;
  s.mask.assign(num_poses, 0);
  for (int p = 0; p < num_poses; ++p) {
    if (p >= num_submaps && p < first_node) {
      s.mask[p] = kFixedFrameMask;
    } else if (p >= first_landmark) {
      if (in.landmark_constant == nullptr || in.landmark_constant[p - first_landmark] == 0) s.mask[p] = static_cast<int32_t>(kTranslationBits | kRotationBits);
    } else {
      const bool is_submap = p < num_submaps;
      const unsigned char* constant = is_submap ? in.submap_constant : in.node_constant;
      if (constant != nullptr && constant[is_submap ? p : p - first_node] != 0) continue;
      s.mask[p] = is_submap && p == in.gravity_aligned_submap ? 24 : static_cast<int32_t>(translation | kRotationBits);
    }
  }
  // residual blocks that stay, and the poses they use
  s.fixed.assign(num_constraints, 0);
  s.observation_fixed.assign(num_observations, 0);
  s.node_promoted.assign(num_nodes, 0);
  std::vector<int32_t> degree(num_poses, 0), observation_degree(num_poses, 0);
  for (int64_t c = 0; c < num_constraints; ++c) {
    const int a = kept(c), n = node(c);
    if (s.mask[a] == 0 && s.mask[n] == 0) {
      s.fixed[c] = 1;
      continue;
    }
    ++degree[a];
    ++degree[n];
  }
  for (int64_t o = 0; o < num_observations; ++o) {
    if (s.mask[observed(o, 0)] == 0 && s.mask[observed(o, 1)] == 0 && s.mask[observed(o, 2)] == 0) {
      s.observation_fixed[o] = 1;
      continue;
    }
    for (int slot = 0; slot < 3; ++slot) {
      const int p = observed(o, slot);
      ++observation_degree[p];
      if (slot < 2 && s.mask[p] != 0) s.node_promoted[p - first_node] = 1;
    }
  }
  s.pose_start.assign(num_poses + 1, 0);
  s.pose_observation_start.assign(num_poses + 1, 0);
  for (int p = 0; p < num_poses; ++p) {
    s.pose_start[p + 1] = s.pose_start[p] + degree[p];
    s.pose_observation_start[p + 1] = s.pose_observation_start[p] + observation_degree[p];
    if (degree[p] == 0 && observation_degree[p] == 0) s.mask[p] = 0;  // a block that nothing uses
  }
  s.pose_constraints.assign(s.pose_start[num_poses], 0);
  s.pose_observations.assign(s.pose_observation_start[num_poses], 0);
  std::vector<int32_t> fill(s.pose_start.begin(), s.pose_start.end() - 1);
  for (int64_t c = 0; c < num_constraints; ++c) {
    if (s.fixed[c]) continue;
    s.pose_constraints[fill[kept(c)]++] = static_cast<int32_t>(c);
    s.pose_constraints[fill[node(c)]++] = static_cast<int32_t>(c);
  }
  fill.assign(s.pose_observation_start.begin(), s.pose_observation_start.end() - 1);
  for (int64_t o = 0; o < num_observations; ++o) {
    if (s.observation_fixed[o]) continue;
    for (int slot = 0; slot < 3; ++slot) s.pose_observations[fill[observed(o, slot)]++] = static_cast<int32_t>(3 * o + slot);
  }
  // columns: submaps, fixed frames, promoted nodes, landmarks -- which is the poses' order with the other nodes left out
  auto is_kept = [&](int p) { return p < first_node || p >= first_landmark || s.node_promoted[p - first_node] != 0; };
  s.column.assign(static_cast<size_t>(num_poses) * 6, -1);
  int64_t columns = 0;
  for (int p = 0; p < num_poses; ++p) {
    if (!is_kept(p)) continue;
    for (int i = 0; i < 6; ++i)
      if ((s.mask[p] >> i) & 1) s.column[static_cast<size_t>(p) * 6 + i] = static_cast<int32_t>(columns++);
  }
  s.reduced_dimension = static_cast<int>(std::min<int64_t>(columns, INT32_MAX));
  if (columns > in.max_reduced_dimension) return kStructureTooLarge;
  // the pairs: kind 0 the diagonal block's marker, 1 an elimination term, 2 a direct term.  They are made in the order
  // the lists have inside one block pair -- the marker first, the elimination terms by (node, c, c'), the direct terms by
  // residual block; a pair has terms of one kind only, an eliminated node's pairs being among submaps and fixed frames and
  // a direct term's a being a promoted node or a landmark --, so that a stable sort by block pair is all that is left.
  struct Term {
    int32_t a, b, kind, c, c2;
  };
  std::vector<Term> terms;
  auto push = [&terms](const Term& t) {
    if (terms.size() >= static_cast<size_t>(INT32_MAX / 2)) return false;
    terms.push_back(t);
    return true;
  };
  for (int p = 0; p < num_poses; ++p)
    if (is_kept(p) && s.mask[p] != 0) terms.push_back(Term{p, p, 0, -1, -1});
  for (int n = 0; n < num_nodes; ++n) {
    const int p = first_node + n;
    if (s.mask[p] == 0) continue;
    for (int i = s.pose_start[p]; i < s.pose_start[p + 1]; ++i) {
      const int32_t c = s.pose_constraints[i];
      const int32_t a = kept(c);
      if (s.mask[a] == 0) continue;
      if (s.node_promoted[n] != 0) {  // a direct term: the node's block lies behind every submap and fixed frame
        if (!push(Term{p, a, 2, 2 * c + 1, 2 * c})) return kStructureTooLarge;
        continue;
      }
      for (int j = s.pose_start[p]; j < s.pose_start[p + 1]; ++j) {
        const int32_t c2 = s.pose_constraints[j];
        const int32_t b = kept(c2);
        if (s.mask[b] == 0 || b > a) continue;
        if (!push(Term{a, b, 1, c, c2})) return kStructureTooLarge;
      }
    }
  }
  for (int64_t o = 0; o < num_observations; ++o) {
    if (s.observation_fixed[o]) continue;
    for (int x = 0; x < 3; ++x)
      for (int y = 0; y < 3; ++y) {
        const int32_t a = observed(o, x), b = observed(o, y);
        if (a <= b || s.mask[a] == 0 || s.mask[b] == 0) continue;
        const int32_t base = static_cast<int32_t>(2 * num_constraints + 3 * o);
        if (!push(Term{a, b, 2, base + x, base + y})) return kStructureTooLarge;
      }
  }
  std::stable_sort(terms.begin(), terms.end(), [](const Term& x, const Term& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
  for (size_t i = 0; i < terms.size(); ++i) {
    const Term& t = terms[i];
    if (i == 0 || t.a != terms[i - 1].a || t.b != terms[i - 1].b) {
      s.pair_a.push_back(t.a);
      s.pair_b.push_back(t.b);
      s.pair_start.push_back(static_cast<int32_t>(s.pair_c.size()));
      s.pair_direct_start.push_back(static_cast<int32_t>(s.pair_direct_a.size()));
    }
    if (t.kind == 1) {
      s.pair_c.push_back(t.c);
      s.pair_c2.push_back(t.c2);
    } else if (t.kind == 2) {
      s.pair_direct_a.push_back(t.c);
      s.pair_direct_b.push_back(t.c2);
    }
  }
  s.pair_start.push_back(static_cast<int32_t>(s.pair_c.size()));
  s.pair_direct_start.push_back(static_cast<int32_t>(s.pair_direct_a.size()));
  return kStructureOk;
}

}  // namespace pose_graph
}  // namespace dliom

#endif  // DLIOM_CSRC_POSE_GRAPH_STRUCTURE_H_
