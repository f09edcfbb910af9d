// Index structure of one pose graph solve (pose_graph.hip): which tangent columns exist, the constraints grouped by
// pose, and the (constraint, constraint) pairs of the node elimination sorted by block pair; with landmark observations
// also the nodes that move into the reduced system and the block pairs' direct terms.  Host code on indices only, without
// HIP, so that it compiles alone (tests/cpp/pose_graph_*structure_check.cc run it under sanitisers).
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
  int num_submaps = 0, num_fixed_frames = 0, num_nodes = 0;
  int64_t num_constraints = 0;        // residual blocks: the constraints, then the fixed-frame constraints
  int reduced_dimension = 0;          // columns of the kept blocks' system
  std::vector<int32_t> kind;          // per kept block (submaps, then fixed frames): kKind*
  std::vector<int32_t> mask;          // per pose (submaps, fixed frames, then nodes): the slots that are columns
  std::vector<int32_t> column;        // 6 per kept block: the slot's column in the reduced system, or -1
  std::vector<int32_t> fixed;         // per constraint: 1 = all four blocks constant
  std::vector<int32_t> pose_start;    // CSR over poses (their count + 1) ...
  std::vector<int32_t> pose_constraints;  // ... of the constraints that stay, in input order
  // block pairs (a >= b, both with columns) in (a, b) order, every (a, a) among them; their (c, c') pairs -- c on a,
  // c' on b, both on one eliminated node -- in (node, c, c') order
  std::vector<int32_t> pair_a, pair_b, pair_start, pair_c, pair_c2;
  // Landmarks (build_structure_landmarks; everything below stays empty without them).  The poses gain the landmarks
  // behind the nodes -- `mask` and `pose_start` cover them --, the kept blocks the promoted nodes and the landmarks, and
  // pair_a / pair_b are pose indices (a kept block's equal its kept index as long as it is a submap or a fixed frame).
  int num_landmarks = 0;
  int64_t num_observations = 0;
  std::vector<int32_t> node_promoted;      // per node: 1 = kept (non-constant and named by a remaining observation)
  std::vector<int32_t> pose_column;        // 6 per pose: the slot's column in the reduced system, or -1
  std::vector<int32_t> observation_fixed;  // per observation: 1 = all six blocks constant
  // CSR over the poses of the remaining observations' blocks, 3 * observation + slot (0 prev, 1 next, 2 landmark), in
  // input order
  std::vector<int32_t> pose_observation_start, pose_observations;
  // per block pair a > b: the direct terms J_a^T J_b of the residual blocks that never enter the elimination, in residual
  // order, as indices of 6 x 6 Jacobian blocks: 2 c (kept side) and 2 c + 1 (node) of constraint c, 2 C + 3 o + slot of
  // observation o
  std::vector<int32_t> pair_direct_start, pair_direct_a, pair_direct_b;
};

// Parameterisation of a kept block's rotation (rotation_parameterization.h): QuaternionParameterization, the gravity-
// aligned submap's ConstantYawQuaternionPlus (two columns), a fixed frame's YawOnlyQuaternionPlus (one column, slot 3).
constexpr int kKindQuaternion = 0, kKindConstantYaw = 1, kKindYawOnly = 2;
// a fixed frame: the translation has no parameterisation (three columns even under fix_z), the yaw is slot 3
constexpr int kFixedFrameMask = 15;

// The kept side is the submaps followed by the fixed frames; the residual blocks are the constraints followed by the
// fixed-frame constraints (frame / frame_node: their indices, frame_stride in int32 words), and that is the input order
// of every list below.  A fixed frame is never constant.  submap / node: the constraints' indices (stride in int32
// words).  *_constant may be null.
inline int build_structure_terms(int num_submaps, const unsigned char* submap_constant, int gravity_aligned_submap,
                                 int num_fixed_frames, int num_nodes, const unsigned char* node_constant,
                                 int64_t num_submap_constraints, const int32_t* submap_index, const int32_t* submap_node,
                                 int64_t stride, int64_t num_frame_constraints, const int32_t* frame, const int32_t* frame_node,
                                 int64_t frame_stride, bool fix_z, int max_reduced_dimension, Structure* out) {
  Structure& s = *out;
  s = Structure();
  s.num_submaps = num_submaps;
  s.num_fixed_frames = num_fixed_frames;
  s.num_nodes = num_nodes;
  if (num_submap_constraints > INT32_MAX / 2 || num_frame_constraints > INT32_MAX / 2 - num_submap_constraints) return kStructureTooLarge;
  const int64_t num_constraints = num_submap_constraints + num_frame_constraints;
  s.num_constraints = num_constraints;
  for (int64_t c = 0; c < num_submap_constraints; ++c) {
    const int32_t a = submap_index[c * stride], n = submap_node[c * stride];
    if (a < 0 || a >= num_submaps || n < 0 || n >= num_nodes) return kStructureBadIndex;
  }
  for (int64_t c = 0; c < num_frame_constraints; ++c) {
    const int32_t f = frame[c * frame_stride], n = frame_node[c * frame_stride];
    if (f < 0 || f >= num_fixed_frames || n < 0 || n >= num_nodes) return kStructureBadIndex;
  }
  // from here on the kept blocks take the submaps' place: kept index and node of residual block c
  const int num_kept = num_submaps + num_fixed_frames;
  auto kept = [&](int64_t c) -> int32_t {
    return c < num_submap_constraints ? submap_index[c * stride] : num_submaps + frame[(c - num_submap_constraints) * frame_stride];
  };
  auto node = [&](int64_t c) -> int32_t {
    return c < num_submap_constraints ? submap_node[c * stride] : frame_node[(c - num_submap_constraints) * frame_stride];
  };
  const int num_poses = num_kept + num_nodes;
  s.kind.assign(num_kept, kKindQuaternion);
  if (gravity_aligned_submap >= 0 && gravity_aligned_submap < num_submaps) s.kind[gravity_aligned_submap] = kKindConstantYaw;
  for (int f = 0; f < num_fixed_frames; ++f) s.kind[num_submaps + f] = kKindYawOnly;
  const unsigned translation = fix_z ? 3u : 7u;
  s.mask.assign(num_poses, 0);
  for (int p = 0; p < num_poses; ++p) {
    if (p >= num_submaps && p < num_kept) {
      s.mask[p] = kFixedFrameMask;
      continue;
    }
    const bool is_submap = p < num_submaps;
    const unsigned char* constant = is_submap ? submap_constant : node_constant;
    if (constant != nullptr && constant[is_submap ? p : p - num_kept] != 0) continue;
    s.mask[p] = is_submap && p == gravity_aligned_submap ? 24 : static_cast<int32_t>(translation | kRotationBits);
  }
  // constraints that stay, and the poses they use
  s.fixed.assign(num_constraints, 0);
  std::vector<int32_t> degree(num_poses + 1, 0);
  for (int64_t c = 0; c < num_constraints; ++c) {
    const int a = kept(c), n = num_kept + node(c);
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
    s.pose_constraints[fill[kept(c)]++] = static_cast<int32_t>(c);
    s.pose_constraints[fill[num_kept + node(c)]++] = static_cast<int32_t>(c);
  }
  s.column.assign(static_cast<size_t>(num_kept) * 6, -1);
  int64_t columns = 0;
  for (int a = 0; a < num_kept; ++a)
    for (int i = 0; i < 6; ++i)
      if ((s.mask[a] >> i) & 1) s.column[a * 6 + i] = static_cast<int32_t>(columns++);
  s.reduced_dimension = static_cast<int>(columns);
  if (columns > max_reduced_dimension) return kStructureTooLarge;
  // the elimination's pairs
  struct Triple {
    int32_t a, b, n, c, c2;
  };
  std::vector<Triple> triples;
  for (int a = 0; a < num_kept; ++a)
    if (s.mask[a] != 0) triples.push_back(Triple{a, a, -1, -1, -1});  // every diagonal block exists
  for (int n = 0; n < num_nodes; ++n) {
    const int p = num_kept + n;
    if (s.mask[p] == 0) continue;
    for (int i = s.pose_start[p]; i < s.pose_start[p + 1]; ++i) {
      const int32_t c = s.pose_constraints[i];
      const int32_t a = kept(c);
      if (s.mask[a] == 0) continue;
      for (int j = s.pose_start[p]; j < s.pose_start[p + 1]; ++j) {
        const int32_t c2 = s.pose_constraints[j];
        const int32_t b = kept(c2);
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

// The graph without fixed frames.
inline int build_structure(int num_submaps, const unsigned char* submap_constant, int gravity_aligned_submap, int num_nodes,
                           const unsigned char* node_constant, int64_t num_constraints, const int32_t* submap,
                           const int32_t* node, int64_t stride, bool fix_z, int max_reduced_dimension, Structure* out) {
  return build_structure_terms(num_submaps, submap_constant, gravity_aligned_submap, 0, num_nodes, node_constant, num_constraints,
                               submap, node, stride, 0, nullptr, nullptr, 1, fix_z, max_reduced_dimension, out);
}

// The graph with landmark observations (optimization_problem_3d.cc:124-186): observation o couples the nodes prev[o] and
// next[o] (different) with landmark[o] (stride in int32 words).  A landmark block has six columns also under fix_z (its
// translation has no parameterisation); landmark_constant may be null.  The kept blocks become the submaps, the fixed
// frames, the promoted nodes and the non-constant landmarks, in that order; every other node stays eliminated.  Residual
// blocks: the constraints, the fixed-frame constraints, then the observations.  Without landmarks and observations this
// is build_structure_terms.
inline int build_structure_landmarks(int num_submaps, const unsigned char* submap_constant, int gravity_aligned_submap,
                                     int num_fixed_frames, int num_nodes, const unsigned char* node_constant,
                                     int64_t num_submap_constraints, const int32_t* submap_index, const int32_t* submap_node,
                                     int64_t stride, int64_t num_frame_constraints, const int32_t* frame, const int32_t* frame_node,
                                     int64_t frame_stride, int num_landmarks, const unsigned char* landmark_constant,
                                     int64_t num_observations, const int32_t* observation_landmark, const int32_t* observation_prev,
                                     const int32_t* observation_next, int64_t observation_stride, bool fix_z,
                                     int max_reduced_dimension, Structure* out) {
  if (num_landmarks == 0 && num_observations == 0)
    return build_structure_terms(num_submaps, submap_constant, gravity_aligned_submap, num_fixed_frames, num_nodes, node_constant,
                                 num_submap_constraints, submap_index, submap_node, stride, num_frame_constraints, frame, frame_node,
                                 frame_stride, fix_z, max_reduced_dimension, out);
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
    const int32_t a = submap_index[c * stride], n = submap_node[c * stride];
    if (a < 0 || a >= num_submaps || n < 0 || n >= num_nodes) return kStructureBadIndex;
  }
  for (int64_t c = 0; c < num_frame_constraints; ++c) {
    const int32_t f = frame[c * frame_stride], n = frame_node[c * frame_stride];
    if (f < 0 || f >= num_fixed_frames || n < 0 || n >= num_nodes) return kStructureBadIndex;
  }
  for (int64_t o = 0; o < num_observations; ++o) {
    const int32_t l = observation_landmark[o * observation_stride], p = observation_prev[o * observation_stride],
                  n = observation_next[o * observation_stride];
    if (l < 0 || l >= num_landmarks || p < 0 || p >= num_nodes || n < 0 || n >= num_nodes || p == n) return kStructureBadIndex;
  }
  const int num_kept = num_submaps + num_fixed_frames;
  const int first_landmark = num_kept + num_nodes;
  if (num_landmarks > INT32_MAX / 72 - first_landmark) return kStructureTooLarge;
  const int num_poses = first_landmark + num_landmarks;
  auto kept = [&](int64_t c) -> int32_t {
    return c < num_submap_constraints ? submap_index[c * stride] : num_submaps + frame[(c - num_submap_constraints) * frame_stride];
  };
  auto node = [&](int64_t c) -> int32_t {
    return c < num_submap_constraints ? submap_node[c * stride] : frame_node[(c - num_submap_constraints) * frame_stride];
  };
  // the pose of an observation's slot
  auto observed = [&](int64_t o, int slot) -> int32_t {
    if (slot == 2) return first_landmark + observation_landmark[o * observation_stride];
    return num_kept + (slot == 0 ? observation_prev : observation_next)[o * observation_stride];
  };
  s.kind.assign(num_kept, kKindQuaternion);
  if (gravity_aligned_submap >= 0 && gravity_aligned_submap < num_submaps) s.kind[gravity_aligned_submap] = kKindConstantYaw;
  for (int f = 0; f < num_fixed_frames; ++f) s.kind[num_submaps + f] = kKindYawOnly;
  const unsigned translation = fix_z ? 3u : 7u;
  s.mask.assign(num_poses, 0);
  for (int p = 0; p < num_poses; ++p) {
    if (p >= num_submaps && p < num_kept) {
      s.mask[p] = kFixedFrameMask;
    } else if (p >= first_landmark) {
      if (landmark_constant == nullptr || landmark_constant[p - first_landmark] == 0) s.mask[p] = static_cast<int32_t>(kTranslationBits | kRotationBits);
    } else {
      const bool is_submap = p < num_submaps;
      const unsigned char* constant = is_submap ? submap_constant : node_constant;
      if (constant != nullptr && constant[is_submap ? p : p - num_kept] != 0) continue;
      s.mask[p] = is_submap && p == gravity_aligned_submap ? 24 : static_cast<int32_t>(translation | kRotationBits);
    }
  }
  // residual blocks that stay, and the poses they use
  s.fixed.assign(num_constraints, 0);
  s.observation_fixed.assign(num_observations, 0);
  s.node_promoted.assign(num_nodes, 0);
  std::vector<int32_t> degree(num_poses, 0), observation_degree(num_poses, 0);
  for (int64_t c = 0; c < num_constraints; ++c) {
    const int a = kept(c), n = num_kept + node(c);
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
      if (slot < 2 && s.mask[p] != 0) s.node_promoted[p - num_kept] = 1;
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
    s.pose_constraints[fill[num_kept + node(c)]++] = static_cast<int32_t>(c);
  }
  fill.assign(s.pose_observation_start.begin(), s.pose_observation_start.end() - 1);
  for (int64_t o = 0; o < num_observations; ++o) {
    if (s.observation_fixed[o]) continue;
    for (int slot = 0; slot < 3; ++slot) s.pose_observations[fill[observed(o, slot)]++] = static_cast<int32_t>(3 * o + slot);
  }
  // columns: submaps, fixed frames, promoted nodes, landmarks -- which is the poses' order with the other nodes left out
  s.column.assign(static_cast<size_t>(num_kept) * 6, -1);
  s.pose_column.assign(static_cast<size_t>(num_poses) * 6, -1);
  int64_t columns = 0;
  for (int p = 0; p < num_poses; ++p) {
    if (p >= num_kept && p < first_landmark && s.node_promoted[p - num_kept] == 0) continue;
    for (int i = 0; i < 6; ++i)
      if ((s.mask[p] >> i) & 1) s.pose_column[static_cast<size_t>(p) * 6 + i] = static_cast<int32_t>(columns++);
  }
  std::copy(s.pose_column.begin(), s.pose_column.begin() + static_cast<size_t>(num_kept) * 6, s.column.begin());
  s.reduced_dimension = static_cast<int>(std::min<int64_t>(columns, INT32_MAX));
  if (columns > max_reduced_dimension) return kStructureTooLarge;
  auto is_kept = [&](int p) { return p < num_kept || p >= first_landmark || s.node_promoted[p - num_kept] != 0; };
  // the pairs: kind 0 the diagonal block's marker, 1 an elimination term (order: node, c, c'), 2 a direct term (order: its
  // residual block)
  struct Term {
    int32_t a, b, kind, order, c, c2;
  };
  std::vector<Term> terms;
  auto push = [&terms](const Term& t) {
    if (terms.size() >= static_cast<size_t>(INT32_MAX / 2)) return false;
    terms.push_back(t);
    return true;
  };
  for (int p = 0; p < num_poses; ++p)
    if (is_kept(p) && s.mask[p] != 0) terms.push_back(Term{p, p, 0, -1, -1, -1});
  for (int n = 0; n < num_nodes; ++n) {
    const int p = num_kept + n;
    if (s.mask[p] == 0) continue;
    for (int i = s.pose_start[p]; i < s.pose_start[p + 1]; ++i) {
      const int32_t c = s.pose_constraints[i];
      const int32_t a = kept(c);
      if (s.mask[a] == 0) continue;
      if (s.node_promoted[n] != 0) {  // class (ii): the node's block lies behind every submap and fixed frame
        if (!push(Term{p, a, 2, c, 2 * c + 1, 2 * c})) return kStructureTooLarge;
        continue;
      }
      for (int j = s.pose_start[p]; j < s.pose_start[p + 1]; ++j) {
        const int32_t c2 = s.pose_constraints[j];
        const int32_t b = kept(c2);
        if (s.mask[b] == 0 || b > a) continue;
        if (!push(Term{a, b, 1, n, c, c2})) return kStructureTooLarge;
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
        if (!push(Term{a, b, 2, static_cast<int32_t>(num_constraints + o), base + x, base + y})) return kStructureTooLarge;
      }
  }
  std::sort(terms.begin(), terms.end(), [](const Term& x, const Term& y) {
    if (x.a != y.a) return x.a < y.a;
    if (x.b != y.b) return x.b < y.b;
    if (x.kind != y.kind) return x.kind < y.kind;
    if (x.order != y.order) return x.order < y.order;
    if (x.c != y.c) return x.c < y.c;
    return x.c2 < y.c2;
  });
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
