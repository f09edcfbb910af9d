// Runs the pose graph's host structure builder (build_structure of d-liom_amd/csrc/pose_graph_structure.h) on graphs in
// the input format of tests/cpp/pose_graph_model.cc and checks the structure against a plain recomputation: what remains,
// the promoted nodes, the columns, the two CSR lists, the elimination's pairs and the direct terms.  Built with
// -fsanitize=address,undefined by the three tests/test_pose_graph*_host.py and run as a program of its own.
// usage: pose_graph_structure_check <in>...   prints one line a graph
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "../../d-liom_amd/csrc/pose_graph_structure.h"

namespace pg = dliom::pose_graph;

struct Constraint {
  int32_t submap, node;
  double zbar[7];
  double translation_weight, rotation_weight;
};
struct Observation {
  int32_t landmark, prev_node, next_node, pad;
  double interpolation_parameter;
  double landmark_to_tracking[7];
  double translation_weight, rotation_weight;
};
static_assert(sizeof(Observation) == 96, "the layout of dliom_pose_graph_landmark_observation");

#define CHECK(what)                                                      \
  do {                                                                   \
    if (!(what)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #what);    \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

int main(int argc, char** argv) {
  for (int arg = 1; arg < argc; ++arg) {
    FILE* f = std::fopen(argv[arg], "rb");
    CHECK(f != nullptr);
    int32_t head[13];
    double reals[2];
    CHECK(std::fread(head, 4, 13, f) == 13 && std::fread(reals, 8, 2, f) == 2);
    const int submaps = head[0], N = head[1], submap_constraints = head[2], gravity = head[3], F = head[9], CF = head[10];
    const int L = head[11], O = head[12];
    const bool fix_z = head[4] != 0;
    const int S = submaps + F, C = submap_constraints + CF;
    std::vector<double> poses(7 * static_cast<size_t>(S + N)), landmark_poses(7 * static_cast<size_t>(L));
    std::vector<int32_t> constant(submaps + N), inter_submap(submap_constraints), landmark_flags(L);
    std::vector<Constraint> constraints(C);
    std::vector<Observation> observations(O);
    CHECK(std::fread(poses.data(), 8, poses.size(), f) == poses.size());
    CHECK(std::fread(constant.data(), 4, constant.size(), f) == constant.size());
    CHECK(std::fread(constraints.data(), sizeof(Constraint), constraints.size(), f) == constraints.size());
    CHECK(std::fread(inter_submap.data(), 4, inter_submap.size(), f) == inter_submap.size());
    CHECK(std::fread(landmark_poses.data(), 8, landmark_poses.size(), f) == landmark_poses.size());
    CHECK(std::fread(landmark_flags.data(), 4, landmark_flags.size(), f) == landmark_flags.size());
    CHECK(std::fread(observations.data(), sizeof(Observation), observations.size(), f) == observations.size());
    std::fclose(f);
    std::vector<unsigned char> submap_constant(submaps), node_constant(N), landmark_constant(L);
    for (int i = 0; i < submaps; ++i) submap_constant[i] = constant[i] != 0;
    for (int i = 0; i < N; ++i) node_constant[i] = constant[submaps + i] != 0;
    for (int i = 0; i < L; ++i) landmark_constant[i] = landmark_flags[i] != 0;
    const int32_t* first = submap_constraints > 0 ? reinterpret_cast<const int32_t*>(constraints.data()) : nullptr;
    const int32_t* frame_first = CF > 0 ? reinterpret_cast<const int32_t*>(constraints.data() + submap_constraints) : nullptr;
    const int32_t* observation_first = O > 0 ? reinterpret_cast<const int32_t*>(observations.data()) : nullptr;
    const int64_t stride = sizeof(Constraint) / 4, observation_stride = sizeof(Observation) / 4;
    pg::Indices in;
    in.num_submaps = submaps, in.submap_constant = submap_constant.data(), in.gravity_aligned_submap = gravity;
    in.num_fixed_frames = F;
    in.num_nodes = N, in.node_constant = node_constant.data();
    in.num_constraints = submap_constraints, in.constraint_submap = first, in.constraint_node = first != nullptr ? first + 1 : nullptr;
    in.constraint_stride = stride;
    in.num_frame_constraints = CF, in.frame_constraint_frame = frame_first;
    in.frame_constraint_node = frame_first != nullptr ? frame_first + 1 : nullptr, in.frame_constraint_stride = stride;
    in.num_landmarks = L, in.landmark_constant = landmark_constant.data();
    in.num_observations = O, in.observation_landmark = observation_first;
    in.observation_prev = observation_first != nullptr ? observation_first + 1 : nullptr;
    in.observation_next = observation_first != nullptr ? observation_first + 2 : nullptr, in.observation_stride = observation_stride;
    in.fix_z = fix_z;
    in.max_reduced_dimension = 8192;
    pg::Structure s;
    const int status = pg::build_structure(in, &s);
    if (status != pg::kStructureOk) {
      std::printf("%s status %d\n", argv[arg], status);
      continue;
    }
    // in pose indices: submaps, fixed frames, nodes, landmarks
    const int P = S + N + L;
    for (int c = submap_constraints; c < C; ++c) constraints[c].submap += submaps;
    std::vector<int> is_constant(P, 0);
    for (int i = 0; i < submaps; ++i) is_constant[i] = constant[i] != 0;
    for (int i = 0; i < N; ++i) is_constant[S + i] = constant[submaps + i] != 0;
    for (int i = 0; i < L; ++i) is_constant[S + N + i] = landmark_flags[i] != 0;
    auto observed = [&](int o, int slot) {
      return slot == 2 ? S + N + observations[o].landmark : S + (slot == 0 ? observations[o].prev_node : observations[o].next_node);
    };
    CHECK(s.num_submaps == submaps && s.num_fixed_frames == F && s.num_nodes == N && s.num_landmarks == L && s.num_observations == O &&
          s.num_constraints == C);
    CHECK(static_cast<int>(s.mask.size()) == P && static_cast<int>(s.pose_start.size()) == P + 1 &&
          static_cast<int>(s.pose_observation_start.size()) == P + 1 && static_cast<int>(s.column.size()) == 6 * P &&
          static_cast<int>(s.node_promoted.size()) == N && static_cast<int>(s.observation_fixed.size()) == O &&
          static_cast<int>(s.fixed.size()) == C && static_cast<int>(s.kind.size()) == S);
    for (int a = 0; a < S; ++a)
      CHECK(s.kind[a] == (a >= submaps ? pg::kKindYawOnly : (a == gravity ? pg::kKindConstantYaw : pg::kKindQuaternion)));
    // what remains, recomputed
    std::vector<int> used(P, 0), promoted(N, 0);
    int kept_constraints = 0, kept_observations = 0;
    for (int c = 0; c < C; ++c) {
      const bool fixed = is_constant[constraints[c].submap] && is_constant[S + constraints[c].node];
      CHECK((s.fixed[c] != 0) == fixed);
      if (fixed) continue;
      ++kept_constraints;
      used[constraints[c].submap] = used[S + constraints[c].node] = 1;
    }
    for (int o = 0; o < O; ++o) {
      const bool fixed = is_constant[observed(o, 0)] && is_constant[observed(o, 1)] && is_constant[observed(o, 2)];
      CHECK((s.observation_fixed[o] != 0) == fixed);
      if (fixed) continue;
      ++kept_observations;
      for (int slot = 0; slot < 3; ++slot) {
        used[observed(o, slot)] = 1;
        if (slot < 2 && !is_constant[observed(o, slot)]) promoted[observed(o, slot) - S] = 1;
      }
    }
    int num_promoted = 0, columns = 0;
    for (int p = 0; p < P; ++p) {
      const bool in = used[p] && !is_constant[p];
      int want = 0;
      if (in) want = p < submaps ? (p == gravity ? 24 : ((fix_z ? 3 : 7) | 56)) : p < S ? 15 : p < S + N ? ((fix_z ? 3 : 7) | 56) : 63;
      CHECK(s.mask[p] == want);
      const bool node = p >= S && p < S + N;
      if (node) CHECK((s.node_promoted[p - S] != 0) == (promoted[p - S] != 0));
      if (node) num_promoted += promoted[p - S];
      const bool kept = !node || promoted[p - S];
      for (int i = 0; i < 6; ++i) {
        if (kept && ((s.mask[p] >> i) & 1)) CHECK(s.column[p * 6 + i] == columns++);
        else CHECK(s.column[p * 6 + i] == -1);
      }
      if (node && promoted[p - S]) CHECK(s.mask[p] != 0);  // a promoted node is in the problem
    }
    CHECK(columns == s.reduced_dimension);
    // the two CSR lists
    CHECK(s.pose_start[0] == 0 && s.pose_start[P] == 2 * kept_constraints && s.pose_observation_start[0] == 0 &&
          s.pose_observation_start[P] == 3 * kept_observations);
    CHECK(static_cast<int>(s.pose_constraints.size()) == 2 * kept_constraints && static_cast<int>(s.pose_observations.size()) == 3 * kept_observations);
    for (int p = 0; p < P; ++p) {
      CHECK(s.pose_start[p] <= s.pose_start[p + 1] && s.pose_observation_start[p] <= s.pose_observation_start[p + 1]);
      for (int at = s.pose_start[p]; at < s.pose_start[p + 1]; ++at) {
        const int c = s.pose_constraints[at];
        CHECK(c >= 0 && c < C && !s.fixed[c]);
        CHECK(p < S ? constraints[c].submap == p : S + constraints[c].node == p);
        if (at > s.pose_start[p]) CHECK(s.pose_constraints[at - 1] < c);
      }
      for (int at = s.pose_observation_start[p]; at < s.pose_observation_start[p + 1]; ++at) {
        const int entry = s.pose_observations[at];
        CHECK(entry >= 0 && entry < 3 * O && !s.observation_fixed[entry / 3] && observed(entry / 3, entry % 3) == p);
        if (at > s.pose_observation_start[p]) CHECK(s.pose_observations[at - 1] < entry);
      }
    }
    // the pairs
    const int pairs = static_cast<int>(s.pair_a.size());
    CHECK(static_cast<int>(s.pair_start.size()) == pairs + 1 && static_cast<int>(s.pair_direct_start.size()) == pairs + 1);
    CHECK(s.pair_start[0] == 0 && s.pair_direct_start[0] == 0 && s.pair_start[pairs] == static_cast<int>(s.pair_c.size()) &&
          s.pair_c.size() == s.pair_c2.size() && s.pair_direct_start[pairs] == static_cast<int>(s.pair_direct_a.size()) &&
          s.pair_direct_a.size() == s.pair_direct_b.size());
    long expected = 0, expected_direct = 0;
    for (int n = 0; n < N; ++n) {
      if (s.mask[S + n] == 0) continue;
      for (int i = s.pose_start[S + n]; i < s.pose_start[S + n + 1]; ++i) {
        const int a = constraints[s.pose_constraints[i]].submap;
        if (promoted[n]) {
          expected_direct += s.mask[a] != 0;
          continue;
        }
        for (int j = s.pose_start[S + n]; j < s.pose_start[S + n + 1]; ++j) {
          const int b = constraints[s.pose_constraints[j]].submap;
          expected += s.mask[a] != 0 && s.mask[b] != 0 && a >= b;
        }
      }
    }
    for (int o = 0; o < O; ++o) {
      if (s.observation_fixed[o]) continue;
      const int in = (s.mask[observed(o, 0)] != 0) + (s.mask[observed(o, 1)] != 0) + (s.mask[observed(o, 2)] != 0);
      expected_direct += in * (in - 1) / 2;
    }
    CHECK(expected == static_cast<long>(s.pair_c.size()) && expected_direct == static_cast<long>(s.pair_direct_a.size()));
    // the pose and the residual block of a Jacobian block index
    auto block_pose = [&](int block) {
      if (block < 2 * C) return block % 2 == 0 ? constraints[block / 2].submap : S + constraints[block / 2].node;
      return observed((block - 2 * C) / 3, (block - 2 * C) % 3);
    };
    auto block_residual = [&](int block) { return block < 2 * C ? block / 2 : C + (block - 2 * C) / 3; };
    std::set<std::pair<int, int>> seen;
    auto is_kept = [&](int p) { return p < S || p >= S + N || promoted[p - S]; };
    for (int k = 0; k < pairs; ++k) {
      const int a = s.pair_a[k], b = s.pair_b[k];
      CHECK(a >= b && b >= 0 && a < P && is_kept(a) && is_kept(b) && s.mask[a] != 0 && s.mask[b] != 0);
      CHECK(seen.insert(std::make_pair(a, b)).second);
      if (k > 0) CHECK(std::make_pair(s.pair_a[k - 1], s.pair_b[k - 1]) < std::make_pair(a, b));
      for (int at = s.pair_start[k]; at < s.pair_start[k + 1]; ++at) {
        const Constraint& c = constraints[s.pair_c[at]];
        const Constraint& c2 = constraints[s.pair_c2[at]];
        CHECK(c.submap == a && c2.submap == b && c.node == c2.node && s.mask[S + c.node] != 0 && !promoted[c.node]);
      }
      for (int at = s.pair_direct_start[k]; at < s.pair_direct_start[k + 1]; ++at) {
        const int block_a = s.pair_direct_a[at], block_b = s.pair_direct_b[at];
        CHECK(a > b && block_a >= 0 && block_b >= 0 && block_a < 2 * C + 3 * O && block_b < 2 * C + 3 * O);
        CHECK(block_pose(block_a) == a && block_pose(block_b) == b && block_residual(block_a) == block_residual(block_b));
        const int r = block_residual(block_a);
        CHECK(r < C ? !s.fixed[r] && promoted[constraints[r].node] : !s.observation_fixed[r - C]);
        if (at > s.pair_direct_start[k]) CHECK(block_residual(s.pair_direct_a[at - 1]) <= r);  // residual order
      }
    }
    for (int p = 0; p < P; ++p) CHECK((seen.count(std::make_pair(p, p)) != 0) == (is_kept(p) && s.mask[p] != 0));
    std::printf("%s ok columns %d pairs %d entries %zu kept %d direct %zu promoted %d\n", argv[arg], s.reduced_dimension, pairs,
                s.pair_c.size(), kept_constraints, s.pair_direct_a.size(), num_promoted);
  }
  return 0;
}
