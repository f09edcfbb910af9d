// Runs the pose graph's generalised host structure builder (build_structure_terms of d-liom_amd/csrc/
// pose_graph_structure.h: fixed frames behind the submaps, their constraints behind the constraints) on graphs in the
// input format of tests/cpp/pose_graph_terms_model.cc and checks its invariants; without fixed frames also that
// build_structure gives the same structure.  Built with -fsanitize=address,undefined by
// tests/test_pose_graph_terms_host.py and run as a program of its own.
// usage: pose_graph_terms_structure_check <in>...   prints one line a graph
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
    int32_t head[11];
    double reals[2];
    CHECK(std::fread(head, 4, 11, f) == 11 && std::fread(reals, 8, 2, f) == 2);
    const int submaps = head[0], N = head[1], submap_constraints = head[2], gravity = head[3], F = head[9], CF = head[10];
    const int S = submaps + F, C = submap_constraints + CF;  // kept blocks and residual blocks
    std::vector<double> poses(7 * static_cast<size_t>(S + N));
    std::vector<int32_t> constant(submaps + N);
    std::vector<Constraint> constraints(C);
    CHECK(std::fread(poses.data(), 8, poses.size(), f) == poses.size());
    CHECK(std::fread(constant.data(), 4, constant.size(), f) == constant.size());
    CHECK(std::fread(constraints.data(), sizeof(Constraint), constraints.size(), f) == constraints.size());
    std::fclose(f);
    std::vector<unsigned char> submap_constant(submaps), node_constant(N);
    for (int i = 0; i < submaps; ++i) submap_constant[i] = constant[i] != 0;
    for (int i = 0; i < N; ++i) node_constant[i] = constant[submaps + i] != 0;
    const int32_t* first = submap_constraints > 0 ? reinterpret_cast<const int32_t*>(constraints.data()) : nullptr;
    const int32_t* frame_first = CF > 0 ? reinterpret_cast<const int32_t*>(constraints.data() + submap_constraints) : nullptr;
    const int64_t stride = sizeof(Constraint) / 4;
    pg::Structure s;
    const int status = pg::build_structure_terms(submaps, submap_constant.data(), gravity, F, N, node_constant.data(),
                                                 submap_constraints, first, first != nullptr ? first + 1 : nullptr, stride, CF,
                                                 frame_first, frame_first != nullptr ? frame_first + 1 : nullptr, stride,
                                                 head[4] != 0, 8192, &s);
    if (status != pg::kStructureOk) {
      std::printf("%s status %d\n", argv[arg], status);
      continue;
    }
    if (F == 0 && CF == 0) {  // the wrapper is the same structure
      pg::Structure t;
      CHECK(pg::build_structure(submaps, submap_constant.data(), gravity, N, node_constant.data(), C, first,
                                first != nullptr ? first + 1 : nullptr, stride, head[4] != 0, 8192, &t) == pg::kStructureOk);
      CHECK(t.mask == s.mask && t.column == s.column && t.fixed == s.fixed && t.pose_start == s.pose_start &&
            t.pose_constraints == s.pose_constraints && t.pair_a == s.pair_a && t.pair_b == s.pair_b && t.pair_start == s.pair_start &&
            t.pair_c == s.pair_c && t.pair_c2 == s.pair_c2 && t.kind == s.kind && t.reduced_dimension == s.reduced_dimension);
    }
    // from here on in kept indices: a fixed-frame constraint's block follows the submaps, and no fixed frame is constant
    for (int c = submap_constraints; c < C; ++c) constraints[c].submap += submaps;
    {
      std::vector<int32_t> all(S + N, 0);
      for (int i = 0; i < submaps; ++i) all[i] = constant[i];
      for (int i = 0; i < N; ++i) all[S + i] = constant[submaps + i];
      constant.swap(all);
    }
    CHECK(s.num_submaps == submaps && s.num_fixed_frames == F && s.num_nodes == N && s.num_constraints == C);
    CHECK(static_cast<int>(s.kind.size()) == S);
    for (int a = 0; a < S; ++a) {
      CHECK(s.kind[a] == (a >= submaps ? pg::kKindYawOnly : (a == gravity ? pg::kKindConstantYaw : pg::kKindQuaternion)));
      // a fixed frame in the problem: three translation columns also under fix_z, and the yaw in slot 3
      if (a >= submaps) CHECK(s.mask[a] == 0 || s.mask[a] == 15);
      else if (s.mask[a] != 0 && a != gravity) CHECK(s.mask[a] == ((head[4] != 0 ? 3 : 7) | 56));
    }
    const int P = S + N;
    CHECK(static_cast<int>(s.mask.size()) == P && static_cast<int>(s.pose_start.size()) == P + 1);
    CHECK(static_cast<int>(s.column.size()) == 6 * S && static_cast<int>(s.fixed.size()) == C);
    int columns = 0, kept = 0;
    for (int a = 0; a < S; ++a)
      for (int i = 0; i < 6; ++i) {
        if ((s.mask[a] >> i) & 1) CHECK(s.column[a * 6 + i] == columns++);
        else CHECK(s.column[a * 6 + i] == -1);
      }
    CHECK(columns == s.reduced_dimension);
    for (int c = 0; c < C; ++c) {
      const bool fixed = (constant[constraints[c].submap] != 0) && (constant[S + constraints[c].node] != 0);
      CHECK((s.fixed[c] != 0) == fixed);
      kept += !fixed;
    }
    CHECK(s.pose_start[0] == 0 && s.pose_start[P] == 2 * kept && static_cast<int>(s.pose_constraints.size()) == 2 * kept);
    for (int p = 0; p < P; ++p) {
      CHECK(s.pose_start[p] <= s.pose_start[p + 1]);
      if (s.pose_start[p] == s.pose_start[p + 1] || constant[p] != 0) CHECK(s.mask[p] == 0);
      else CHECK(s.mask[p] != 0);
      for (int at = s.pose_start[p]; at < s.pose_start[p + 1]; ++at) {
        const int c = s.pose_constraints[at];
        CHECK(c >= 0 && c < C && !s.fixed[c]);
        CHECK(p < S ? constraints[c].submap == p : constraints[c].node == p - S);
        if (at > s.pose_start[p]) CHECK(s.pose_constraints[at - 1] < c);  // input order
      }
    }
    if (gravity >= 0 && s.mask[gravity] != 0) CHECK(s.mask[gravity] == 24);
    // the pairs: sorted, unique, every diagonal block of a submap with columns, lists on one eliminated node
    const int pairs = static_cast<int>(s.pair_a.size());
    CHECK(static_cast<int>(s.pair_start.size()) == pairs + 1 && s.pair_start[0] == 0);
    CHECK(s.pair_start[pairs] == static_cast<int>(s.pair_c.size()) && s.pair_c.size() == s.pair_c2.size());
    std::set<std::pair<int, int>> seen;
    long expected = 0;
    for (int n = 0; n < N; ++n) {
      if (s.mask[S + n] == 0) continue;
      for (int i = s.pose_start[S + n]; i < s.pose_start[S + n + 1]; ++i)
        for (int j = s.pose_start[S + n]; j < s.pose_start[S + n + 1]; ++j) {
          const int a = constraints[s.pose_constraints[i]].submap, b = constraints[s.pose_constraints[j]].submap;
          expected += s.mask[a] != 0 && s.mask[b] != 0 && a >= b;
        }
    }
    CHECK(expected == static_cast<long>(s.pair_c.size()));
    for (int k = 0; k < pairs; ++k) {
      const int a = s.pair_a[k], b = s.pair_b[k];
      CHECK(a >= b && b >= 0 && a < S && s.mask[a] != 0 && s.mask[b] != 0);
      CHECK(seen.insert(std::make_pair(a, b)).second);
      if (k > 0) CHECK(std::make_pair(s.pair_a[k - 1], s.pair_b[k - 1]) < std::make_pair(a, b));
      for (int at = s.pair_start[k]; at < s.pair_start[k + 1]; ++at) {
        const Constraint& c = constraints[s.pair_c[at]];
        const Constraint& c2 = constraints[s.pair_c2[at]];
        CHECK(c.submap == a && c2.submap == b && c.node == c2.node && s.mask[S + c.node] != 0);
      }
    }
    for (int a = 0; a < S; ++a) CHECK((seen.count(std::make_pair(a, a)) != 0) == (s.mask[a] != 0));
    std::printf("%s ok columns %d pairs %d entries %zu kept %d\n", argv[arg], s.reduced_dimension, pairs, s.pair_c.size(), kept);
  }
  return 0;
}
