// mapping::optimization::OptimizationProblem3D of dliom_cartographer.h driven through Add / Insert / Trim / Solve on a
// graph in the CPU model's input format (tests/pose_graph_common.py).  The graph's submap a becomes SubmapId{a % 2, .}
// and its node j NodeId{j % 2, .}: two trajectories, so MapById order differs from the file's order; one extra submap
// and one extra node are added and trimmed again, and one node is inserted out of order.  Output: the solved poses in
// the file's order (submaps, then nodes) and the summary's termination, iterations and final cost.
// usage: pose_graph_adapter <in> <out> [frozen trajectory]
#include <cstdio>
#include <cstdlib>

#include "dliom_cartographer.h"

namespace opt = dliom::mapping::optimization;
using dliom::mapping::NodeId;
using dliom::mapping::SubmapId;
using dliom::transform::Rigid3d;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) return 2;
  int32_t head[9];
  double radius;
  if (std::fread(head, 4, 9, f) != 9 || std::fread(&radius, 8, 1, f) != 1) return 2;
  const int S = head[0], N = head[1], C = head[2];
  std::vector<double> poses(7 * static_cast<size_t>(S + N));
  std::vector<int32_t> constant(S + N);
  std::vector<dliom_pose_graph_constraint> constraints(C);
  if (std::fread(poses.data(), 8, poses.size(), f) != poses.size() || std::fread(constant.data(), 4, constant.size(), f) != constant.size() ||
      std::fread(constraints.data(), sizeof(dliom_pose_graph_constraint), constraints.size(), f) != constraints.size())
    return 2;
  std::fclose(f);

  dliom::Context context(0);
  opt::OptimizationProblemOptions options;
  options.fix_z_in_3d = head[4] != 0;
  options.use_nonmonotonic_steps = head[5] != 0;
  options.max_num_iterations = 1;
  opt::OptimizationProblem3D problem(&context, options);
  problem.SetMaxNumIterations(head[6]);
  problem.AddImuData(0, dliom::sensor::ImuData{0, {0, 0, 9.81}, {0, 0, 0}});
  std::vector<SubmapId> submap_ids(S);
  std::vector<NodeId> node_ids(N);
  for (int a = 0; a < S; ++a) {
    submap_ids[a] = SubmapId{a % 2, a / 2};
    problem.AddSubmap(a % 2, Rigid3d::FromArray(&poses[7 * a]));
  }
  for (int j = 0; j < N; ++j) {
    node_ids[j] = NodeId{j % 2, j / 2};
    const Rigid3d pose = Rigid3d::FromArray(&poses[7 * (S + j)]);
    if (j == 5) continue;  // inserted below, out of order
    if (j > 5 && j % 2 == 1) problem.InsertTrajectoryNode(node_ids[j], opt::NodeSpec3D{j, pose, pose});
    else problem.AddTrajectoryNode(j % 2, opt::NodeSpec3D{j, pose, pose});
  }
  if (N > 5) {
    const Rigid3d pose = Rigid3d::FromArray(&poses[7 * (S + 5)]);
    problem.InsertTrajectoryNode(node_ids[5], opt::NodeSpec3D{5, pose, pose});
  }
  // one more of each at the end of trajectory 1, trimmed again
  problem.AddSubmap(1, Rigid3d());
  problem.AddTrajectoryNode(1, opt::NodeSpec3D{0, Rigid3d(), Rigid3d()});
  problem.TrimSubmap(problem.submap_data().rbegin()->first);
  problem.TrimTrajectoryNode(problem.node_data().rbegin()->first);
  if (static_cast<int>(problem.submap_data().size()) != S || static_cast<int>(problem.node_data().size()) != N) return 3;
  for (int a = 0; a < S; ++a)
    if (problem.submap_data().count(submap_ids[a]) != 1) return 3;
  for (int j = 0; j < N; ++j)
    if (problem.node_data().count(node_ids[j]) != 1) return 3;

  std::vector<opt::OptimizationProblem3D::Constraint> list;
  for (const dliom_pose_graph_constraint& c : constraints)
    list.push_back({submap_ids[c.submap], node_ids[c.node], {Rigid3d::FromArray(c.zbar), c.translation_weight, c.rotation_weight},
                    opt::OptimizationProblem3D::Constraint::INTRA_SUBMAP});
  std::set<int> frozen;
  if (argc > 3) frozen.insert(std::atoi(argv[3]));
  problem.Solve(list, frozen, {});

  FILE* o = std::fopen(argv[2], "wb");
  if (o == nullptr) return 2;
  for (int a = 0; a < S; ++a) {
    const std::array<double, 7> p = problem.submap_data().at(submap_ids[a]).global_pose.ToArray();
    std::fwrite(p.data(), 8, 7, o);
  }
  for (int j = 0; j < N; ++j) {
    const std::array<double, 7> p = problem.node_data().at(node_ids[j]).global_pose.ToArray();
    std::fwrite(p.data(), 8, 7, o);
  }
  const int32_t ints[2] = {problem.summary().termination_type, problem.summary().num_iterations};
  std::fwrite(ints, 4, 2, o);
  std::fwrite(&problem.summary().final_cost, 8, 1, o);
  std::fclose(o);
  return 0;
}
