// mapping::optimization::OptimizationProblem3D of dliom_cartographer.h with landmark nodes (options.use_landmarks).  In: a
// graph in the CPU model's input format (tests/pose_graph_common.py), and behind it int32 frozen trajectory (-1: none),
// int32 extra (1: trajectory 2 gets one node, at time 1000, that nothing constrains), int32 landmarks, and a landmark:
// int32 has_global_pose, double pose[7], int32 observations, each int32 trajectory, int64 time, double
// landmark_to_tracking[7], double translation_weight, rotation_weight.  Landmark l is "landmark%03d".  As in
// pose_graph_adapter.cc submap a becomes SubmapId{a % 2, .} and node j NodeId{j % 2, .}; node j's time is 1000 + j * 10^7
// ticks.
//   --host <in> <out>  no context: CompactLandmarks alone -> int32 landmarks, observations; the start poses; the constant
//                      flags as int32; an observation: int32 landmark, prev_node, next_node, double t,
//                      landmark_to_tracking[7], the weights
//   <in> <out>         Solve -> the poses in the file's order, int32 landmarks in landmark_data(), their poses in the
//                      map's order, int32 termination, iterations, double final cost
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dliom_cartographer.h"

namespace opt = dliom::mapping::optimization;
using dliom::mapping::NodeId;
using dliom::mapping::SubmapId;
using dliom::transform::Rigid3d;

int main(int argc, char** argv) {
  const bool host_only = argc == 4 && std::string(argv[1]) == "--host";
  if (!host_only && argc != 3) return 2;
  FILE* f = std::fopen(argv[host_only ? 2 : 1], "rb");
  if (f == nullptr) return 2;
  int32_t head[9];
  double radius;
  if (std::fread(head, 4, 9, f) != 9 || std::fread(&radius, 8, 1, f) != 1) return 2;
  const int S = head[0], N = head[1], C = head[2];
  std::vector<double> poses(7 * static_cast<size_t>(S + N));
  std::vector<int32_t> constant(S + N);
  std::vector<dliom_pose_graph_constraint> constraints(C);
  int32_t tail[3];
  if (std::fread(poses.data(), 8, poses.size(), f) != poses.size() || std::fread(constant.data(), 4, constant.size(), f) != constant.size() ||
      std::fread(constraints.data(), sizeof(dliom_pose_graph_constraint), constraints.size(), f) != constraints.size() ||
      std::fread(tail, 4, 3, f) != 3)
    return 2;
  std::map<std::string, opt::LandmarkNode> landmark_nodes;
  for (int l = 0; l < tail[2]; ++l) {
    int32_t has_pose, count;
    double pose[7];
    if (std::fread(&has_pose, 4, 1, f) != 1 || std::fread(pose, 8, 7, f) != 7 || std::fread(&count, 4, 1, f) != 1) return 2;
    char name[32];
    std::snprintf(name, sizeof(name), "landmark%03d", l);
    opt::LandmarkNode& node = landmark_nodes[name];
    if (has_pose != 0) node.global_landmark_pose = Rigid3d::FromArray(pose);
    for (int i = 0; i < count; ++i) {
      int32_t trajectory;
      int64_t time;
      double z[7], weights[2];
      if (std::fread(&trajectory, 4, 1, f) != 1 || std::fread(&time, 8, 1, f) != 1 || std::fread(z, 8, 7, f) != 7 || std::fread(weights, 8, 2, f) != 2)
        return 2;
      node.landmark_observations.push_back({trajectory, time, Rigid3d::FromArray(z), weights[0], weights[1]});
    }
  }
  std::fclose(f);
  std::set<int> frozen;
  if (tail[0] >= 0) frozen.insert(tail[0]);

  std::unique_ptr<dliom::Context> context;
  if (!host_only) context.reset(new dliom::Context(0));
  opt::OptimizationProblemOptions options;
  options.fix_z_in_3d = head[4] != 0;
  options.use_nonmonotonic_steps = head[5] != 0;
  options.max_num_iterations = head[6];
  options.use_landmarks = true;
  opt::OptimizationProblem3D problem(context.get(), options);
  std::vector<SubmapId> submap_ids(S);
  std::vector<NodeId> node_ids(N);
  for (int a = 0; a < S; ++a) {
    submap_ids[a] = SubmapId{a % 2, a / 2};
    problem.AddSubmap(a % 2, Rigid3d::FromArray(&poses[7 * a]));
  }
  for (int j = 0; j < N; ++j) {
    node_ids[j] = NodeId{j % 2, j / 2};
    const Rigid3d pose = Rigid3d::FromArray(&poses[7 * (S + j)]);
    problem.AddTrajectoryNode(j % 2, opt::NodeSpec3D{1000 + j * int64_t{10000000}, pose, pose});
  }
  if (tail[1] != 0) problem.AddTrajectoryNode(2, opt::NodeSpec3D{1000, Rigid3d(), Rigid3d()});
  FILE* o = std::fopen(argv[host_only ? 3 : 2], "wb");
  if (o == nullptr) return 2;
  if (host_only) {
    const opt::OptimizationProblem3D::LandmarkBlocks blocks = problem.CompactLandmarks(frozen, landmark_nodes);
    const int32_t counts[2] = {static_cast<int32_t>(blocks.ids.size()), static_cast<int32_t>(blocks.observations.size())};
    std::fwrite(counts, 4, 2, o);
    std::fwrite(blocks.poses.data(), 8, blocks.poses.size(), o);
    for (unsigned char flag : blocks.constant) {
      const int32_t value = flag;
      std::fwrite(&value, 4, 1, o);
    }
    for (const dliom_pose_graph_landmark_observation& k : blocks.observations) {
      const int32_t ints[3] = {k.landmark, k.prev_node, k.next_node};
      std::fwrite(ints, 4, 3, o);
      std::fwrite(&k.interpolation_parameter, 8, 1, o);
      std::fwrite(k.landmark_to_tracking7, 8, 7, o);
      std::fwrite(&k.translation_weight, 8, 1, o);
      std::fwrite(&k.rotation_weight, 8, 1, o);
    }
    std::fclose(o);
    return 0;
  }
  std::vector<opt::OptimizationProblem3D::Constraint> list;
  for (int c = 0; c < C; ++c)
    list.push_back({submap_ids[constraints[c].submap], node_ids[constraints[c].node],
                    {Rigid3d::FromArray(constraints[c].zbar), constraints[c].translation_weight, constraints[c].rotation_weight},
                    opt::OptimizationProblem3D::Constraint::INTRA_SUBMAP});
  problem.Solve(list, frozen, landmark_nodes);
  for (int a = 0; a < S; ++a) {
    const std::array<double, 7> p = problem.submap_data().at(submap_ids[a]).global_pose.ToArray();
    std::fwrite(p.data(), 8, 7, o);
  }
  for (int j = 0; j < N; ++j) {
    const std::array<double, 7> p = problem.node_data().at(node_ids[j]).global_pose.ToArray();
    std::fwrite(p.data(), 8, 7, o);
  }
  const int32_t count = static_cast<int32_t>(problem.landmark_data().size());
  std::fwrite(&count, 4, 1, o);
  for (const auto& id_pose : problem.landmark_data()) {
    const std::array<double, 7> p = id_pose.second.ToArray();
    std::fwrite(p.data(), 8, 7, o);
  }
  const int32_t ints[2] = {problem.summary().termination_type, problem.summary().num_iterations};
  std::fwrite(ints, 4, 2, o);
  std::fwrite(&problem.summary().final_cost, 8, 1, o);
  std::fclose(o);
  return 0;
}
