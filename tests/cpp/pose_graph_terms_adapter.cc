// mapping::optimization::OptimizationProblem3D of dliom_cartographer.h with fixed-frame pose data, tagged constraints
// and a loss.  In: a graph in the CPU model's input format (tests/pose_graph_common.py), and behind it int32
// inter_submap[C], double huber_scale, and for trajectories 0 and 1 an int32 count of fixed-frame samples, each int64
// time, int32 has_pose, double pose[7].  As in pose_graph_adapter.cc submap a becomes SubmapId{a % 2, .} and node j
// NodeId{j % 2, .}; node j's time is 1000 + j * 10^7 ticks.  Solve runs twice -- the second starts from the stored
// fixed_frame_origin_in_map -- and each time the poses in the file's order, then for either trajectory an int32 "has an
// origin" and the origin, then termination, iterations and final cost are written.  With --landmark it only calls Solve with a
// landmark on a problem without a context: the refusal is Check's abort, before anything touches a device.
// usage: pose_graph_terms_adapter <in> <out> | pose_graph_terms_adapter --landmark
#include <cstdio>
#include <cstdlib>

#include "dliom_cartographer.h"

namespace opt = dliom::mapping::optimization;
using dliom::mapping::NodeId;
using dliom::mapping::SubmapId;
using dliom::transform::Rigid3d;

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--landmark") {
    opt::OptimizationProblem3D problem(nullptr, opt::OptimizationProblemOptions());
    problem.AddSubmap(0, Rigid3d());
    problem.AddTrajectoryNode(0, opt::NodeSpec3D{0, Rigid3d(), Rigid3d()});
    problem.Solve({}, {}, {{"landmark", opt::LandmarkNode{}}});
    return 0;  // not reached
  }
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) return 2;
  int32_t head[9];
  double radius, huber_scale;
  if (std::fread(head, 4, 9, f) != 9 || std::fread(&radius, 8, 1, f) != 1) return 2;
  const int S = head[0], N = head[1], C = head[2];
  std::vector<double> poses(7 * static_cast<size_t>(S + N));
  std::vector<int32_t> constant(S + N), inter_submap(C);
  std::vector<dliom_pose_graph_constraint> constraints(C);
  if (std::fread(poses.data(), 8, poses.size(), f) != poses.size() || std::fread(constant.data(), 4, constant.size(), f) != constant.size() ||
      std::fread(constraints.data(), sizeof(dliom_pose_graph_constraint), constraints.size(), f) != constraints.size() ||
      std::fread(inter_submap.data(), 4, inter_submap.size(), f) != inter_submap.size() || std::fread(&huber_scale, 8, 1, f) != 1)
    return 2;

  dliom::Context context(0);
  opt::OptimizationProblemOptions options;
  options.fix_z_in_3d = head[4] != 0;
  options.use_nonmonotonic_steps = head[5] != 0;
  options.max_num_iterations = head[6];
  options.huber_scale = huber_scale;
  options.fixed_frame_pose_translation_weight = 2e1;
  options.fixed_frame_pose_rotation_weight = 3e2;
  opt::OptimizationProblem3D problem(&context, options);
  for (int trajectory = 0; trajectory < 2; ++trajectory) {
    int32_t count;
    if (std::fread(&count, 4, 1, f) != 1) return 2;
    for (int i = 0; i < count; ++i) {
      int64_t time;
      int32_t has_pose;
      double pose[7];
      if (std::fread(&time, 8, 1, f) != 1 || std::fread(&has_pose, 4, 1, f) != 1 || std::fread(pose, 8, 7, f) != 7) return 2;
      dliom::sensor::FixedFramePoseData data{time, dliom::common::optional<Rigid3d>()};
      if (has_pose != 0) data.pose = Rigid3d::FromArray(pose);
      problem.AddFixedFramePoseData(trajectory, data);
    }
  }
  std::fclose(f);
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
  // TrimTrajectoryNode drops the fixed-frame data only the trimmed node needed: a node far behind the others with five
  // samples (without a pose, so that nothing interpolates towards them) around it, of which the first stays
  const size_t samples = problem.fixed_frame_pose_data().at(1).size();
  const int64_t far = 1000 + (N + 100) * int64_t{10000000};
  for (int i = -1; i <= 3; ++i) problem.AddFixedFramePoseData(1, dliom::sensor::FixedFramePoseData{far + i * 1000, dliom::common::optional<Rigid3d>()});
  problem.AddTrajectoryNode(1, opt::NodeSpec3D{far, Rigid3d(), Rigid3d()});
  problem.TrimTrajectoryNode(problem.node_data().rbegin()->first);
  if (problem.fixed_frame_pose_data().at(1).size() != samples + 1 || static_cast<int>(problem.node_data().size()) != N) return 3;
  if (problem.trajectory_data().size() != 2 || problem.trajectory_data().at(0).fixed_frame_origin_in_map.has_value()) return 3;

  std::vector<opt::OptimizationProblem3D::Constraint> list;
  for (int c = 0; c < C; ++c)
    list.push_back({submap_ids[constraints[c].submap], node_ids[constraints[c].node],
                    {Rigid3d::FromArray(constraints[c].zbar), constraints[c].translation_weight, constraints[c].rotation_weight},
                    inter_submap[c] != 0 ? opt::OptimizationProblem3D::Constraint::INTER_SUBMAP
                                         : opt::OptimizationProblem3D::Constraint::INTRA_SUBMAP});
  FILE* o = std::fopen(argv[2], "wb");
  if (o == nullptr) return 2;
  for (int solve = 0; solve < 2; ++solve) {
    problem.Solve(list, {}, {});
    for (int a = 0; a < S; ++a) {
      const std::array<double, 7> p = problem.submap_data().at(submap_ids[a]).global_pose.ToArray();
      std::fwrite(p.data(), 8, 7, o);
    }
    for (int j = 0; j < N; ++j) {
      const std::array<double, 7> p = problem.node_data().at(node_ids[j]).global_pose.ToArray();
      std::fwrite(p.data(), 8, 7, o);
    }
    for (int trajectory = 0; trajectory < 2; ++trajectory) {
      const auto& origin = problem.trajectory_data().at(trajectory).fixed_frame_origin_in_map;
      const int32_t has = origin.has_value();
      const std::array<double, 7> p = has ? origin.value().ToArray() : Rigid3d().ToArray();
      std::fwrite(&has, 4, 1, o);
      std::fwrite(p.data(), 8, 7, o);
    }
    const int32_t ints[2] = {problem.summary().termination_type, problem.summary().num_iterations};
    std::fwrite(ints, 4, 2, o);
    std::fwrite(&problem.summary().final_cost, 8, 1, o);
  }
  std::fclose(o);
  return 0;
}
