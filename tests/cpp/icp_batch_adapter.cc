// dliom::registration::AlignPairs and GenerateGroundTruthIcp (dliom_cartographer.h) on the device, against
// IterativeClosestPoint one pair at a time.
//
//   icp_batch_adapter      exit status 0 and a last line "ok": every check held; a line per failure otherwise
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "dliom_cartographer.h"

namespace {
namespace registration = dliom::registration;
using dliom::sensor::PointCloud;
using dliom::sensor::Vector3f;
using dliom::transform::Quaterniond;
using dliom::transform::Rigid3d;
using dliom::transform::Vector3d;

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++failures;
  }
}

struct Lcg {  // a fixed stream of numbers in [0, 1)
  unsigned long long s;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<double>(s >> 11) / 9007199254740992.0;
  }
};

// a floor, two walls and scattered points around a 50 m corridor
std::vector<Vector3d> world_points() {
  Lcg rng{7};
  std::vector<Vector3d> out;
  for (int i = 0; i < 1400; ++i) {
    Vector3d p{{-15.0 + 80.0 * rng.next(), -15.0 + 30.0 * rng.next(), -1.8 + 6.0 * rng.next()}};
    if (i % 4 == 0) p.v[2] = -1.8;
    if (i % 4 == 1) p.v[1] = 15.0;
    if (i % 4 == 2) p.v[0] = -15.0 + 0.5 * p.v[2];
    out.push_back(p);
  }
  return out;
}

Rigid3d node_pose(double x, double y, double yaw) {
  return Rigid3d(Vector3d{{x, y, 0.0}}, Quaterniond{{std::cos(0.5 * yaw), 0.0, 0.0, std::sin(0.5 * yaw)}});
}

// what the sensor at `pose` sees of the world within 35 m, in its own frame, with 1 cm of noise
PointCloud scan_from(const Rigid3d& pose, const std::vector<Vector3d>& world, unsigned long long seed) {
  namespace ff = dliom::mapping::optimization::fixed_frame;
  const Rigid3d inverse = ff::Inverse(pose);
  Lcg rng{seed};
  PointCloud out;
  for (const Vector3d& p : world) {
    const std::array<double, 3> q = ff::Rotate(inverse.rotation(), p.v);
    const double v[3] = {q[0] + inverse.translation().v[0], q[1] + inverse.translation().v[1], q[2] + inverse.translation().v[2]};
    const double noise[3] = {0.01 * (rng.next() - 0.5), 0.01 * (rng.next() - 0.5), 0.01 * (rng.next() - 0.5)};
    if (v[0] * v[0] + v[1] * v[1] + v[2] * v[2] > 35.0 * 35.0) continue;
    out.push_back(Vector3f(static_cast<float>(v[0] + noise[0]), static_cast<float>(v[1] + noise[1]), static_cast<float>(v[2] + noise[2])));
  }
  return out;
}

bool same_result(const dliom_icp_result& a, const dliom_icp_result& b) {
  return a.converged == b.converged && a.reason == b.reason && a.iterations == b.iterations && a.correspondences == b.correspondences &&
         std::memcmp(a.transform, b.transform, sizeof(a.transform)) == 0 && std::memcmp(&a.mse, &b.mse, 8) == 0 &&
         ((a.fitness_score != a.fitness_score && b.fitness_score != b.fitness_score) || std::memcmp(&a.fitness_score, &b.fitness_score, 8) == 0) &&
         a.fitness_count == b.fitness_count && a.read_backs == b.read_backs && a.settled_by_grid == b.settled_by_grid &&
         a.settled_by_brute_force == b.settled_by_brute_force;
}

int64_t read_backs(dliom::Context* context) {
  int64_t n = 0;
  dliom::Check(dliom_ctx_read_backs(context->get(), &n), "dliom_ctx_read_backs");
  return n;
}

// the tool's loop, :151-261, one pair at a time through the PCL-shaped class
std::string pair_at_a_time(dliom::Context* context, const std::vector<Rigid3d>& poses, const std::vector<int64_t>& stamps,
                           const std::vector<int64_t>& bag, const std::vector<PointCloud>& clouds, const std::vector<size_t>& from_nodes,
                           int* no_revisit, int* past_the_bag, int* not_converged) {
  std::string text;
  auto icp = registration::IterativeClosestPoint::GroundTruthIcp(context);
  for (const size_t from : from_nodes) {
    const int to = registration::FindRevisitNode(poses, stamps, from);
    if (to < 0) {
      ++*no_revisit;
      continue;
    }
    const auto it_to = std::lower_bound(bag.begin(), bag.end(), stamps[static_cast<size_t>(to)]);
    const auto it_from = std::lower_bound(bag.begin(), bag.end(), stamps[from]);
    if (it_to == bag.end() || it_from == bag.end()) {
      ++*past_the_bag;
      continue;
    }
    const registration::Matrix4f gt = registration::GroundTruthGuess(poses[static_cast<size_t>(to)], poses[from]);
    icp->setInputSource(&clouds[static_cast<size_t>(it_from - bag.begin())]);
    icp->setInputTarget(&clouds[static_cast<size_t>(it_to - bag.begin())]);
    icp->align(nullptr, gt);
    if (!icp->hasConverged()) {
      ++*not_converged;
      continue;
    }
    const registration::Matrix4f trans = icp->getFinalTransformation();
    text += registration::FormatGroundTruthLine(stamps[from], stamps[static_cast<size_t>(to)], icp->getFitnessScore(), trans,
                                                registration::GroundTruthDifferenceNorm(gt, trans));
  }
  return text;
}
}  // namespace

int main() {
  dliom::Context context(0);
  const std::vector<Vector3d> world = world_points();
  // out for 45 s and back beside the way out, nodes 9 s apart: node 5 (45 s) has no node 60 s away
  const double xs[12] = {0, 10, 20, 30, 40, 50, 40, 30, 20, 10, 0, 10}, ys[12] = {0, 0, 0, 0, 0, 0, 0.6, 0.6, 0.6, 0.6, 0.6, 1.2};
  std::vector<Rigid3d> poses;
  std::vector<int64_t> stamps, bag;
  std::vector<PointCloud> clouds;
  for (int k = 0; k < 12; ++k) {
    poses.push_back(node_pose(xs[k], ys[k], 0.02 * k));
    stamps.push_back(1600000000000000000ll + 9000000000ll * k);
    if (k < 11) {  // the bag ends before node 11's stamp
      bag.push_back(stamps.back());
      clouds.push_back(scan_from(poses.back(), world, 100 + static_cast<unsigned long long>(k)));
    }
  }
  clouds[2].assign(5, Vector3f(std::numeric_limits<float>::quiet_NaN(), 0.f, 0.f));  // node 2's scan: nothing to align

  // ---- AlignPairs: three pairs on one target, two of them on one source, against the class
  {
    registration::Matrix4f guess;
    guess(0, 3) = 0.05f;
    std::vector<registration::AlignmentPair> pairs(4);
    pairs[0].source = &clouds[9];
    pairs[0].target = &clouds[1];
    pairs[1].source = &clouds[8];
    pairs[1].target = &clouds[1];
    pairs[1].guess = guess;
    pairs[2].source = &clouds[9];
    pairs[2].target = &clouds[1];
    pairs[2].guess = guess;
    pairs[3].source = &clouds[0];
    pairs[3].target = &clouds[10];
    auto icp = registration::IterativeClosestPoint::GroundTruthIcp(&context);
    std::vector<dliom_icp_result> want;
    std::vector<PointCloud> want_clouds(pairs.size());
    for (size_t i = 0; i < pairs.size(); ++i) {
      icp->setInputSource(pairs[i].source);
      icp->setInputTarget(pairs[i].target);
      icp->align(&want_clouds[i], pairs[i].guess);
      want.push_back(icp->result());
    }
    const int64_t before = read_backs(&context);
    dliom_icp_batch_stats stats;
    std::vector<PointCloud> got_clouds;
    const std::vector<dliom_icp_result> got = registration::AlignPairs(&context, icp->options(), pairs, nullptr, &got_clouds, &stats);
    // an index's creation is one polled read-back (its bounding box): two distinct targets, not four
    expect(read_backs(&context) - before == 2 + stats.read_backs, "AlignPairs builds one index per distinct target");
    expect(stats.pairs == 4 && stats.chunks == 1, "AlignPairs runs the pairs in one chunk");
    int64_t longest = 0;
    for (size_t i = 0; i < pairs.size(); ++i) {
      expect(same_result(got[i], want[i]), "AlignPairs gives IterativeClosestPoint's result");
      expect(got_clouds[i].size() == want_clouds[i].size() &&
                 std::memcmp(got_clouds[i].data(), want_clouds[i].data(), 12 * got_clouds[i].size()) == 0,
             "AlignPairs gives IterativeClosestPoint's aligned cloud");
      longest = std::max<int64_t>(longest, want[i].read_backs);
    }
    expect(stats.read_backs == longest, "one read-back a lock-step round");
    expect(registration::AlignPairs(&context, icp->options(), {}).empty(), "AlignPairs of no pair");
  }

  // ---- GenerateGroundTruthIcp against the pair-at-a-time loop
  {
    const std::vector<size_t> from_nodes = {0, 1, 5, 2, 9, 10, 11, 3, 8, 0};
    int no_revisit = 0, past_the_bag = 0, not_converged = 0;
    const std::string want = pair_at_a_time(&context, poses, stamps, bag, clouds, from_nodes, &no_revisit, &past_the_bag, &not_converged);
    std::printf("%s", want.c_str());
    std::printf("no revisit %d, past the bag %d, not converged %d\n", no_revisit, past_the_bag, not_converged);
    expect(no_revisit == 1 && past_the_bag >= 1 && not_converged >= 1, "the trajectory holds each kind of skipped pair");
    const size_t lines = static_cast<size_t>(std::count(want.begin(), want.end(), '\n'));
    expect(lines >= 4 && lines + static_cast<size_t>(no_revisit + past_the_bag + not_converged) == from_nodes.size(),
           "every other pair writes a line");
    for (const size_t batch_size : {size_t{1}, size_t{3}, size_t{4}, size_t{100}})
      expect(registration::GenerateGroundTruthIcp(&context, poses, stamps, bag, clouds, from_nodes, batch_size) == want,
             "GenerateGroundTruthIcp is byte-equal to the pair-at-a-time loop");
    expect(registration::GenerateGroundTruthIcp(&context, poses, stamps, bag, clouds, {}, 4).empty(), "no constraint, no text");
  }
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
