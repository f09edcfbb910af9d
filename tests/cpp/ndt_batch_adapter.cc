// dliom::registration::AlignPairsNdt and GenerateGroundTruthNdt (dliom_cartographer.h) on the device, against
// NormalDistributionsTransform one pair at a time; and GenerateGroundTruthIcp, whose pair collection the two now share,
// against IterativeClosestPoint one pair at a time.
//
//   ndt_batch_adapter      exit status 0 and a last line "ok": every check held; a line per failure otherwise
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

// eighty clusters of forty points along a 70 m corridor: most of them fill a 1 m cell with more than six points
std::vector<Vector3d> world_points() {
  Lcg rng{11};
  std::vector<Vector3d> out;
  for (int b = 0; b < 80; ++b) {
    const double c[3] = {-10.0 + 70.0 * rng.next(), -10.0 + 20.0 * rng.next(), -1.0 + 3.0 * rng.next()};
    for (int i = 0; i < 40; ++i) out.push_back(Vector3d{{c[0] + 0.3 * (rng.next() - 0.5), c[1] + 0.3 * (rng.next() - 0.5), c[2] + 0.3 * (rng.next() - 0.5)}});
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

bool same_double(double a, double b) { return (a != a && b != b) || std::memcmp(&a, &b, 8) == 0; }
// every field dliom.h promises of a batch (read_backs apart: the batch counts the pair's rounds)
bool same_result(const dliom_ndt_result& a, const dliom_ndt_result& b) {
  return a.converged == b.converged && a.reason == b.reason && a.iterations == b.iterations &&
         a.evaluations_with_hessian == b.evaluations_with_hessian && a.evaluations_without_hessian == b.evaluations_without_hessian &&
         std::memcmp(a.p, b.p, sizeof(a.p)) == 0 && std::memcmp(a.transform, b.transform, sizeof(a.transform)) == 0 &&
         same_double(a.score, b.score) && same_double(a.transformation_probability, b.transformation_probability) &&
         same_double(a.fitness_score, b.fitness_score) && a.fitness_count == b.fitness_count && a.pairs == b.pairs;
}

int64_t read_backs(dliom::Context* context) {
  int64_t n = 0;
  dliom::Check(dliom_ctx_read_backs(context->get(), &n), "dliom_ctx_read_backs");
  return n;
}

// the tool's loop, :151-261, one pair at a time through the PCL-shaped classes
template <class Method>
std::string pair_at_a_time(Method* method, const std::vector<Rigid3d>& poses, const std::vector<int64_t>& stamps,
                           const std::vector<int64_t>& bag, const std::vector<PointCloud>& clouds, const std::vector<size_t>& from_nodes,
                           int* no_revisit, int* past_the_bag, int* not_converged, int* degenerate) {
  std::string text;
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
    method->setInputSource(&clouds[static_cast<size_t>(it_from - bag.begin())]);
    method->setInputTarget(&clouds[static_cast<size_t>(it_to - bag.begin())]);
    method->align(nullptr, gt);
    if (!method->hasConverged()) {
      ++*not_converged;
      continue;
    }
    if (method->getFitnessScore() != method->getFitnessScore()) ++*degenerate;
    const registration::Matrix4f trans = method->getFinalTransformation();
    text += registration::FormatGroundTruthLine(stamps[from], stamps[static_cast<size_t>(to)], method->getFitnessScore(), trans,
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
  // Node 2's scan: nothing to align.  It is the pair ICP does not converge on.  NDT as dliom.h states it reports
  // converged == 0 only for a Newton step that is NaN, which no finite input reaches (a point that is not finite takes no
  // part in an evaluation); NDT ends this pair at once with a step of zero and a fitness score of NaN, and the line is
  // written, as the tool would write it.
  clouds[2].assign(5, Vector3f(std::numeric_limits<float>::quiet_NaN(), 0.f, 0.f));

  // ---- AlignPairsNdt: three pairs on one target, two of them on one source, against the class
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
    for (const int mode : {DLIOM_NDT_STEP_CLAMPED, DLIOM_NDT_STEP_MORE_THUENTE}) {
      auto ndt = registration::NormalDistributionsTransform::GroundTruthNdt(&context);
      ndt->setStepMode(mode);
      ndt->setMaximumIterations(4);
      std::vector<dliom_ndt_result> want;
      std::vector<PointCloud> want_clouds(pairs.size());
      for (size_t i = 0; i < pairs.size(); ++i) {
        ndt->setInputSource(pairs[i].source);
        ndt->setInputTarget(pairs[i].target);
        ndt->align(&want_clouds[i], pairs[i].guess);
        want.push_back(ndt->result());
      }
      const int64_t before = read_backs(&context);
      dliom_ndt_batch_stats stats;
      std::vector<PointCloud> got_clouds;
      const std::vector<dliom_ndt_result> got =
          registration::AlignPairsNdt(&context, ndt->options(), pairs, true, nullptr, &got_clouds, &stats);
      // what one target's cells and its index cost in polled read-backs (setInputTarget builds both): two distinct targets, not four
      const int64_t after = read_backs(&context);
      ndt->setInputTarget(pairs[0].target);
      const int64_t a_target = read_backs(&context) - after;
      expect(a_target >= 2 && after - before == 2 * a_target + stats.read_backs,
             "AlignPairsNdt builds one target and one index per distinct target");
      expect(stats.pairs == 4 && stats.chunks == 1, "AlignPairsNdt runs the pairs in one chunk");
      int64_t longest = 0, evaluations = 0;
      for (size_t i = 0; i < pairs.size(); ++i) {
        expect(same_result(got[i], want[i]), "AlignPairsNdt gives NormalDistributionsTransform's result");
        expect(want[i].pairs > 100 && want[i].iterations >= 1, "the pair is a real alignment");
        expect(got_clouds[i].size() == want_clouds[i].size() &&
                   std::memcmp(got_clouds[i].data(), want_clouds[i].data(), 12 * got_clouds[i].size()) == 0,
               "AlignPairsNdt gives NormalDistributionsTransform's aligned cloud");
        const int64_t own = want[i].evaluations_with_hessian + want[i].evaluations_without_hessian;
        expect(got[i].read_backs == own + 1 && want[i].read_backs == own + 2, "a pair's rounds: its evaluations and one final round");
        longest = std::max(longest, own + 1);
        evaluations += own;
      }
      expect(stats.read_backs == longest && stats.pair_evaluations == evaluations, "one read-back a lock-step round");
      const std::vector<dliom_ndt_result> plain = registration::AlignPairsNdt(&context, ndt->options(), pairs, false);
      for (size_t i = 0; i < pairs.size(); ++i)
        expect(plain[i].fitness_count == 0 && plain[i].fitness_score != plain[i].fitness_score &&
                   std::memcmp(plain[i].transform, want[i].transform, sizeof(want[i].transform)) == 0,
               "without the fitness score: the same alignment");
      expect(registration::AlignPairsNdt(&context, ndt->options(), {}).empty(), "AlignPairsNdt of no pair");
    }
  }

  const std::vector<size_t> from_nodes = {0, 1, 5, 2, 9, 10, 11, 3, 8, 0};
  // ---- GenerateGroundTruthNdt against the pair-at-a-time loop
  {
    int no_revisit = 0, past_the_bag = 0, not_converged = 0, degenerate = 0;
    auto ndt = registration::NormalDistributionsTransform::GroundTruthNdt(&context);
    const std::string want =
        pair_at_a_time(ndt.get(), poses, stamps, bag, clouds, from_nodes, &no_revisit, &past_the_bag, &not_converged, &degenerate);
    std::printf("%s", want.c_str());
    std::printf("ndt: no revisit %d, past the bag %d, not converged %d, nothing to align %d\n", no_revisit, past_the_bag, not_converged,
                degenerate);
    expect(no_revisit == 1 && past_the_bag >= 1 && degenerate >= 1, "the trajectory holds each kind of skipped or empty pair");
    const size_t lines = static_cast<size_t>(std::count(want.begin(), want.end(), '\n'));
    expect(lines >= 4 && lines + static_cast<size_t>(no_revisit + past_the_bag + not_converged) == from_nodes.size(),
           "every other pair writes a line");
    for (const size_t batch_size : {size_t{1}, size_t{3}, size_t{100}})
      expect(registration::GenerateGroundTruthNdt(&context, poses, stamps, bag, clouds, from_nodes, batch_size) == want,
             "GenerateGroundTruthNdt is byte-equal to the pair-at-a-time loop");
    expect(registration::GenerateGroundTruthNdt(&context, poses, stamps, bag, clouds, {}, 4).empty(), "no constraint, no text");
  }
  // ---- GenerateGroundTruthIcp: its text is what it was
  {
    int no_revisit = 0, past_the_bag = 0, not_converged = 0, degenerate = 0;
    auto icp = registration::IterativeClosestPoint::GroundTruthIcp(&context);
    const std::string want =
        pair_at_a_time(icp.get(), poses, stamps, bag, clouds, from_nodes, &no_revisit, &past_the_bag, &not_converged, &degenerate);
    std::printf("icp: no revisit %d, past the bag %d, not converged %d\n", no_revisit, past_the_bag, not_converged);
    expect(no_revisit == 1 && past_the_bag >= 1 && not_converged >= 1, "ICP's trajectory holds each kind of skipped pair");
    for (const size_t batch_size : {size_t{1}, size_t{3}, size_t{100}})
      expect(registration::GenerateGroundTruthIcp(&context, poses, stamps, bag, clouds, from_nodes, batch_size) == want,
             "GenerateGroundTruthIcp is byte-equal to the pair-at-a-time loop");
  }
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
