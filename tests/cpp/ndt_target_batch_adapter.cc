// dliom::registration::BuildNdtTargets (dliom_cartographer.h) on the device against
// NormalDistributionsTransform::setInputTarget one cloud at a time, and GenerateGroundTruthNdt -- whose targets are now built
// through it, all distinct targets of a batch in one call -- against the pair-at-a-time loop on the 12-node trajectory of
// ndt_batch_adapter.cc.
//
//   ndt_target_batch_adapter      exit status 0 and a last line "ok": every check held; a line per failure otherwise
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
// every field of a result but its read-backs and times
bool same_result(const dliom_ndt_result& a, const dliom_ndt_result& b) {
  return a.converged == b.converged && a.reason == b.reason && a.iterations == b.iterations &&
         a.evaluations_with_hessian == b.evaluations_with_hessian && a.evaluations_without_hessian == b.evaluations_without_hessian &&
         std::memcmp(a.p, b.p, sizeof(a.p)) == 0 && std::memcmp(a.transform, b.transform, sizeof(a.transform)) == 0 &&
         same_double(a.score, b.score) && same_double(a.transformation_probability, b.transformation_probability) && a.pairs == b.pairs;
}

std::vector<dliom_ndt_cell> cells_of(const dliom_ndt_target* target) {
  int64_t count = 0;
  dliom::Check(dliom_ndt_target_cells(target, nullptr, 0, &count), "dliom_ndt_target_cells");
  std::vector<dliom_ndt_cell> cells(static_cast<size_t>(count));
  if (count > 0) dliom::Check(dliom_ndt_target_cells(target, cells.data(), count, &count), "dliom_ndt_target_cells");
  return cells;
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
  clouds[2].assign(5, Vector3f(std::numeric_limits<float>::quiet_NaN(), 0.f, 0.f));  // node 2's scan: no cell at all

  // ---- BuildNdtTargets: every scan, node 2's among them and node 1's twice, against setInputTarget cloud by cloud
  {
    const std::vector<size_t> which = {0, 1, 2, 3, 1, 4, 5, 6, 7, 8, 9, 10};
    auto ndt = registration::NormalDistributionsTransform::GroundTruthNdt(&context);
    ndt->setMaximumIterations(3);
    std::vector<dliom_cloud*> uploaded;
    std::vector<const dliom_cloud*> named;
    for (const size_t k : which) {
      dliom_cloud* cloud = nullptr;
      dliom::Check(dliom_cloud_create(context.get(), &clouds[k][0].x, static_cast<int64_t>(clouds[k].size()), &cloud), "dliom_cloud_create");
      uploaded.push_back(cloud);
      named.push_back(cloud);
    }
    dliom_cloud* source = nullptr;
    dliom::Check(dliom_cloud_create(context.get(), &clouds[9][0].x, static_cast<int64_t>(clouds[9].size()), &source), "dliom_cloud_create");
    const int64_t before = read_backs(&context);
    dliom_ndt_target_batch_stats stats;
    const std::vector<dliom_ndt_target*> built = registration::BuildNdtTargets(&context, ndt->options(), named, nullptr, &stats);
    expect(read_backs(&context) - before == 2 && stats.read_backs == 2 && stats.chunks == 1 && stats.synchronizations == 1 &&
               stats.targets == static_cast<int64_t>(which.size()),
           "BuildNdtTargets builds every target in one chunk with two read-backs");
    expect(built.size() == which.size(), "a target a cloud");
    for (dliom_cloud* cloud : uploaded) dliom_cloud_destroy(cloud);  // a target outlives its cloud
    int64_t cells = 0;
    const double guess16[16] = {1, 0, 0, static_cast<double>(0.05f), 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    registration::Matrix4f guess;
    guess(0, 3) = 0.05f;
    for (size_t i = 0; i < which.size(); ++i) {
      // the cells: what dliom_ndt_target_create, which setInputTarget calls, builds
      dliom_cloud* cloud = nullptr;
      dliom_ndt_target* single = nullptr;
      dliom::Check(dliom_cloud_create(context.get(), &clouds[which[i]][0].x, static_cast<int64_t>(clouds[which[i]].size()), &cloud),
                   "dliom_cloud_create");
      dliom::Check(dliom_ndt_target_create(context.get(), cloud, &ndt->options(), &single), "dliom_ndt_target_create");
      dliom_cloud_destroy(cloud);
      const std::vector<dliom_ndt_cell> got = cells_of(built[i]), want = cells_of(single);
      expect(got.size() == want.size() && (got.empty() || std::memcmp(got.data(), want.data(), sizeof(dliom_ndt_cell) * got.size()) == 0),
             "BuildNdtTargets gives dliom_ndt_target_create's cells, byte for byte");
      dliom_ndt_target_memory m_got, m_want;
      dliom::Check(dliom_ndt_target_memory_stats(built[i], &m_got), "dliom_ndt_target_memory_stats");
      dliom::Check(dliom_ndt_target_memory_stats(single, &m_want), "dliom_ndt_target_memory_stats");
      expect(m_got.points == m_want.points && m_got.kept_points == m_want.kept_points && m_got.cells == m_want.cells &&
                 m_got.valid_cells == m_want.valid_cells && m_got.target_bytes == m_want.target_bytes && m_got.read_backs == 2,
             "BuildNdtTargets gives dliom_ndt_target_create's counts");
      dliom_ndt_target_destroy(single);
      cells += m_got.cells;
      // the valid cells on the device: the class's alignment through setInputTarget against dliom_ndt_align on the built target
      ndt->setInputSource(&clouds[9]);
      ndt->setInputTarget(&clouds[which[i]], false);
      ndt->align(nullptr, guess);
      dliom_ndt_result result;
      dliom::Check(dliom_ndt_align(built[i], source, guess16, &ndt->options(), nullptr, &result, nullptr), "dliom_ndt_align");
      expect(same_result(result, ndt->result()), "a built target aligns as setInputTarget's does");
      if (which[i] == 8) expect(result.pairs > 100 && result.iterations >= 1, "the pair is a real alignment");
      if (which[i] == 2) expect(m_got.cells == 0 && m_got.kept_points == 0, "node 2's scan has no cell");
    }
    expect(stats.cells == cells && cells > 100, "the statistics count the targets' cells");
    // destroyed out of order, each on its own
    for (size_t i = 0; i < built.size(); i += 2) dliom_ndt_target_destroy(built[i]);
    dliom_ndt_result result;
    dliom::Check(dliom_ndt_align(built[9], source, guess16, &ndt->options(), nullptr, &result, nullptr), "dliom_ndt_align");
    expect(result.pairs > 100, "a target is usable after its neighbours are gone");
    for (size_t i = 1; i < built.size(); i += 2) dliom_ndt_target_destroy(built[i]);
    dliom_cloud_destroy(source);
    expect(registration::BuildNdtTargets(&context, ndt->options(), {}).empty(), "BuildNdtTargets of no cloud");
  }

  // ---- GenerateGroundTruthNdt, its targets built a batch at a time, against the pair-at-a-time loop
  {
    const std::vector<size_t> from_nodes = {0, 1, 5, 2, 9, 10, 11, 3, 8, 0};
    int no_revisit = 0, past_the_bag = 0, not_converged = 0, degenerate = 0;
    auto ndt = registration::NormalDistributionsTransform::GroundTruthNdt(&context);
    const std::string want =
        pair_at_a_time(ndt.get(), poses, stamps, bag, clouds, from_nodes, &no_revisit, &past_the_bag, &not_converged, &degenerate);
    std::printf("%s", want.c_str());
    expect(no_revisit == 1 && past_the_bag >= 1 && degenerate >= 1, "the trajectory holds each kind of skipped or empty pair");
    expect(std::count(want.begin(), want.end(), '\n') >= 4, "the loop writes lines");
    for (const size_t batch_size : {size_t{1}, size_t{3}, size_t{100}})
      expect(registration::GenerateGroundTruthNdt(&context, poses, stamps, bag, clouds, from_nodes, batch_size) == want,
             "GenerateGroundTruthNdt is byte-equal to the pair-at-a-time loop");
  }
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
