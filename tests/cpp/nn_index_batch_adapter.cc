// dliom::registration::BuildNnIndices and the IndexBuild::kBatched path of AlignPairs, AlignPairsNdt and the two
// generators (dliom_cartographer.h) on the device, against the one-by-one path.
//
//   nn_index_batch_adapter      exit status 0 and a last line "ok": every check held; a line per failure otherwise
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
using registration::IndexBuild;

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

// eighty clusters of forty points along a 70 m corridor (tests/cpp/ndt_batch_adapter.cc): both methods align on it
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
bool same_icp(const dliom_icp_result& a, const dliom_icp_result& b) {
  return a.converged == b.converged && a.reason == b.reason && a.iterations == b.iterations && a.correspondences == b.correspondences &&
         std::memcmp(a.transform, b.transform, sizeof(a.transform)) == 0 && same_double(a.mse, b.mse) &&
         same_double(a.fitness_score, b.fitness_score) && a.fitness_count == b.fitness_count && a.read_backs == b.read_backs &&
         a.settled_by_grid == b.settled_by_grid && a.settled_by_brute_force == b.settled_by_brute_force;
}
bool same_ndt(const dliom_ndt_result& a, const dliom_ndt_result& b) {
  return a.converged == b.converged && a.reason == b.reason && a.iterations == b.iterations &&
         a.evaluations_with_hessian == b.evaluations_with_hessian && a.evaluations_without_hessian == b.evaluations_without_hessian &&
         std::memcmp(a.p, b.p, sizeof(a.p)) == 0 && std::memcmp(a.transform, b.transform, sizeof(a.transform)) == 0 &&
         same_double(a.score, b.score) && same_double(a.transformation_probability, b.transformation_probability) &&
         same_double(a.fitness_score, b.fitness_score) && a.fitness_count == b.fitness_count && a.pairs == b.pairs &&
         a.read_backs == b.read_backs;
}
bool same_clouds(const std::vector<PointCloud>& a, const std::vector<PointCloud>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].size() != b[i].size() || std::memcmp(a[i].data(), b[i].data(), 12 * a[i].size()) != 0) return false;
  return true;
}

int64_t read_backs(dliom::Context* context) {
  int64_t n = 0;
  dliom::Check(dliom_ctx_read_backs(context->get(), &n), "dliom_ctx_read_backs");
  return n;
}

dliom_cloud* upload(dliom::Context* context, const PointCloud& cloud) {
  dliom_cloud* out = nullptr;
  dliom::Check(dliom_cloud_create(context->get(), &cloud[0].x, static_cast<int64_t>(cloud.size()), &out), "dliom_cloud_create");
  return out;
}
}  // namespace

int main() {
  dliom::Context context(0);
  const std::vector<Vector3d> world = world_points();
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

  // ---- BuildNnIndices: four clouds, one of them without a finite point and one named twice, against dliom_nn_index_create
  {
    const size_t picked[4] = {1, 2, 10, 1};
    std::vector<dliom_cloud*> device;
    for (const size_t k : picked) device.push_back(upload(&context, clouds[k]));
    dliom_cloud* queries = upload(&context, clouds[9]);
    const int64_t before = read_backs(&context);
    dliom_nn_index_batch_stats stats;
    const std::vector<dliom_nn_index*> built =
        registration::BuildNnIndices(&context, std::vector<const dliom_cloud*>(device.begin(), device.end()), nullptr, nullptr, &stats);
    expect(read_backs(&context) - before == 1 && stats.read_backs == 1 && stats.chunks == 1 && stats.indices == 4 && stats.cell_runs == 1,
           "BuildNnIndices builds four indices in one chunk with one read-back");
    expect(built.size() == 4 && built[0] != built[3], "each mention gets an index of its own");
    const size_t n = clouds[9].size();
    for (size_t k = 0; k < built.size(); ++k) {
      dliom_nn_index* single = nullptr;
      dliom::Check(dliom_nn_index_create(context.get(), device[k], nullptr, &single), "dliom_nn_index_create");
      dliom_nn_index_memory a, b;
      dliom::Check(dliom_nn_index_memory_stats(built[k], &a), "dliom_nn_index_memory_stats");
      dliom::Check(dliom_nn_index_memory_stats(single, &b), "dliom_nn_index_memory_stats");
      expect(a.points == b.points && a.finite_points == b.finite_points && a.cells == b.cells && std::memcmp(a.dims, b.dims, sizeof(a.dims)) == 0 &&
                 a.index_bytes == b.index_bytes && same_double(a.cell_edge, b.cell_edge),
             "a batch-built index has the single build's memory statistics");
      std::vector<int32_t> j[2] = {std::vector<int32_t>(n), std::vector<int32_t>(n)};
      std::vector<float> d2[2] = {std::vector<float>(n), std::vector<float>(n)};
      dliom_nn_query_stats st[2];
      dliom_nn_index* const both[2] = {built[k], single};
      for (int w = 0; w < 2; ++w)
        dliom::Check(dliom_nn_index_query(both[w], queries, nullptr, 30.0, DLIOM_NN_AUTO, j[w].data(), d2[w].data(), &st[w]), "dliom_nn_index_query");
      expect(j[0] == j[1] && std::memcmp(d2[0].data(), d2[1].data(), 4 * n) == 0 && st[0].settled_by_grid == st[1].settled_by_grid &&
                 st[0].settled_by_brute_force == st[1].settled_by_brute_force && st[0].non_finite == st[1].non_finite,
             "a batch-built index answers as the single-built one");
      expect(k == 1 ? a.finite_points == 0 : st[0].settled_by_grid + st[0].settled_by_brute_force == static_cast<int64_t>(n),
             "the queries are real searches");
      dliom_nn_index_destroy(single);
    }
    for (dliom_cloud* c : device) dliom_cloud_destroy(c);  // the clouds go first
    dliom_nn_index_destroy(built[2]);
    dliom_nn_index_destroy(built[0]);
    dliom_nn_index_destroy(built[3]);
    dliom_nn_index_destroy(built[1]);
    dliom_cloud_destroy(queries);
    expect(registration::BuildNnIndices(&context, {}).empty(), "BuildNnIndices of no cloud");
  }

  registration::Matrix4f guess;
  guess(0, 3) = 0.05f;
  std::vector<registration::AlignmentPair> pairs(5);  // three distinct targets, in the order 1, 10, 3
  pairs[0].source = &clouds[9];
  pairs[0].target = &clouds[1];
  pairs[1].source = &clouds[8];
  pairs[1].target = &clouds[1];
  pairs[1].guess = guess;
  pairs[2].source = &clouds[0];
  pairs[2].target = &clouds[10];
  pairs[3].source = &clouds[9];
  pairs[3].target = &clouds[1];
  pairs[3].guess = guess;
  pairs[4].source = &clouds[7];
  pairs[4].target = &clouds[3];

  // ---- AlignPairs: kBatched against kOneByOne
  {
    const dliom_icp_options options = registration::IterativeClosestPoint::GroundTruthIcp(&context)->options();
    dliom_icp_batch_stats stats[2];
    std::vector<PointCloud> got_clouds[2];
    std::vector<dliom_icp_result> got[2];
    int64_t cost[2];
    const IndexBuild builds[2] = {IndexBuild::kOneByOne, IndexBuild::kBatched};
    for (int w = 0; w < 2; ++w) {
      const int64_t before = read_backs(&context);
      got[w] = registration::AlignPairs(&context, options, pairs, nullptr, &got_clouds[w], &stats[w], builds[w]);
      cost[w] = read_backs(&context) - before - stats[w].read_backs;
    }
    expect(cost[0] == 3 && cost[1] == 1, "AlignPairs: kBatched costs one build read-back a chunk, kOneByOne one a distinct target");
    expect(stats[0].read_backs == stats[1].read_backs && stats[0].pair_searches == stats[1].pair_searches, "the alignments cost the same");
    for (size_t i = 0; i < pairs.size(); ++i) {
      expect(same_icp(got[0][i], got[1][i]), "AlignPairs gives the same result under both builds");
      expect(got[0][i].iterations >= 1 && got[0][i].correspondences > 100, "the pair is a real alignment");
    }
    expect(same_clouds(got_clouds[0], got_clouds[1]), "AlignPairs gives the same aligned clouds under both builds");
    expect(registration::AlignPairs(&context, options, {}, nullptr, nullptr, nullptr, IndexBuild::kBatched).empty(), "AlignPairs of no pair");
  }

  // ---- AlignPairsNdt: kBatched against kOneByOne
  {
    auto ndt = registration::NormalDistributionsTransform::GroundTruthNdt(&context);
    ndt->setMaximumIterations(4);
    dliom_ndt_batch_stats stats[2];
    std::vector<PointCloud> got_clouds[2];
    std::vector<dliom_ndt_result> got[2];
    int64_t cost[2];
    const IndexBuild builds[2] = {IndexBuild::kOneByOne, IndexBuild::kBatched};
    for (int w = 0; w < 2; ++w) {
      const int64_t before = read_backs(&context);
      got[w] = registration::AlignPairsNdt(&context, ndt->options(), pairs, true, nullptr, &got_clouds[w], &stats[w], builds[w]);
      cost[w] = read_backs(&context) - before - stats[w].read_backs;
    }
    // both build the three targets' cells in one call (the same read-backs); the indices cost three read-backs or one
    expect(cost[0] - cost[1] == 3 - 1, "AlignPairsNdt: kBatched costs one index read-back a chunk, kOneByOne one a distinct target");
    for (size_t i = 0; i < pairs.size(); ++i) {
      expect(same_ndt(got[0][i], got[1][i]), "AlignPairsNdt gives the same result under both builds");
      expect(got[0][i].fitness_count > 100, "the fitness score is a real search");
    }
    expect(same_clouds(got_clouds[0], got_clouds[1]), "AlignPairsNdt gives the same aligned clouds under both builds");
    const int64_t before = read_backs(&context);
    dliom_ndt_batch_stats plain_stats;
    const std::vector<dliom_ndt_result> plain =
        registration::AlignPairsNdt(&context, ndt->options(), pairs, false, nullptr, nullptr, &plain_stats, IndexBuild::kBatched);
    expect(read_backs(&context) - before - plain_stats.read_backs == cost[1] - 1, "without the fitness score no index is built");
    expect(plain.size() == pairs.size() && plain[0].fitness_count == 0, "without the fitness score: no count");
  }

  // ---- the generators' text
  {
    const std::vector<size_t> from_nodes = {0, 1, 5, 2, 9, 10, 11, 3, 8, 0};
    const std::string icp = registration::GenerateGroundTruthIcp(&context, poses, stamps, bag, clouds, from_nodes, 100);
    const std::string ndt = registration::GenerateGroundTruthNdt(&context, poses, stamps, bag, clouds, from_nodes, 100);
    std::printf("%s%s", icp.c_str(), ndt.c_str());
    expect(std::count(icp.begin(), icp.end(), '\n') >= 3 && std::count(ndt.begin(), ndt.end(), '\n') >= 3, "the generators write lines");
    for (const size_t batch_size : {size_t{1}, size_t{3}, size_t{100}}) {
      expect(registration::GenerateGroundTruthIcp(&context, poses, stamps, bag, clouds, from_nodes, batch_size, IndexBuild::kBatched) == icp,
             "GenerateGroundTruthIcp's text is byte-equal under both builds");
      expect(registration::GenerateGroundTruthNdt(&context, poses, stamps, bag, clouds, from_nodes, batch_size, IndexBuild::kBatched) == ndt,
             "GenerateGroundTruthNdt's text is byte-equal under both builds");
    }
  }
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
