// mapping::scan_matching::ComputeConstraints (d-liom_amd/cpp/dliom_cartographer.h) against the adapter's serial chain
// for the same queries: FastCorrelativeScanMatcher3D::MatchWith3DofInitial, then CeresScanMatcher3D::Match with the
// match as target and initial pose on both grids (constraint_builder_3d.cc:202-334).  Found flags, fast results and
// refined poses must be identical.  Built by tests/test_constraint_batch_host.py (no GPU); run by
// tests/test_gpu_constraint_batch.py.
#include <cstdio>
#include <cstring>

#include "../../d-liom_amd/cpp/dliom_cartographer.h"

using namespace dliom;
using mapping::HybridGrid;
using mapping::scan_matching::CeresScanMatcher3D;
using mapping::scan_matching::FastCorrelativeScanMatcher3D;
using sensor::Vector3f;
using transform::Rigid3d;

static int g_failures = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++g_failures;                                                   \
    }                                                                 \
  } while (0)

static bool SameBits(const Rigid3d& a, const Rigid3d& b) {
  const std::array<double, 7> x = a.ToArray(), y = b.ToArray();
  return std::memcmp(x.data(), y.data(), sizeof(double) * 7) == 0;
}

int main() {
  Context context(0);
  // the reference test's 12-point cloud (fast_correlative_scan_matcher_3d_test.cc), its cells set at a known pose
  sensor::PointCloud cloud;
  for (int a = 0; a < 3; ++a)
    for (float r : {4.f, 4.5f, 5.f, 5.5f}) cloud.push_back(Vector3f(a == 0 ? r : 0.f, a == 1 ? r : 0.f, a == 2 ? r : 0.f));
  const float tx = 0.3f, ty = -0.2f, tz = 0.1f;
  HybridGrid hi(&context, 0.05f), lo(&context, 0.1f);
  for (const Vector3f& p : cloud) {
    const Vector3f q(p.x + tx, p.y + ty, p.z + tz);
    hi.SetProbability(hi.GetCellIndex(q), 0.9f);
    lo.SetProbability(lo.GetCellIndex(q), 0.9f);
  }
  const mapping::scan_matching::FastCorrelativeScanMatcherOptions3D fo{6, 6, 0.1, 0.15, 0.8, 0.8, 0.3};
  const FastCorrelativeScanMatcher3D matcher(&context, hi, &lo, {{std::vector<float>(10, 0.f), 0.f}}, fo);
  mapping::scan_matching::CeresScanMatcherOptions3D co;
  co.occupied_space_weight = {1.0, 6.0};
  co.translation_weight = 5.0;
  co.rotation_weight = 4e2;
  co.max_num_iterations = 12;
  const CeresScanMatcher3D ceres(&context, co);
  mapping::scan_matching::TrajectoryNodeData data;
  data.high_resolution_point_cloud = cloud;
  data.low_resolution_point_cloud = cloud;
  data.rotational_scan_matcher_histogram.assign(10, 0.f);

  std::vector<mapping::scan_matching::ConstraintQuery> queries;
  for (int k = 0; k < 12; ++k) {  // guesses around the pose; the last two are out of the window (no constraint)
    const double d = k < 10 ? 0.05 * (k % 5) - 0.1 : 3.0;
    const Rigid3d guess({{tx + d, ty - 0.5 * d, tz + 0.25 * d}}, {{1., 0., 0., 0.}});
    queries.push_back({{&matcher, FastCorrelativeScanMatcher3D::Kind::kMatchWith3DofInitial, guess, Rigid3d(), &data,
                        k % 3 == 0 ? 0.2f : 0.1f},
                       &hi, &lo});
  }
  dliom_batch_stats fast_stats, ceres_stats;
  const std::vector<mapping::scan_matching::ComputedConstraint> got =
      mapping::scan_matching::ComputeConstraints(ceres, queries, &fast_stats, &ceres_stats);
  int found = 0;
  for (size_t i = 0; i < queries.size(); ++i) {
    FastCorrelativeScanMatcher3D::Result r;
    const bool f = matcher.MatchWith3DofInitial(queries[i].search.pose, data, queries[i].search.min_score, &r);
    EXPECT(f == got[i].found);
    if (!f || !got[i].found) continue;
    ++found;
    EXPECT(r.score == got[i].match.score);
    EXPECT(r.rotational_score == got[i].match.rotational_score);
    EXPECT(r.low_resolution_score == got[i].match.low_resolution_score);
    EXPECT(SameBits(r.pose_estimate, got[i].match.pose_estimate));
    Rigid3d refined;
    mapping::scan_matching::Summary summary;
    ceres.Match(r.pose_estimate.translation(), r.pose_estimate, {{&data.high_resolution_point_cloud, &hi}, {&data.low_resolution_point_cloud, &lo}},
                &refined, &summary);
    EXPECT(SameBits(refined, got[i].pose));
  }
  EXPECT(found >= 8);
  EXPECT(found < static_cast<int>(queries.size()));
  EXPECT(fast_stats.batched == 12 && fast_stats.frontier_chains == 1);
  EXPECT(ceres_stats.batched == found && ceres_stats.lm_launches == 1);
  std::printf("%s: %d of %zu queries found a constraint\n", g_failures ? "FAILED" : "ok", found, queries.size());
  return g_failures ? 1 : 0;
}
