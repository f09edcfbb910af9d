// Known answers for the host pieces of dliom::registration (dliom_cartographer.h) that need no device: the ground-truth
// line against an ostream written here, the revisit node on a hand-made trajectory.  The IterativeClosestPoint class is
// instantiated only to prove that it compiles; nothing of it runs (no context is created).
//
//   icp_adapter_kat        exit status 0: every check held; a line per failure otherwise
#include <cstdio>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "dliom_cartographer.h"

namespace {
namespace registration = dliom::registration;
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

// what `ofs << ts_from << " " << ts_to << " " << align_error << " " << R.row(0)[0] ... << diff_norm << "\n"` writes
std::string stream_line(int64_t from, int64_t to, double error, const registration::Matrix4f& m, float norm) {
  std::ostringstream out;
  out << from << " " << to << " " << error << " ";
  for (int r = 0; r < 3; ++r) out << m(r, 0) << " " << m(r, 1) << " " << m(r, 2) << " " << m(r, 3) << " ";
  out << norm << "\n";
  return out.str();
}

Rigid3d at(double x, double y, double z) { return Rigid3d(Vector3d{{x, y, z}}, Quaterniond{{1, 0, 0, 0}}); }

// never called: the adapter's members must compile under -Wall -Werror
void instantiate(dliom::Context* context, const dliom::sensor::PointCloud* cloud) {
  auto icp = registration::IterativeClosestPoint::GroundTruthIcp(context);
  icp->setInputSource(cloud);
  icp->setInputTarget(cloud);
  dliom::sensor::PointCloud output;
  icp->align(&output, registration::Matrix4f::Identity());
  (void)icp->hasConverged();
  (void)icp->getFitnessScore();
  (void)icp->getFinalTransformation();
  (void)registration::IterativeClosestPoint::MatchByIcp(context)->options();
}
}  // namespace

int main(int argc, char**) {
  if (argc > 1000) instantiate(nullptr, nullptr);
  registration::Matrix4f m;
  const float values[12] = {0.99984771f, -0.017452406f, 1e-9f,        12.5f,  0.017452406f, 0.99984771f,
                            -3.25e-5f,   -7.0f,         123456.789f, 1e-5f,  1.0f,         1e10f};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) m(r, c) = values[4 * r + c];
  const struct {
    int64_t from, to;
    double error;
    float norm;
  } cases[] = {{1600000000123456789ll, 1600000075000000001ll, 0.0123456789, 0.25f},
               {0, -5, 99999.0, 0.f},
               {7, 8, 1e-7, 1234567.f},
               {9, 10, std::numeric_limits<double>::infinity(), std::numeric_limits<float>::quiet_NaN()},
               {11, 12, 1.0 / 3.0, 2.f / 3.f}};
  for (const auto& c : cases)
    expect(registration::FormatGroundTruthLine(c.from, c.to, c.error, m, c.norm) == stream_line(c.from, c.to, c.error, m, c.norm),
           "FormatGroundTruthLine is byte-equal to the ostream");
  expect(registration::FormatGroundTruthLine(1, 2, 0.5, registration::Matrix4f::Identity(), 0.f) ==
             "1 2 0.5 1 0 0 0 0 1 0 0 0 0 1 0 0\n",
         "FormatGroundTruthLine of the identity");

  // a loop: out for 100 s, back past the start.  Nodes 10 s apart.
  std::vector<Rigid3d> poses;
  std::vector<int64_t> stamps;
  const double xs[12] = {0, 10, 20, 30, 40, 50, 40, 30, 20, 10, 0, 10};
  for (int k = 0; k < 12; ++k) {
    poses.push_back(at(xs[k], k == 8 ? 0.5 : 0.0, 0.0));
    stamps.push_back(1000000000ll * 10 * k);
  }
  expect(registration::FindRevisitNode(poses, stamps, 0) == 10, "node 0 is revisited by node 10");
  expect(registration::FindRevisitNode(poses, stamps, 1) == 9, "node 1: nodes 9 and 11 are equally near, the first wins");
  expect(registration::FindRevisitNode(poses, stamps, 11) == 1, "node 11 looks back to node 1 (9 is 20 s away)");
  expect(registration::FindRevisitNode(poses, stamps, 2) == 8, "node 2: node 8 is 0.5 m off and 60 s away, exactly: kept");
  expect(registration::FindRevisitNode(poses, stamps, 5) == 11, "node 5: only node 11 is 60 s away");
  std::vector<Rigid3d> few(poses.begin(), poses.begin() + 6);
  std::vector<int64_t> few_stamps(stamps.begin(), stamps.begin() + 6);
  expect(registration::FindRevisitNode(few, few_stamps, 2) == -1, "no node 60 s away: none is reported");
  expect(registration::FindRevisitNode(few, few_stamps, 0) == -1, "50 s is not enough");
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
