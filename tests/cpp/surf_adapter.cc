// mapping::constraints::SubmapFeatureMatcher::AddSubmap(id, HybridGrid, global_submap_pose, ...) of dliom_cartographer.h:
//
//   surf_adapter <scans>      scans: int32 n, then n x (int32 points, float origin[3], points x float xyz), world frame
//
// Inserts the scans into one grid as they are and into a second one with the world turned by a right angle about z
// ((x, y) -> (-y, x)), adds the first as submap (0, 0) and the second as (1, 0), both at the identity pose, and prints the
// second call's result: the number of matched submaps, the first one's trajectory id, and theta, tx, ty of its
// dliom_submap_match (%.17g).
#include <cstdio>
#include <cstring>
#include <vector>

#include "dliom_cartographer.h"

int main(int argc, char** argv) {
  using dliom::mapping::SubmapId;
  namespace constraints = dliom::mapping::constraints;
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) return 2;
  int32_t num_scans = 0;
  if (std::fread(&num_scans, 4, 1, f) != 1) return 2;
  dliom::Context context(0);
  dliom::mapping::HybridGrid straight(&context, 0.1f), turned(&context, 0.1f);
  dliom::mapping::RangeDataInserter3D inserter(&context, {0.55, 0.49, 2});
  for (int s = 0; s < num_scans; ++s) {
    int32_t n = 0;
    float origin[3];
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(origin, 4, 3, f) != 3) return 2;
    std::vector<float> xyz(3 * static_cast<size_t>(n));
    if (std::fread(xyz.data(), 4, xyz.size(), f) != xyz.size()) return 2;
    dliom::sensor::RangeData a, b;
    a.origin = {origin[0], origin[1], origin[2]};
    b.origin = {-origin[1], origin[0], origin[2]};
    for (int k = 0; k < n; ++k) {
      a.returns.push_back({xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]});
      b.returns.push_back({-xyz[3 * k + 1], xyz[3 * k], xyz[3 * k + 2]});
    }
    inserter.Insert(a, &straight);
    inserter.Insert(b, &turned);
  }
  std::fclose(f);
  const constraints::FeatureMatchOptions options{0.5, 5, 3.0, 0.1, 7};
  const dliom_surf_options surf = dliom_surf_default_options();
  const dliom::transform::Rigid3d identity = dliom::transform::Embed3D(0.0, 0.0, 0.0);
  constraints::SubmapFeatureMatcher matcher(&context, DLIOM_SURF_DESCRIPTOR_SIZE);
  if (!matcher.AddSubmap(SubmapId{0, 0}, straight, identity, surf, options).empty()) return 3;
  std::map<SubmapId, dliom_submap_match> results;
  const auto matched = matcher.AddSubmap(SubmapId{1, 0}, turned, identity, surf, options, &results);
  if (matched.empty()) {
    std::printf("0 -1 0 0 0\n");
    return 0;
  }
  const dliom_submap_match& m = results.at(matched.begin()->first);
  std::printf("%d %d %.17g %.17g %.17g\n", static_cast<int>(matched.size()), matched.begin()->first.trajectory_id, m.theta, m.tx,
              m.ty);
  return 0;
}
