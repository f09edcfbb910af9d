// mapping::constraints::SubmapFeatureMatcher of dliom_cartographer.h over the sets of a model input file
// (tests/cpp/feature_match_model.cc, mode 2):
//
//   feature_match_adapter <input> <output> <trajectory_id submap_index> ...   (one id a set, in the file's order)
//
// Adds every set but the query in the file's order, then the query, and writes the query's matched_submaps: int32 n, then
// n x (int32 trajectory_id, int32 submap_index, double pose[7]); then deletes the first matched submap, adds the query's
// features again under the id (99, 0) and writes that call's matched_submaps the same way.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dliom_cartographer.h"

namespace {
struct Set {
  std::vector<dliom::mapping::constraints::KeyPoint> key_points;
  std::vector<float> descriptors;
  double ox, oy, resolution;
};

template <class T>
T take(const std::vector<unsigned char>& data, size_t* at) {
  T v;
  if (*at + sizeof(T) > data.size()) std::abort();
  std::memcpy(&v, data.data() + *at, sizeof(T));
  *at += sizeof(T);
  return v;
}

void write_matches(FILE* f, const std::map<dliom::mapping::SubmapId, dliom::transform::Rigid3d>& matched) {
  const int32_t n = static_cast<int32_t>(matched.size());
  std::fwrite(&n, 4, 1, f);
  for (const auto& e : matched) {
    const int32_t id[2] = {e.first.trajectory_id, e.first.submap_index};
    const std::array<double, 7> pose = e.second.ToArray();
    std::fwrite(id, 4, 2, f);
    std::fwrite(pose.data(), 8, 7, f);
  }
}
}  // namespace

int main(int argc, char** argv) {
  using dliom::mapping::SubmapId;
  namespace constraints = dliom::mapping::constraints;
  if (argc < 3) return 2;
  std::vector<unsigned char> data;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (f == nullptr) return 2;
    std::fseek(f, 0, SEEK_END);
    data.resize(static_cast<size_t>(std::ftell(f)));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(data.data(), 1, data.size(), f) != data.size()) return 2;
    std::fclose(f);
  }
  size_t at = 0;
  if (take<int32_t>(data, &at) != 2) return 2;
  const int D = take<int32_t>(data, &at), num_sets = take<int32_t>(data, &at), query = take<int32_t>(data, &at);
  const int num_train = take<int32_t>(data, &at);
  const dliom_feature_match_options o = take<dliom_feature_match_options>(data, &at);
  at += 4 * static_cast<size_t>(num_train);
  if (argc != 3 + 2 * num_sets) return 2;
  std::vector<Set> sets(num_sets);
  for (Set& s : sets) {
    const int count = take<int32_t>(data, &at);
    (void)take<int32_t>(data, &at);
    s.ox = take<double>(data, &at);
    s.oy = take<double>(data, &at);
    s.resolution = take<double>(data, &at);
    s.descriptors.resize(static_cast<size_t>(count) * D);
    for (float& v : s.descriptors) v = take<float>(data, &at);
    s.key_points.resize(count);
    for (auto& k : s.key_points) {
      k.x = take<float>(data, &at);
      k.y = take<float>(data, &at);
    }
  }
  const constraints::FeatureMatchOptions options{o.good_match_ratio_of_distance, o.minimum_good_match_num, o.ransac_threshold,
                                                 o.scale_estimated_tolerance, o.seed};
  dliom::Context context(0);
  constraints::SubmapFeatureMatcher matcher(&context, D);
  auto id_of = [&](int k) { return SubmapId{std::atoi(argv[3 + 2 * k]), std::atoi(argv[4 + 2 * k])}; };
  for (int k = 0; k < num_sets; ++k) {
    if (k == query) continue;
    (void)matcher.AddSubmap(id_of(k), sets[k].key_points, sets[k].descriptors.data(), sets[k].ox, sets[k].oy, sets[k].resolution,
                            options);
  }
  const Set& q = sets[query];
  const auto matched = matcher.AddSubmap(id_of(query), q.key_points, q.descriptors.data(), q.ox, q.oy, q.resolution, options);
  FILE* f = std::fopen(argv[2], "wb");
  if (f == nullptr) return 2;
  write_matches(f, matched);
  if (!matched.empty()) matcher.DeleteSubmap(matched.begin()->first);
  matcher.DeleteSubmap(id_of(query));
  write_matches(f, matcher.AddSubmap(SubmapId{99, 0}, q.key_points, q.descriptors.data(), q.ox, q.oy, q.resolution, options));
  std::fclose(f);
  return 0;
}
