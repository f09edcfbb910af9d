// CPU model of the two points-processor stages that libdliom runs on the device (csrc/outlier.hip), for
// tests/test_outlier_host.py, tests/test_gpu_outlier.py, tools/fuzz_outlier.py and tools/outlier_bench.py: a
// restatement, with line citations, of
//   io/outlier_removing_points_processor.{h,cc}        OutlierRemovingPointsProcessor (three phases over VoxelData)
//   io/min_max_range_filtering_points_processor.cc     MinMaxRangeFiteringPointsProcessor::Process
//   io/points_batch.cc:22-49                           RemovePoints (survivors keep their order)
//   mapping/3d/hybrid_grid.h                           GetCellIndex (:430-434), value() outside the grid (:266-271),
//                                                      Grow()'s CHECK_LE(new_bits, 8) (:389)
// The grid is a std::map keyed by (z, y, x), so no detail of the device's table is shared with it.  Eigen's orders are
// written out: Vector3f::norm() is sqrt(x*x + (y*y + z*z)).  Build: g++ -std=c++17 -O2 -ffp-contract=off -Wall -Werror.
//
//   outlier_model ops.bin out.bin [--time]
//
// ops.bin: double voxel_size, then operations until the end of the file.  Each: int32 op, float origin[3],
//   double a, double b, int32 n, n * 3 floats (points in the map frame).
//     op 1  ProcessInPhaseOne     out: int32 status
//     op 2  ProcessInPhaseTwo     out: int32 status
//     op 3  ProcessInPhaseThree   out: int32 status, int32 kept, kept * int32 input indices
//     op 4  min/max range filter, min_range = a, max_range = b          out: as op 3
//     op 5  the samples of every ray, without touching the grid         out: per ray int32 samples, then per sample
//           3 * int32 cell index and 3 * int32 cell index of the product form x = k * float(voxel_size)
//   status: 0; -6 a hit outside [-8192, 8191] (the reference aborts, hybrid_grid.h:389); -1 a non-finite coordinate
//   (lround undefined); -7 a ray of voxel_size * 2^24 or more (the loop at .cc:98 stops advancing).  The grid is
//   unchanged after a status other than 0.
// out.bin ends with the grid: int64 count, then per voxel with hits > 0, sorted by (z, y, x): int32 x, y, z, hits, rays.
// --time prints the seconds spent in each op kind to stdout (one thread): "phase1 s phase2 s phase3 s samples".
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

struct VoxelData {  // outlier_removing_points_processor.h:55-58
  int hits = 0;
  int rays = 0;
};
using Index = std::array<long, 3>;  // (z, y, x)
using Vector3f = std::array<float, 3>;

constexpr long kMinIndex = -8192, kMaxIndex = 8191;  // grid_size() = 64 << 8 at bits_ == 8, shifted by half of it

struct Model {
  double voxel_size_;                 // .h:79
  float resolution_;                  // voxels_(voxel_size_): HybridGridBase(const float resolution), hybrid_grid.h:423
  std::map<Index, VoxelData> voxels_;
  int64_t samples = 0;

  // hybrid_grid.h:430-434 and common/port.h RoundToInt = lround; false where the grid has no such cell
  bool GetCellIndex(const Vector3f& point, Index* index) const {
    for (int k = 0; k < 3; ++k) {
      const float q = point[k] / resolution_;
      if (!(std::fabs(q) < 1e9f)) return false;
      const long c = std::lround(q);
      if (c < kMinIndex || c > kMaxIndex) return false;
      (*index)[2 - k] = c;
    }
    return true;
  }
  static bool Finite(const Vector3f& p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }
  static float Norm(const Vector3f& d) { return std::sqrt(d[0] * d[0] + (d[1] * d[1] + d[2] * d[2])); }

  int PhaseOne(const std::vector<Vector3f>& points) {  // .cc:84-90
    Index index;
    for (const Vector3f& p : points)
      if (!Finite(p)) return -1;
    for (const Vector3f& p : points)
      if (!GetCellIndex(p, &index)) return -6;  // mutable_value -> Grow() -> CHECK_LE(new_bits, 8)
    for (const Vector3f& p : points) {
      GetCellIndex(p, &index);
      ++voxels_[index].hits;
    }
    return 0;
  }

  int PhaseTwo(const Vector3f& origin, const std::vector<Vector3f>& points) {  // .cc:92-108
    if (!Finite(origin)) return -1;
    for (const Vector3f& p : points) {
      if (!Finite(p)) return -1;
    }
    for (const Vector3f& p : points) {
      const Vector3f delta{p[0] - origin[0], p[1] - origin[1], p[2] - origin[2]};
      if (!(static_cast<double>(Norm(delta)) < voxel_size_ * 16777216.0)) return -7;
    }
    for (const Vector3f& p : points) {
      const Vector3f delta{p[0] - origin[0], p[1] - origin[1], p[2] - origin[2]};
      const float length = Norm(delta);
      for (float x = 0; x < length; x += voxel_size_) {  // float += double: x = float(double(x) + voxel_size_)
        ++samples;
        const float s = x / length;
        const Vector3f sample{origin[0] + s * delta[0], origin[1] + s * delta[1], origin[2] + s * delta[2]};
        Index index;
        if (!GetCellIndex(sample, &index)) continue;  // value(): ValueType() outside the grid
        const auto it = voxels_.find(index);
        if (it != voxels_.end() && it->second.hits > 0) ++it->second.rays;
      }
    }
    return 0;
  }

  int PhaseThree(const std::vector<Vector3f>& points, std::vector<int32_t>* kept) const {  // .cc:110-124
    constexpr double kMissPerHitLimit = 3;
    for (const Vector3f& p : points)
      if (!Finite(p)) return -1;
    for (size_t i = 0; i < points.size(); ++i) {
      VoxelData voxel;
      Index index;
      if (GetCellIndex(points[i], &index)) {
        const auto it = voxels_.find(index);
        if (it != voxels_.end()) voxel = it->second;
      }
      if (!(voxel.rays < kMissPerHitLimit * voxel.hits)) continue;  // to_remove
      kept->push_back(static_cast<int32_t>(i));
    }
    return 0;
  }

  // min_max_range_filtering_points_processor.cc:40-51
  static void MinMaxRange(const Vector3f& origin, const std::vector<Vector3f>& points, double min_range_, double max_range_,
                          std::vector<int32_t>* kept) {
    for (size_t i = 0; i < points.size(); ++i) {
      const Vector3f delta{points[i][0] - origin[0], points[i][1] - origin[1], points[i][2] - origin[2]};
      const float range = Norm(delta);
      if (!(min_range_ <= range && range <= max_range_)) continue;
      kept->push_back(static_cast<int32_t>(i));
    }
  }
};

void Put(std::FILE* f, const void* p, size_t bytes) { std::fwrite(p, 1, bytes, f); }
void PutInt(std::FILE* f, int32_t v) { Put(f, &v, 4); }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s ops.bin out.bin [--time]\n", argv[0]);
    return 2;
  }
  const bool timing = argc > 3 && std::string(argv[3]) == "--time";
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (in == nullptr || out == nullptr) return 2;
  Model m;
  if (std::fread(&m.voxel_size_, 8, 1, in) != 1) return 2;
  m.resolution_ = static_cast<float>(m.voxel_size_);
  double seconds[6] = {};
  for (;;) {
    int32_t op, n;
    Vector3f origin;
    double a, b;
    if (std::fread(&op, 4, 1, in) != 1) break;
    if (std::fread(origin.data(), 4, 3, in) != 3 || std::fread(&a, 8, 1, in) != 1 || std::fread(&b, 8, 1, in) != 1 ||
        std::fread(&n, 4, 1, in) != 1 || n < 0 || op < 1 || op > 5)
      return 2;
    std::vector<Vector3f> points(static_cast<size_t>(n));
    if (n > 0 && std::fread(points.data(), 12, points.size(), in) != points.size()) return 2;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> kept;
    int status = 0;
    if (op == 1) status = m.PhaseOne(points);
    if (op == 2) status = m.PhaseTwo(origin, points);
    if (op == 3) status = m.PhaseThree(points, &kept);
    if (op == 4) Model::MinMaxRange(origin, points, a, b, &kept);
    seconds[op] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (op <= 4) PutInt(out, status);
    if (op == 3 || op == 4) {
      if (status != 0) kept.clear();
      PutInt(out, static_cast<int32_t>(kept.size()));
      Put(out, kept.data(), kept.size() * 4);
    }
    if (op == 5) {
      for (const Vector3f& p : points) {
        const Vector3f delta{p[0] - origin[0], p[1] - origin[1], p[2] - origin[2]};
        const float length = Model::Norm(delta);
        std::vector<int32_t> cells;
        int k = 0;
        for (float x = 0; x < length; x += m.voxel_size_, ++k) {
          const float xs[2] = {x, static_cast<float>(k) * m.resolution_};
          for (const float xv : xs) {
            const float s = xv / length;
            for (int c = 0; c < 3; ++c) cells.push_back(static_cast<int32_t>(std::lround((origin[c] + s * delta[c]) / m.resolution_)));
          }
        }
        PutInt(out, k);
        Put(out, cells.data(), cells.size() * 4);
      }
    }
  }
  int64_t count = 0;
  for (const auto& v : m.voxels_) count += v.second.hits > 0;
  Put(out, &count, 8);
  for (const auto& v : m.voxels_) {
    if (v.second.hits <= 0) continue;
    const int32_t row[5] = {static_cast<int32_t>(v.first[2]), static_cast<int32_t>(v.first[1]), static_cast<int32_t>(v.first[0]),
                            v.second.hits, v.second.rays};
    Put(out, row, sizeof row);
  }
  std::fclose(in);
  std::fclose(out);
  if (timing) std::printf("phase1 %.6f phase2 %.6f phase3 %.6f samples %lld\n", seconds[1], seconds[2], seconds[3],
                          static_cast<long long>(m.samples));
  return 0;
}
