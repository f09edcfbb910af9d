// CPU model of the X-ray stage that libdliom runs on the device (csrc/points_xray.hip), for
// tests/test_points_xray_host.py, tests/test_gpu_points_xray.py, tools/fuzz_points_xray.py and
// tools/points_xray_bench.py: a restatement, with line citations, of
//   io/xray_points_processor.{h,cc}   Insert (:195-213), WriteVoxels (:144-175), IntoImage and Mix (:46-84)
//   io/color.h:35-38                  FloatComponentToUint8
//   io/image.cc                       Uint8ColorToCairo: 0xFF000000 | r << 16 | g << 8 | b, pixels_[y * width + x]
//   mapping/3d/hybrid_grid.h          GetCellIndex (:430-434), Grow()'s CHECK_LE(new_bits, 8) (:389)
// The voxels are a std::set keyed by (z, y, x) and the columns a std::map keyed by (y, z), so no detail of the device's
// tables is shared with it.  Eigen's orders are written out: Rigid3f * v is rotation * v + translation, and
// Quaternionf * v is uv = q.vec x v; uv += uv; (v + w * uv) + q.vec x uv.
// Build: g++ -std=c++17 -O2 -ffp-contract=off -Wall -Werror.
//
//   points_xray_model ops.bin out.bin [--time]
//
// ops.bin: double voxel_size, float transform[7] (tx ty tz qw qx qy qz), int32 number of aggregations (floors), then
// operations until the end of the file:
//     int32 1, int32 aggregation, int32 n, int32 num_colors (0, 1 or n), n * 3 floats, num_colors * 3 floats
//                                                                       out: int32 status
//     int32 2, int32 k, k * {uint32 occupied, uint32 max_occupied, float mean[3]}   (IntoImage's pixel expression alone)
//                                                                       out: k * uint32 pixel
//   status: 0; -6 a cell outside [-8192, 8191] (the reference aborts); -1 a non-finite camera point (lround undefined).
//   Nothing changes after a status other than 0.
// out.bin ends with: the shared bounding box (int32 empty, min[3], max[3]), then per aggregation
//     its own box in the same form,
//     int64 columns, per column sorted by (y, z): int32 y, z, float sum_r, sum_g, sum_b, uint32 count, uint32 occupied,
//     int64 voxels, per voxel sorted by (z, y, x): int32 x, y, z,
//     int32 width, height, width * height uint32 pixels: the image in the shared box (0, 0: "Not writing output").
// --time prints "insert <seconds> draw <seconds>" (one thread) to stdout.
#include <array>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace {

using Vector3f = std::array<float, 3>;
using Index = std::array<int, 3>;  // (x, y, z)
constexpr long kMinIndex = -8192, kMaxIndex = 8191;

struct ColumnData {  // .h:61-66
  float sum_r = 0.;
  float sum_g = 0.;
  float sum_b = 0.;
  uint32_t count = 0;
};

struct Box {  // Eigen::AlignedBox3i
  Index min{INT_MAX, INT_MAX, INT_MAX}, max{INT_MIN, INT_MIN, INT_MIN};
  bool isEmpty() const { return min[0] > max[0] || min[1] > max[1] || min[2] > max[2]; }
  void extend(const Index& p) {
    for (int k = 0; k < 3; ++k) {
      if (p[k] < min[k]) min[k] = p[k];
      if (p[k] > max[k]) max[k] = p[k];
    }
  }
};

struct Aggregation {  // .h:68-71
  std::set<std::array<int, 3>> voxels;  // (z, y, x)
  std::map<std::pair<int, int>, ColumnData> column_data;
  Box own_box;  // not in the reference: what this aggregation alone would extend
};

struct Pixel {  // PixelData (.cc:36-41)
  size_t num_occupied_cells_in_column = 0;
  float mean_r = 0.;
  float mean_g = 0.;
  float mean_b = 0.;
};

float Mix(const float a, const float b, const float t) { return a * (1. - t) + t * b; }  // .cc:46-48

uint32_t Component(float c) {  // FloatComponentToUint8
  const float clamped = c > 1.f ? 1.f : (c < 0.f ? 0.f : c);
  return static_cast<uint8_t>(std::lround(clamped * 255));
}

uint32_t Paint(const Pixel& cell, float max) {  // .cc:67-80
  if (cell.num_occupied_cells_in_column == 0.) return 0xFFFFFFFFu;
  const float saturation = std::log(cell.num_occupied_cells_in_column) / max;
  return 0xFF000000u | (Component(Mix(1.f, cell.mean_r, saturation)) << 16) | (Component(Mix(1.f, cell.mean_g, saturation)) << 8) |
         Component(Mix(1.f, cell.mean_b, saturation));
}

struct Model {
  float resolution_;  // HybridGridBase<bool>(voxel_size): float
  float t_[3], w_, qx_, qy_, qz_;
  std::vector<Aggregation> aggregations_;
  Box bounding_box_;

  Vector3f Camera(const Vector3f& v) const {  // transform_ * batch.points[i]
    float uvx = qy_ * v[2] - qz_ * v[1], uvy = qz_ * v[0] - qx_ * v[2], uvz = qx_ * v[1] - qy_ * v[0];
    uvx += uvx;
    uvy += uvy;
    uvz += uvz;
    const float cx = qy_ * uvz - qz_ * uvy, cy = qz_ * uvx - qx_ * uvz, cz = qx_ * uvy - qy_ * uvx;
    return Vector3f{((v[0] + w_ * uvx) + cx) + t_[0], ((v[1] + w_ * uvy) + cy) + t_[1], ((v[2] + w_ * uvz) + cz) + t_[2]};
  }
  bool GetCellIndex(const Vector3f& point, Index* index) const {  // hybrid_grid.h:430-434; false: no such cell
    for (int k = 0; k < 3; ++k) {
      const float q = point[k] / resolution_;
      if (!(std::fabs(q) < 1e9f)) return false;
      const long c = std::lround(q);
      if (c < kMinIndex || c > kMaxIndex) return false;
      (*index)[k] = static_cast<int>(c);
    }
    return true;
  }

  int Insert(const std::vector<Vector3f>& points, const std::vector<Vector3f>& colors, Aggregation* aggregation) {  // .cc:195-213
    Index cell_index;
    for (const Vector3f& p : points) {
      const Vector3f c = Camera(p);
      if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2])) return -1;
    }
    for (const Vector3f& p : points)
      if (!GetCellIndex(Camera(p), &cell_index)) return -6;  // mutable_value -> Grow() -> CHECK_LE(new_bits, 8)
    const Vector3f kDefaultColor{0.f, 0.f, 0.f};
    for (size_t i = 0; i < points.size(); ++i) {
      const Vector3f camera_point = Camera(points[i]);
      GetCellIndex(camera_point, &cell_index);
      aggregation->voxels.insert({cell_index[2], cell_index[1], cell_index[0]});
      bounding_box_.extend(cell_index);
      aggregation->own_box.extend(cell_index);
      ColumnData& column_data = aggregation->column_data[std::make_pair(cell_index[1], cell_index[2])];
      const Vector3f& color = colors.empty() ? kDefaultColor : (colors.size() == 1 ? colors[0] : colors.at(i));
      column_data.sum_r += color[0];
      column_data.sum_g += color[1];
      column_data.sum_b += color[2];
      ++column_data.count;
    }
    return 0;
  }

  // WriteVoxels (.cc:144-175) and IntoImage (.cc:51-84); false: "Not writing output: bounding box is empty."
  bool Draw(const Aggregation& aggregation, int* width, int* height, std::vector<uint32_t>* image) const {
    *width = *height = 0;
    image->clear();
    if (bounding_box_.isEmpty()) return false;
    const int xsize = bounding_box_.max[1] - bounding_box_.min[1] + 1;
    const int ysize = bounding_box_.max[2] - bounding_box_.min[2] + 1;
    std::vector<Pixel> mat(static_cast<size_t>(xsize) * ysize);
    for (const auto& v : aggregation.voxels) {
      const int px = bounding_box_.max[1] - v[1], py = bounding_box_.max[2] - v[0];  // voxel_index_to_pixel: y flipped
      Pixel& pixel_data = mat[static_cast<size_t>(py) * xsize + px];
      const ColumnData& column_data = aggregation.column_data.at(std::make_pair(v[1], v[0]));
      pixel_data.mean_r = column_data.sum_r / column_data.count;
      pixel_data.mean_g = column_data.sum_g / column_data.count;
      pixel_data.mean_b = column_data.sum_b / column_data.count;
      ++pixel_data.num_occupied_cells_in_column;
    }
    float max = std::numeric_limits<float>::min();
    for (const Pixel& cell : mat) {
      if (cell.num_occupied_cells_in_column == 0.) continue;
      max = std::max<float>(max, std::log(cell.num_occupied_cells_in_column));
    }
    image->resize(mat.size());
    for (size_t i = 0; i < mat.size(); ++i) (*image)[i] = Paint(mat[i], max);
    *width = xsize;
    *height = ysize;
    return true;
  }
};

void Put(std::FILE* f, const void* p, size_t bytes) { std::fwrite(p, 1, bytes, f); }
void PutInt(std::FILE* f, int32_t v) { Put(f, &v, 4); }
void PutBox(std::FILE* f, const Box& b) {
  PutInt(f, b.isEmpty() ? 1 : 0);
  for (int k = 0; k < 3; ++k) PutInt(f, b.min[k]);
  for (int k = 0; k < 3; ++k) PutInt(f, b.max[k]);
}

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
  double voxel_size;
  float transform[7];
  int32_t floors;
  if (std::fread(&voxel_size, 8, 1, in) != 1 || std::fread(transform, 4, 7, in) != 7 || std::fread(&floors, 4, 1, in) != 1 || floors < 1)
    return 2;
  m.resolution_ = static_cast<float>(voxel_size);
  for (int k = 0; k < 3; ++k) m.t_[k] = transform[k];
  m.w_ = transform[3];
  m.qx_ = transform[4];
  m.qy_ = transform[5];
  m.qz_ = transform[6];
  m.aggregations_.resize(static_cast<size_t>(floors));
  double insert_seconds = 0.0, draw_seconds = 0.0;
  for (;;) {
    int32_t op;
    if (std::fread(&op, 4, 1, in) != 1) break;
    if (op == 1) {
      int32_t a, n, num_colors;
      if (std::fread(&a, 4, 1, in) != 1 || std::fread(&n, 4, 1, in) != 1 || std::fread(&num_colors, 4, 1, in) != 1 || a < 0 ||
          a >= floors || n < 0 || (num_colors != 0 && num_colors != 1 && num_colors != n))
        return 2;
      std::vector<Vector3f> points(static_cast<size_t>(n)), colors(static_cast<size_t>(num_colors));
      if (n > 0 && std::fread(points.data(), 12, points.size(), in) != points.size()) return 2;
      if (num_colors > 0 && std::fread(colors.data(), 12, colors.size(), in) != colors.size()) return 2;
      const auto t0 = std::chrono::steady_clock::now();
      const int status = m.Insert(points, colors, &m.aggregations_[static_cast<size_t>(a)]);
      insert_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      PutInt(out, status);
    } else if (op == 2) {
      int32_t k;
      if (std::fread(&k, 4, 1, in) != 1 || k < 0) return 2;
      for (int32_t i = 0; i < k; ++i) {
        uint32_t counts[2];
        float mean[3];
        if (std::fread(counts, 4, 2, in) != 2 || std::fread(mean, 4, 3, in) != 3) return 2;
        Pixel cell;
        cell.num_occupied_cells_in_column = counts[0];
        cell.mean_r = mean[0];
        cell.mean_g = mean[1];
        cell.mean_b = mean[2];
        float max = std::numeric_limits<float>::min();
        if (counts[1] != 0) max = std::max<float>(max, std::log(static_cast<size_t>(counts[1])));
        const uint32_t pixel = Paint(cell, max);
        Put(out, &pixel, 4);
      }
    } else {
      return 2;
    }
  }
  PutBox(out, m.bounding_box_);
  for (const Aggregation& a : m.aggregations_) {
    PutBox(out, a.own_box);
    std::map<std::pair<int, int>, uint32_t> occupied;
    for (const auto& v : a.voxels) ++occupied[std::make_pair(v[1], v[0])];
    const int64_t columns = static_cast<int64_t>(a.column_data.size());
    Put(out, &columns, 8);
    for (const auto& c : a.column_data) {
      PutInt(out, c.first.first);
      PutInt(out, c.first.second);
      Put(out, &c.second.sum_r, 4);
      Put(out, &c.second.sum_g, 4);
      Put(out, &c.second.sum_b, 4);
      Put(out, &c.second.count, 4);
      Put(out, &occupied[c.first], 4);
    }
    const int64_t voxels = static_cast<int64_t>(a.voxels.size());
    Put(out, &voxels, 8);
    for (const auto& v : a.voxels) {
      PutInt(out, v[2]);
      PutInt(out, v[1]);
      PutInt(out, v[0]);
    }
    int width, height;
    std::vector<uint32_t> image;
    const auto t0 = std::chrono::steady_clock::now();
    m.Draw(a, &width, &height, &image);
    draw_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    PutInt(out, width);
    PutInt(out, height);
    Put(out, image.data(), image.size() * 4);
  }
  std::fclose(in);
  std::fclose(out);
  if (timing) std::printf("insert %.6f draw %.6f\n", insert_seconds, draw_seconds);
  return 0;
}
