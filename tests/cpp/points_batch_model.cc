// CPU model of the points-processor stages that dliom_points_batch runs on the device, written for the tests from the
// reference's loops; it shares no code with the library.
//   RemovePoints                         io/points_batch.cc:22-49 (points, intensities, colors)
//   common::FixedRatioSampler::Pulse     common/fixed_ratio_sampler.cc:32-39
//   ColoringPointsProcessor              io/coloring_points_processor.cc:45-53
//   IntensityToColorPointsProcessor      io/intensity_to_color_points_processor.cc:47-58
//   ToUint8Color                         io/color.h:35-45
//   the PLY / PCD record loops           io/ply_writing_points_processor.cc:138-147, io/pcd_writing_points_processor.cc:121-128
//   the PLY / PCD headers                io/ply_writing_points_processor.cc:35-56, io/pcd_writing_points_processor.cc:35-57
// Build: g++ -std=c++17 -O2 -ffp-contract=off.   Usage: points_batch_model OPS OUT [--time]
// OPS is a sequence of records, each an int32 opcode followed by its operands (little-endian, packed); OUT receives the
// results back to back.  --time prints the seconds the ops took (tools/points_batch_bench.py).
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iomanip>
#include <sstream>
#include <string>
#include <unordered_set>
#include <vector>

namespace {

using FloatColor = std::array<float, 3>;
using Uint8Color = std::array<uint8_t, 3>;
struct Point {
  float x, y, z;
};

struct PointsBatch {
  std::vector<Point> points;
  std::vector<float> intensities;
  std::vector<FloatColor> colors;
};

// io/points_batch.cc:22-49
void RemovePoints(std::unordered_set<int> to_remove, PointsBatch* batch) {
  const int new_num_points = static_cast<int>(batch->points.size() - to_remove.size());
  std::vector<Point> points;
  points.reserve(new_num_points);
  std::vector<float> intensities;
  if (!batch->intensities.empty()) intensities.reserve(new_num_points);
  std::vector<FloatColor> colors;
  if (!batch->colors.empty()) colors.reserve(new_num_points);
  for (size_t i = 0; i < batch->points.size(); ++i) {
    if (to_remove.count(static_cast<int>(i)) == 1) continue;
    points.push_back(batch->points[i]);
    if (!batch->colors.empty()) colors.push_back(batch->colors[i]);
    if (!batch->intensities.empty()) intensities.push_back(batch->intensities[i]);
  }
  batch->points = std::move(points);
  batch->intensities = std::move(intensities);
  batch->colors = std::move(colors);
}

// common/fixed_ratio_sampler.cc
struct FixedRatioSampler {
  double ratio_;
  int64_t num_pulses_ = 0, num_samples_ = 0;
  bool Pulse() {
    ++num_pulses_;
    if (static_cast<double>(num_samples_) / num_pulses_ < ratio_) {
      ++num_samples_;
      return true;
    }
    return false;
  }
};

// common/math.h:32-40
template <typename T>
T Clamp(const T value, const T min, const T max) {
  if (value > max) return max;
  if (value < min) return min;
  return value;
}

// io/color.h:35-45
uint8_t FloatComponentToUint8(float c) { return static_cast<uint8_t>(std::lround(Clamp(c, 0.f, 1.f) * 255)); }
Uint8Color ToUint8Color(const FloatColor& color) {
  return {{FloatComponentToUint8(color[0]), FloatComponentToUint8(color[1]), FloatComponentToUint8(color[2])}};
}

void Write(std::vector<char>* file, const void* data, size_t n) {
  const char* c = static_cast<const char*>(data);
  file->insert(file->end(), c, c + n);
}

void WritePoint(std::vector<char>* file, const Point& p) {
  char buffer[12];
  std::memcpy(buffer, &p.x, 4);
  std::memcpy(buffer + 4, &p.y, 4);
  std::memcpy(buffer + 8, &p.z, 4);
  Write(file, buffer, 12);
}

void PlyRecords(const PointsBatch& batch, bool has_colors, bool has_intensities, std::vector<char>* file) {
  for (size_t i = 0; i < batch.points.size(); ++i) {
    WritePoint(file, batch.points[i]);
    if (has_colors) {
      const Uint8Color c = ToUint8Color(batch.colors[i]);
      Write(file, c.data(), c.size());
    }
    if (has_intensities) Write(file, &batch.intensities[i], sizeof(float));
  }
}

void PcdRecords(const PointsBatch& batch, std::vector<char>* file) {
  for (size_t i = 0; i < batch.points.size(); ++i) {
    WritePoint(file, batch.points[i]);
    if (!batch.colors.empty()) {
      const Uint8Color color = ToUint8Color(batch.colors[i]);
      char buffer[4];
      buffer[0] = color[2];
      buffer[1] = color[1];
      buffer[2] = color[0];
      buffer[3] = 0;
      Write(file, buffer, 4);
    }
  }
}

std::string PlyHeader(bool has_color, bool has_intensities, int64_t num_points) {
  const std::string color_header = !has_color ? ""
                                              : "property uchar red\n"
                                                "property uchar green\n"
                                                "property uchar blue\n";
  const std::string intensity_header = !has_intensities ? "" : "property float intensity\n";
  std::ostringstream stream;
  stream << "ply\n"
         << "format binary_little_endian 1.0\n"
         << "comment generated by Cartographer\n"
         << "element vertex " << std::setw(15) << std::setfill('0') << num_points << "\n"
         << "property float x\n"
         << "property float y\n"
         << "property float z\n"
         << color_header << intensity_header << "end_header\n";
  return stream.str();
}

std::string PcdHeader(bool has_color, int64_t num_points) {
  std::string color_header_field = !has_color ? "" : " rgb";
  std::string color_header_type = !has_color ? "" : " U";
  std::string color_header_size = !has_color ? "" : " 4";
  std::string color_header_count = !has_color ? "" : " 1";
  std::ostringstream stream;
  stream << "# generated by Cartographer\n"
         << "VERSION .7\n"
         << "FIELDS x y z" << color_header_field << "\n"
         << "SIZE 4 4 4" << color_header_size << "\n"
         << "TYPE F F F" << color_header_type << "\n"
         << "COUNT 1 1 1" << color_header_count << "\n"
         << "WIDTH " << std::setw(15) << std::setfill('0') << num_points << "\n"
         << "HEIGHT 1\n"
         << "VIEWPOINT 0 0 0 1 0 0 0\n"
         << "POINTS " << std::setw(15) << std::setfill('0') << num_points << "\n"
         << "DATA binary\n";
  return stream.str();
}

enum { kRemove = 1, kPulse = 2, kColor = 3, kIntensityToColor = 4, kPack = 5, kHeader = 6 };

struct Reader {
  std::vector<char> data;
  size_t at = 0;
  template <typename T>
  T get() {
    T v;
    std::memcpy(&v, data.data() + at, sizeof v);
    at += sizeof v;
    return v;
  }
  template <typename T>
  void fill(std::vector<T>* v, size_t n) {
    v->resize(n);
    if (n > 0) std::memcpy(static_cast<void*>(v->data()), data.data() + at, n * sizeof(T));
    at += n * sizeof(T);
  }
  // a batch: n, has_intensities, num_colors, then the arrays that exist
  PointsBatch batch() {
    PointsBatch b;
    const int64_t n = get<int64_t>();
    const int32_t has_intensities = get<int32_t>();
    const int64_t num_colors = get<int64_t>();
    fill(&b.points, n);
    if (has_intensities) fill(&b.intensities, n);
    fill(&b.colors, num_colors);
    return b;
  }
};

template <typename T>
void put(std::vector<char>* out, const T& v) {
  Write(out, &v, sizeof v);
}

void put_batch(std::vector<char>* out, const PointsBatch& b) {
  put<int64_t>(out, b.points.size());
  put<int64_t>(out, b.intensities.size());
  put<int64_t>(out, b.colors.size());
  Write(out, b.points.data(), b.points.size() * sizeof(Point));
  Write(out, b.intensities.data(), b.intensities.size() * 4);
  Write(out, b.colors.data(), b.colors.size() * 12);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  Reader in;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (f == nullptr) return 2;
    char buffer[1 << 16];
    size_t got;
    while ((got = std::fread(buffer, 1, sizeof buffer, f)) > 0) in.data.insert(in.data.end(), buffer, buffer + got);
    std::fclose(f);
  }
  std::vector<char> out;
  const auto t0 = std::chrono::steady_clock::now();
  while (in.at < in.data.size()) {
    const int32_t op = in.get<int32_t>();
    if (op == kRemove) {  // batch, keep flags (one byte a point) -> batch
      PointsBatch b = in.batch();
      std::vector<uint8_t> keep;
      in.fill(&keep, b.points.size());
      std::unordered_set<int> to_remove;
      for (size_t i = 0; i < keep.size(); ++i)
        if (!keep[i]) to_remove.insert(static_cast<int>(i));
      RemovePoints(to_remove, &b);
      put_batch(&out, b);
    } else if (op == kPulse) {  // ratio, num_pulses, num_samples, n -> n keep bytes, num_pulses, num_samples
      FixedRatioSampler s{in.get<double>()};
      s.num_pulses_ = in.get<int64_t>();
      s.num_samples_ = in.get<int64_t>();
      const int64_t n = in.get<int64_t>();
      for (int64_t i = 0; i < n; ++i) put<uint8_t>(&out, s.Pulse() ? 1 : 0);
      put<int64_t>(&out, s.num_pulses_);
      put<int64_t>(&out, s.num_samples_);
    } else if (op == kColor) {  // batch, rgb -> batch
      PointsBatch b = in.batch();
      FloatColor color_;
      for (int k = 0; k < 3; ++k) color_[k] = in.get<float>();
      b.colors.clear();
      for (size_t i = 0; i < b.points.size(); ++i) b.colors.push_back(color_);
      put_batch(&out, b);
    } else if (op == kIntensityToColor) {  // batch, min, max -> batch
      PointsBatch b = in.batch();
      const float min_intensity_ = in.get<float>(), max_intensity_ = in.get<float>();
      if (!b.intensities.empty()) {
        b.colors.clear();
        for (const float intensity : b.intensities) {
          const float gray = Clamp((intensity - min_intensity_) / (max_intensity_ - min_intensity_), 0.f, 1.f);
          b.colors.push_back({{gray, gray, gray}});
        }
      }
      put_batch(&out, b);
    } else if (op == kPack) {  // batch, format (0 PLY, 1 PCD), has_colors, has_intensities -> int64 bytes, the bytes
      PointsBatch b = in.batch();
      const int32_t format = in.get<int32_t>(), has_colors = in.get<int32_t>(), has_intensities = in.get<int32_t>();
      std::vector<char> file;
      if (format == 0) PlyRecords(b, has_colors != 0, has_intensities != 0, &file);
      else PcdRecords(b, &file);
      put<int64_t>(&out, file.size());
      Write(&out, file.data(), file.size());
    } else if (op == kHeader) {  // format, has_colors, has_intensities, count -> int64 length, the text
      const int32_t format = in.get<int32_t>(), has_colors = in.get<int32_t>(), has_intensities = in.get<int32_t>();
      const int64_t count = in.get<int64_t>();
      const std::string text = format == 0 ? PlyHeader(has_colors != 0, has_intensities != 0, count) : PcdHeader(has_colors != 0, count);
      put<int64_t>(&out, text.size());
      Write(&out, text.data(), text.size());
    } else {
      return 3;
    }
  }
  const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  FILE* f = std::fopen(argv[2], "wb");
  if (f == nullptr) return 2;
  std::fwrite(out.data(), 1, out.size(), f);
  std::fclose(f);
  if (argc > 3 && std::strcmp(argv[3], "--time") == 0) std::printf("%.9f\n", seconds);
  return 0;
}
