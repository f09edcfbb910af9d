// CPU model of the two X-ray projections for tests/test_gpu_xray.py and tests/test_xray_host.py: a restatement, with
// line citations, of the reference's float arithmetic over the cells of a serialized mapping::proto::HybridGrid
// (which lists them in HybridGrid::Iterator order, grid_proto.cc):
//   texture  AddToTextureProto without gzip (mapping/3d/submap_3d.cc:31-180): ExtractVoxelData, AccumulatePixelData,
//            ComputePixelValues, the slice pose
//   image    ProjectToCvMat (submap_3d.cc:381-443)
// Eigen's evaluation orders are written out (Eigen 3.3 on x86-64/SSE2: QuaternionBase::_transformVector, the SSE
// Quaternionf product and 4-lane normalisation, scalar Quaterniond ops).  Build: g++ -std=c++17 -O2 -ffp-contract=off.
//
//   xray_model texture|image grid.pb tx ty tz qw qx qy qz out.bin
//     out.bin: int32 width, int32 height, double resolution, then 7 doubles slice pose (texture) or 2 doubles ox, oy
//     (image), then the bytes (texture: height * width (value, alpha) pairs; image: height * width bytes)
//
// Built with -DXRAY_MODEL_EXHAUSTIVE and linked to libdliom.so, main() instead compares
// dliom_probability_to_log_odds_integer with ProbabilityToLogOddsInteger (mapping/submaps.h:37-52, glibc logf) for every
// float in [0.1, 0.9] and checks that the formula is monotone there with values 1..255.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

// probability_values.h:32-44, probability_values.cc:27-36
constexpr float kMinProbability = 0.1f;
constexpr float kMaxProbability = 1.f - kMinProbability;
int RoundToInt(float x) { return static_cast<int>(std::lround(x)); }  // common/port.h

// mapping/submaps.h:37-52
float Logit(float probability) { return std::log(probability / (1.f - probability)); }
float MinLogOdds() {
  volatile float p = kMinProbability;
  return Logit(p);
}
float MaxLogOdds() {
  volatile float p = kMaxProbability;
  return Logit(p);
}
int ProbabilityToLogOddsInteger(float probability) {
  static const float kMinLogOdds = MinLogOdds(), kMaxLogOdds = MaxLogOdds();
  return RoundToInt((Logit(probability) - kMinLogOdds) * 254.f / (kMaxLogOdds - kMinLogOdds)) + 1;
}

#ifndef XRAY_MODEL_EXHAUSTIVE

float ValueToProbability(uint32_t value) {  // kValueToProbability[value]: the table repeats above the update marker
  value &= 0x7FFFu;
  if (value == 0) return kMinProbability;
  const float kScale = (kMaxProbability - kMinProbability) / 32766.f;
  return value * kScale + (kMinProbability - kScale);
}
float ClampProbability(float p) { return p > kMaxProbability ? kMaxProbability : (p < kMinProbability ? kMinProbability : p); }

struct Cell {
  int32_t x, y, z;
  uint32_t value;
};

bool get_varint(const uint8_t*& p, const uint8_t* end, uint64_t* v) {
  *v = 0;
  for (int shift = 0; shift < 64 && p < end; shift += 7) {
    const uint8_t b = *p++;
    *v |= static_cast<uint64_t>(b & 0x7F) << shift;
    if ((b & 0x80) == 0) return true;
  }
  return false;
}

// mapping::proto::HybridGrid: 1 resolution (fixed32), 3/4/5 packed sint32 x/y/z, 6 packed int32 values
bool parse_grid(const std::vector<uint8_t>& buf, float* resolution, std::vector<Cell>* cells) {
  std::vector<int64_t> f[4];
  *resolution = 0.f;
  const uint8_t* p = buf.data();
  const uint8_t* end = p + buf.size();
  while (p < end) {
    uint64_t tag, v;
    if (!get_varint(p, end, &tag)) return false;
    const int field = static_cast<int>(tag >> 3), wire = static_cast<int>(tag & 7);
    auto take = [&](uint64_t raw) {
      if (field >= 3 && field <= 5) f[field - 3].push_back(static_cast<int32_t>((raw >> 1) ^ (~(raw & 1) + 1)));
      if (field == 6) f[3].push_back(static_cast<int64_t>(raw));
    };
    if (wire == 5) {
      if (end - p < 4) return false;
      if (field == 1) std::memcpy(resolution, p, 4);
      p += 4;
    } else if (wire == 0) {
      if (!get_varint(p, end, &v)) return false;
      take(v);
    } else if (wire == 2) {
      if (!get_varint(p, end, &v) || static_cast<uint64_t>(end - p) < v) return false;
      const uint8_t* q = p;
      p += v;
      while (q < p) {
        uint64_t e;
        if (!get_varint(q, p, &e)) return false;
        take(e);
      }
    } else {
      return false;
    }
  }
  const size_t n = f[3].size();
  if (f[0].size() != n || f[1].size() != n || f[2].size() != n) return false;
  for (size_t i = 0; i < n; ++i)
    cells->push_back(Cell{static_cast<int32_t>(f[0][i]), static_cast<int32_t>(f[1][i]), static_cast<int32_t>(f[2][i]),
                          static_cast<uint32_t>(f[3][i]) & 0xFFFFu});
  return true;
}

struct Qf {
  float w, x, y, z;
};
struct Qd {
  double w, x, y, z;
};
// QuaternionBase::_transformVector: uv = 2 (q.vec() x v); v + w uv + q.vec() x uv
void Rotate(const Qf& q, const float v[3], float out[3]) {
  float uv[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
  for (float& e : uv) e = e + e;
  const float c[3] = {q.y * uv[2] - q.z * uv[1], q.z * uv[0] - q.x * uv[2], q.x * uv[1] - q.y * uv[0]};
  out[0] = (v[0] + q.w * uv[0]) + c[0];
  out[1] = (v[1] + q.w * uv[1]) + c[1];
  out[2] = (v[2] + q.w * uv[2]) + c[2];
}
void Rotate(const Qd& q, const double v[3], double out[3]) {
  double uv[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
  for (double& e : uv) e = e + e;
  const double c[3] = {q.y * uv[2] - q.z * uv[1], q.z * uv[0] - q.x * uv[2], q.x * uv[1] - q.y * uv[0]};
  out[0] = (v[0] + q.w * uv[0]) + c[0];
  out[1] = (v[1] + q.w * uv[1]) + c[1];
  out[2] = (v[2] + q.w * uv[2]) + c[2];
}
// Quaternionf product, lanes of Eigen/src/Geometry/arch/Geometry_SSE.h
Qf Mul(const Qf& a, const Qf& b) {
  Qf r;
  r.x = (a.x * b.w - a.z * b.y) + (a.y * b.z + a.w * b.x);
  r.y = (a.y * b.w - a.x * b.z) + (a.z * b.x + a.w * b.y);
  r.z = (a.z * b.w - a.y * b.x) + (a.x * b.y + a.w * b.z);
  r.w = (a.w * b.w - a.x * b.x) - (a.z * b.z + a.y * b.y);
  return r;
}
Qf Normalized(const Qf& q) {  // 4-lane reduction (x2 + z2) + (y2 + w2)
  const float n2 = (q.x * q.x + q.z * q.z) + (q.y * q.y + q.w * q.w);
  if (!(n2 > 0.f)) return q;
  const float n = std::sqrt(n2);
  return Qf{q.w / n, q.x / n, q.y / n, q.z / n};
}
// Quaterniond product, the two Packet2d halves of Geometry_SSE.h
Qd Mul(const Qd& a, const Qd& b) {
  const double t1x = a.w * b.x + a.y * b.z, t1y = a.w * b.y + a.y * b.w;
  const double t2x = a.z * b.x - a.x * b.z, t2y = a.z * b.y - a.x * b.w;
  const double u1z = a.w * b.z - a.y * b.x, u1w = a.w * b.w - a.y * b.y;
  const double u2z = a.z * b.z + a.x * b.x, u2w = a.z * b.w + a.x * b.y;
  return Qd{u1w - u2z, t1x - t2y, t1y + t2x, u1z + u2w};
}
Qd Normalized(const Qd& q) {
  const double n2 = (q.x * q.x + q.z * q.z) + (q.y * q.y + q.w * q.w);
  if (!(n2 > 0.0)) return q;
  const double n = std::sqrt(n2);
  return Qd{q.w / n, q.x / n, q.y / n, q.z / n};
}

struct PixelData {  // submap_3d.cc:31-37
  int min_z = INT_MAX;
  int max_z = INT_MIN;
  int count = 0;
  float probability_sum = 0.f;
  float max_probability = 0.5f;
};

struct Voxel {
  int x, y, z;
  uint32_t value;
};

// ExtractVoxelData (submap_3d.cc:82-111) / the loop of ProjectToCvMat (:401-420)
std::vector<Voxel> Extract(const std::vector<Cell>& cells, float resolution, const Qf& q, const float t[3],
                           float resolution_inverse, int min_index[2], int max_index[2]) {
  std::vector<Voxel> out;
  min_index[0] = min_index[1] = INT_MAX;
  max_index[0] = max_index[1] = INT_MIN;
  for (const Cell& c : cells) {
    if (ValueToProbability(c.value) < 0.501f) continue;  // kXrayObstructedCellProbabilityLimit
    const float center[3] = {static_cast<float>(c.x) * resolution, static_cast<float>(c.y) * resolution,
                             static_cast<float>(c.z) * resolution};  // GetCenterOfCell
    float g[3];
    Rotate(q, center, g);
    for (int i = 0; i < 3; ++i) g[i] = g[i] + t[i];
    const Voxel v{RoundToInt(g[0] * resolution_inverse), RoundToInt(g[1] * resolution_inverse),
                  RoundToInt(g[2] * resolution_inverse), c.value};
    out.push_back(v);
    min_index[0] = std::min(min_index[0], v.x);
    min_index[1] = std::min(min_index[1], v.y);
    max_index[0] = std::max(max_index[0], v.x);
    max_index[1] = std::max(max_index[1], v.y);
  }
  return out;
}

void Accumulate(PixelData& pixel, const Voxel& v) {
  ++pixel.count;
  pixel.min_z = std::min(pixel.min_z, v.z);
  pixel.max_z = std::max(pixel.max_z, v.z);
  const float probability = ValueToProbability(v.value);
  pixel.probability_sum += probability;
  pixel.max_probability = std::max(pixel.max_probability, probability);
}

int Texture(const std::vector<Cell>& cells, float resolution, const double pose[7], FILE* out) {
  const Qf q{static_cast<float>(pose[3]), static_cast<float>(pose[4]), static_cast<float>(pose[5]), static_cast<float>(pose[6])};
  const float t[3] = {static_cast<float>(pose[0]), static_cast<float>(pose[1]), static_cast<float>(pose[2])};
  int min_index[2], max_index[2];
  const std::vector<Voxel> voxels = Extract(cells, resolution, q, t, 1.f / resolution, min_index, max_index);
  int width = 0, height = 0;
  std::string cell_data;
  if (voxels.empty()) {
    max_index[0] = max_index[1] = 0;  // the library's documented 0 x 0 (the reference overflows here)
  } else {
    width = max_index[1] - min_index[1] + 1;
    height = max_index[0] - min_index[0] + 1;
    std::vector<PixelData> pixels(static_cast<size_t>(width) * height);  // AccumulatePixelData (:53-78)
    for (const Voxel& v : voxels) Accumulate(pixels[(max_index[0] - v.x) * width + (max_index[1] - v.y)], v);
    for (const PixelData& pixel : pixels) {  // ComputePixelValues (:116-145)
      const float z_difference = pixel.count > 0 ? pixel.max_z - pixel.min_z : 0;
      if (z_difference < 3.f) {  // kMinZDifference
        cell_data.push_back(0);
        cell_data.push_back(0);
        continue;
      }
      const float free_space = std::max(z_difference - pixel.count, 0.f);
      const float free_space_weight = 0.15f * free_space;  // kFreeSpaceWeight
      const float total_weight = pixel.count + free_space_weight;
      const float free_space_probability = 1.f - pixel.max_probability;
      const float average_probability =
          ClampProbability((pixel.probability_sum + free_space_probability * free_space_weight) / total_weight);
      const int delta = 128 - ProbabilityToLogOddsInteger(average_probability);
      const uint8_t alpha = delta > 0 ? 0 : -delta;
      const uint8_t value = delta > 0 ? delta : 0;
      cell_data.push_back(static_cast<char>(value));
      cell_data.push_back(static_cast<char>((value || alpha) ? alpha : 1));
    }
  }
  // slice pose (:172-176): global_submap_pose.inverse() * Rigid3d::Translation(max_x * res, max_y * res, t.z)
  const Qd gq{pose[3], pose[4], pose[5], pose[6]};
  const Qd iq{gq.w, -gq.x, -gq.y, -gq.z};  // Rigid3::inverse (rigid_transform.h:167-171)
  double it[3];
  Rotate(iq, pose, it);
  for (double& e : it) e = -e;
  const double st[3] = {static_cast<double>(max_index[0] * resolution), static_cast<double>(max_index[1] * resolution), pose[2]};
  double rt[3];
  Rotate(iq, st, rt);  // operator* (rigid_transform.h:206-212)
  const Qd sq = Normalized(Mul(iq, Qd{1.0, 0.0, 0.0, 0.0}));
  const double slice[7] = {rt[0] + it[0], rt[1] + it[1], rt[2] + it[2], sq.w, sq.x, sq.y, sq.z};
  const double res = resolution;
  std::fwrite(&width, 4, 1, out);
  std::fwrite(&height, 4, 1, out);
  std::fwrite(&res, 8, 1, out);
  std::fwrite(slice, 8, 7, out);
  std::fwrite(cell_data.data(), 1, cell_data.size(), out);
  return 0;
}

int Image(const std::vector<Cell>& cells, float grid_resolution, const double pose[7], FILE* out) {
  const double resolution = grid_resolution;  // double& resolution (:384)
  // transform::Rigid3d::Rotation(transform.rotation()).cast<float>()
  const Qf rotation{static_cast<float>(pose[3]), static_cast<float>(pose[4]), static_cast<float>(pose[5]),
                    static_cast<float>(pose[6])};
  // GetYaw (transform.h:43-52): rotation * UnitX, atan2(y, x)
  const double unit_x[3] = {1.0, 0.0, 0.0};
  double direction[3];
  Rotate(Qd{pose[3], pose[4], pose[5], pose[6]}, unit_x, direction);
  const double yaw = std::atan2(direction[1], direction[0]);
  // Embed3D(Rigid2d::Rotation(-yaw)) (transform.h:110-115): Quaterniond(AngleAxisd(-yaw, UnitZ)), then cast<float>
  const double ha = 0.5 * -yaw;
  const double s = std::sin(ha);
  const Qf inv_yaw{static_cast<float>(std::cos(ha)), static_cast<float>(s * 0.0), static_cast<float>(s * 0.0),
                   static_cast<float>(s * 1.0)};
  // inv_yaw_rot * gravity_aligned (rigid_transform.h:206-212): translation inv_yaw * 0 + 0, rotation normalized product
  const float zero[3] = {0.f, 0.f, 0.f};
  float t[3];
  Rotate(inv_yaw, zero, t);
  for (float& e : t) e = e + 0.f;
  const Qf q = Normalized(Mul(inv_yaw, rotation));
  const float resolution_inverse = 1.f / resolution;  // double division, stored to float
  int min_index[2], max_index[2];
  const std::vector<Voxel> voxels = Extract(cells, grid_resolution, q, t, resolution_inverse, min_index, max_index);
  int width = 0, height = 0;
  std::vector<uint8_t> image;
  if (voxels.empty()) {
    min_index[0] = min_index[1] = 0;
  } else {
    width = max_index[0] - min_index[0] + 1;
    height = max_index[1] - min_index[1] + 1;
    std::vector<PixelData> pixels(static_cast<size_t>(width) * height);
    for (const Voxel& v : voxels) Accumulate(pixels[(v.y - min_index[1]) * width + (v.x - min_index[0])], v);
    for (const PixelData& pixel : pixels) {  // (:455-461): int stored into a uchar, modulo 256
      const int cell_value =
          RoundToInt((pixel.probability_sum - kMinProbability) * (255.f / (kMaxProbability - kMinProbability)));
      image.push_back(static_cast<uint8_t>(cell_value));
    }
  }
  const double ox = min_index[0] * resolution, oy = min_index[1] * resolution;
  std::fwrite(&width, 4, 1, out);
  std::fwrite(&height, 4, 1, out);
  std::fwrite(&resolution, 8, 1, out);
  std::fwrite(&ox, 8, 1, out);
  std::fwrite(&oy, 8, 1, out);
  std::fwrite(image.data(), 1, image.size(), out);
  return 0;
}

#endif  // XRAY_MODEL_EXHAUSTIVE

}  // namespace

#ifdef XRAY_MODEL_EXHAUSTIVE
extern "C" uint8_t dliom_probability_to_log_odds_integer(float probability);

int main() {
  uint32_t lo, hi;
  const float a = kMinProbability, b = kMaxProbability;
  std::memcpy(&lo, &a, 4);
  std::memcpy(&hi, &b, 4);
  int64_t checked = 0, mismatches = 0, out_of_range = 0, non_monotone = 0;
  int previous = 0;
  for (uint32_t bits = lo; bits <= hi; ++bits) {
    float p;
    std::memcpy(&p, &bits, 4);
    const int want = ProbabilityToLogOddsInteger(p);
    const int got = dliom_probability_to_log_odds_integer(p);
    if (want < 1 || want > 255) ++out_of_range;
    if (want < previous) ++non_monotone;
    if (got != want && mismatches++ < 5) std::printf("mismatch at %.9g: library %d, formula %d\n", p, got, want);
    previous = want;
    ++checked;
  }
  std::printf("checked %lld floats: %lld mismatches, %lld out of 1..255, %lld decreasing steps, first %d last %d\n",
              static_cast<long long>(checked), static_cast<long long>(mismatches), static_cast<long long>(out_of_range),
              static_cast<long long>(non_monotone), ProbabilityToLogOddsInteger(a), ProbabilityToLogOddsInteger(b));
  return mismatches == 0 && out_of_range == 0 && non_monotone == 0 ? 0 : 1;
}
#else
int main(int argc, char** argv) {
  if (argc != 11) {
    std::fprintf(stderr, "usage: %s texture|image grid.pb tx ty tz qw qx qy qz out.bin\n", argv[0]);
    return 2;
  }
  FILE* in = std::fopen(argv[2], "rb");
  if (in == nullptr) return 2;
  std::vector<uint8_t> buf;
  uint8_t chunk[65536];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof chunk, in)) > 0) buf.insert(buf.end(), chunk, chunk + got);
  std::fclose(in);
  float resolution;
  std::vector<Cell> cells;
  if (!parse_grid(buf, &resolution, &cells)) {
    std::fprintf(stderr, "malformed grid\n");
    return 2;
  }
  double pose[7];
  for (int i = 0; i < 7; ++i) pose[i] = std::strtod(argv[3 + i], nullptr);
  FILE* out = std::fopen(argv[10], "wb");
  if (out == nullptr) return 2;
  const int s = std::strcmp(argv[1], "texture") == 0 ? Texture(cells, resolution, pose, out) : Image(cells, resolution, pose, out);
  std::fclose(out);
  return s;
}
#endif
