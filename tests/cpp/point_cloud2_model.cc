// One-thread C++ restatement of dliom.h "PointCloud2 messages decoded on the device": what a caller of the library writes
// today in front of dliom_add_range_data -- SensorBridge::HandlePointCloud2Message's four branches with HandleRangefinder's
// frame change (cartographer_ros/sensor_bridge.cc:176-240, 286-299) and the export's two conversions
// (msg_conversion.cc:185-226) -- in this project's own words, every field fetched with memcpy.  Independent of
// csrc/point_cloud2_layout.h.  Build with -ffp-contract=off.
//
// As a program:  point_cloud2_model <cases.bin> <results.bin>      (tests/point_cloud2_common.py writes and reads the files)
// As a library (-shared -fPIC -DPOINT_CLOUD2_MODEL_NO_MAIN):  point_cloud2_model(), for tools/point_cloud2_bench.py
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dliom.h"

namespace {

const int kSize[9] = {0, 1, 1, 2, 2, 4, 4, 4, 8};

const dliom_point_field* find(const dliom_point_cloud2& m, const char* name) {
  for (int k = 0; k < m.num_fields; ++k)
    if (std::strcmp(m.fields[k].name, name) == 0) return &m.fields[k];
  return nullptr;
}

bool need(const dliom_point_cloud2& m, const char* name, uint32_t datatype, uint32_t* offset) {
  const dliom_point_field* f = find(m, name);
  if (f == nullptr || f->datatype != datatype || f->count != 1) return false;
  *offset = f->offset;
  return true;
}

template <class T>
T get(const uint8_t* record, uint32_t offset) {
  T v;
  std::memcpy(&v, record + offset, sizeof v);
  return v;
}

// Eigen's QuaternionBase::_transformVector, then the translation, in float
void transform(const float q[4], const float t[3], float* x, float* y, float* z) {
  const float w = q[0], ux = q[1], uy = q[2], uz = q[3], vx = *x, vy = *y, vz = *z;
  float ax = uy * vz - uz * vy, ay = uz * vx - ux * vz, az = ux * vy - uy * vx;
  ax = ax + ax;
  ay = ay + ay;
  az = az + az;
  const float cx = uy * az - uz * ay, cy = uz * ax - ux * az, cz = ux * ay - uy * ax;
  *x = ((vx + w * ax) + cx) + t[0];
  *y = ((vy + w * ay) + cy) + t[1];
  *z = ((vz + w * az) + cz) + t[2];
}

}  // namespace

// xyzt: room for 4 n floats, intensities: n (either may be NULL: not wanted).  Returns DLIOM_OK or DLIOM_ERR_INVALID_ARGUMENT.
extern "C" int point_cloud2_model(const dliom_point_cloud2* message, int mode, const double* sensor_to_tracking, float* xyzt,
                                  float* intensities, int64_t* kept, int* has_intensities, int64_t* time, float origin[3]) {
  const dliom_point_cloud2& m = *message;
  if (mode < 0 || mode > 5 || m.is_bigendian != 0) return DLIOM_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < m.num_fields; ++k) {
    const dliom_point_field& f = m.fields[k];
    if (f.datatype < 1 || f.datatype > 8) return DLIOM_ERR_INVALID_ARGUMENT;
    if (static_cast<uint64_t>(f.offset) + static_cast<uint64_t>(kSize[f.datatype]) * f.count > m.point_step)
      return DLIOM_ERR_INVALID_ARGUMENT;
  }
  const uint64_t n = static_cast<uint64_t>(m.height) * m.width;
  if (static_cast<uint64_t>(m.width) * m.point_step > m.row_step) return DLIOM_ERR_INVALID_ARGUMENT;
  if (static_cast<uint64_t>(m.height) * m.row_step > m.data_size) return DLIOM_ERR_INVALID_ARGUMENT;
  if (n >= (uint64_t{1} << 27)) return DLIOM_ERR_INVALID_ARGUMENT;
  uint32_t ox, oy, oz, ot = 0, oi = 0;
  if (!need(m, "x", 7, &ox) || !need(m, "y", 7, &oy) || !need(m, "z", 7, &oz)) return DLIOM_ERR_INVALID_ARGUMENT;
  const bool slam = mode <= 3;
  int intensity = 0;  // 1 float field, 2 byte field, 3 the constant
  if (mode == 0 && !need(m, "t", 6, &ot)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (mode == 1 && !need(m, "time", 7, &ot)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (mode == 2 && !need(m, "timestamp", 8, &ot)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (mode == 4) {
    intensity = 3;
    if (find(m, "intensity") != nullptr) {
      if (!need(m, "intensity", 7, &oi)) return DLIOM_ERR_INVALID_ARGUMENT;
      intensity = 1;
    }
  }
  if (mode == 5) {
    if (!need(m, "intensity", 2, &oi)) return DLIOM_ERR_INVALID_ARGUMENT;
    intensity = 2;
  }
  if (mode <= 2 && n == 0) return DLIOM_ERR_INVALID_ARGUMENT;
  auto record = [&m](uint64_t i) { return m.data + (i / m.width) * m.row_step + (i % m.width) * m.point_step; };
  int64_t stamp = (static_cast<int64_t>(m.stamp_sec) + 719162LL * 86400LL) * 10000000LL + (static_cast<int64_t>(m.stamp_nsec) + 50) / 100;
  double rel_time_last = 0.;
  if (mode <= 2) {
    const uint8_t* last = record(n - 1);
    if (mode == 0) {
      const float seconds = static_cast<float>(get<uint32_t>(last, ot)) * 1e-9f;
      rel_time_last = seconds;
    } else if (mode == 1) {
      rel_time_last = get<float>(last, ot);
    } else {
      rel_time_last = get<double>(last, ot);
    }
    const double ticks = rel_time_last * 1e7;
    if (!std::isfinite(rel_time_last) || !(std::fabs(ticks) < 9223372036854775808.0)) return DLIOM_ERR_INVALID_ARGUMENT;
    if (mode != 2) stamp += static_cast<int64_t>(ticks);
  }
  float q[4] = {1.f, 0.f, 0.f, 0.f}, t3[3] = {0.f, 0.f, 0.f};
  if (sensor_to_tracking != nullptr) {
    for (int k = 0; k < 3; ++k) t3[k] = static_cast<float>(sensor_to_tracking[k]);
    for (int k = 0; k < 4; ++k) q[k] = static_cast<float>(sensor_to_tracking[3 + k]);
  }
  int64_t count = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t* r = record(i);
    float x = get<float>(r, ox), y = get<float>(r, oy), z = get<float>(r, oz);
    if (slam && !(std::isfinite(x) && std::isfinite(y) && std::isfinite(z))) continue;
    float t = 0.f;
    if (mode == 0) {
      const float seconds = static_cast<float>(get<uint32_t>(r, ot)) * 1e-9f;
      t = static_cast<float>(static_cast<double>(seconds) - rel_time_last);
    } else if (mode == 1) {
      t = static_cast<float>(static_cast<double>(get<float>(r, ot)) - rel_time_last);
    } else if (mode == 2) {
      t = static_cast<float>(get<double>(r, ot) - rel_time_last);
    }
    if (!(std::fabs(static_cast<double>(t) * 1e7) < 9223372036854775808.0)) return DLIOM_ERR_INVALID_ARGUMENT;
    if (sensor_to_tracking != nullptr) transform(q, t3, &x, &y, &z);
    if (xyzt != nullptr) {
      float* o = xyzt + 4 * count;
      o[0] = x;
      o[1] = y;
      o[2] = z;
      o[3] = t;
    }
    if (intensities != nullptr && intensity != 0)
      intensities[count] = intensity == 1 ? get<float>(r, oi) : intensity == 2 ? static_cast<float>(get<uint8_t>(r, oi)) : 1.0f;
    ++count;
  }
  *kept = count;
  *has_intensities = intensity != 0 ? 1 : 0;
  *time = stamp;
  for (int k = 0; k < 3; ++k) origin[k] = t3[k];
  return DLIOM_OK;
}

#ifndef POINT_CLOUD2_MODEL_NO_MAIN
namespace {
template <class T>
bool rd(std::FILE* f, T* v, size_t count = 1) {
  return std::fread(v, sizeof(T), count, f) == count;
}
template <class T>
void wr(std::FILE* f, const T* v, size_t count = 1) {
  std::fwrite(v, sizeof(T), count, f);
}
}  // namespace

// cases.bin: int32 cases, then a case: int32 mode, int32 has_transform, double[7], uint32 height width point_step row_step
// is_bigendian stamp_sec stamp_nsec, int32 num_fields, a field: char[32] name, uint32 offset datatype count; uint64 data_size,
// uint64 lead (bytes the data is shifted by inside its buffer), the bytes.
// results.bin, a case: int32 status, int64 time, float[3] origin, int64 kept, int32 has_intensities, xyzt, intensities.
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (in == nullptr || out == nullptr) return 2;
  int32_t cases = 0;
  if (!rd(in, &cases)) return 2;
  for (int32_t c = 0; c < cases; ++c) {
    int32_t mode, has_transform, num_fields;
    double tf[7];
    uint32_t head[7];
    if (!rd(in, &mode) || !rd(in, &has_transform) || !rd(in, tf, 7) || !rd(in, head, 7) || !rd(in, &num_fields)) return 2;
    std::vector<std::string> names(num_fields);
    std::vector<dliom_point_field> fields(num_fields);
    for (int32_t k = 0; k < num_fields; ++k) {
      char name[33] = {0};
      uint32_t v[3];
      if (!rd(in, name, 32) || !rd(in, v, 3)) return 2;
      names[k] = name;
      fields[k].offset = v[0];
      fields[k].datatype = v[1];
      fields[k].count = v[2];
    }
    for (int32_t k = 0; k < num_fields; ++k) fields[k].name = names[k].c_str();
    uint64_t data_size, lead;
    if (!rd(in, &data_size) || !rd(in, &lead)) return 2;
    std::vector<uint8_t> buffer(data_size + lead + 1);
    if (data_size > 0 && !rd(in, buffer.data() + lead, data_size)) return 2;
    dliom_point_cloud2 m{};
    m.height = head[0];
    m.width = head[1];
    m.point_step = head[2];
    m.row_step = head[3];
    m.is_bigendian = head[4];
    m.stamp_sec = head[5];
    m.stamp_nsec = head[6];
    m.num_fields = num_fields;
    m.fields = fields.data();
    m.data = buffer.data() + lead;
    m.data_size = data_size;
    const uint64_t n = static_cast<uint64_t>(m.height) * m.width;
    std::vector<float> xyzt(4 * n + 4), intensities(n + 1);
    int64_t kept = 0, time = 0;
    int has = 0;
    float origin[3] = {0.f, 0.f, 0.f};
    const int32_t status = n < (uint64_t{1} << 27)
                               ? point_cloud2_model(&m, mode, has_transform ? tf : nullptr, xyzt.data(), intensities.data(), &kept, &has, &time, origin)
                               : DLIOM_ERR_INVALID_ARGUMENT;
    if (status != DLIOM_OK) {
      kept = 0;
      has = 0;
      time = 0;
    }
    const int32_t has32 = has;
    wr(out, &status);
    wr(out, &time);
    wr(out, origin, 3);
    wr(out, &kept);
    wr(out, &has32);
    wr(out, xyzt.data(), 4 * static_cast<size_t>(kept));
    if (has) wr(out, intensities.data(), static_cast<size_t>(kept));
  }
  std::fclose(out);
  std::printf("POINT CLOUD2 MODEL DONE %d\n", cases);
  return 0;
}
#endif
