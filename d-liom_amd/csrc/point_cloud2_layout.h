// The host half of the PointCloud2 decode (dliom.h "PointCloud2 messages decoded on the device"): the message's field
// table turned into a small plan of offsets and types for a mode, the refusals, rel_time_last from the last record's
// bytes and the stamp.  No HIP in here: point_cloud2.hip includes it, and tests/cpp/point_cloud2_layout_check.cc runs it
// under the sanitizers on hostile tables.
#ifndef DLIOM_CSRC_POINT_CLOUD2_LAYOUT_H_
#define DLIOM_CSRC_POINT_CLOUD2_LAYOUT_H_

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/dliom.h"

namespace dliom {

enum : int { kPc2TimeNone = 0, kPc2TimeUint32Ns = 1, kPc2TimeFloat32 = 2, kPc2TimeFloat64 = 3 };
enum : int { kPc2IntensityNone = 0, kPc2IntensityFloat32 = 1, kPc2IntensityUint8 = 2, kPc2IntensityOne = 3 };

// What the kernel needs of a message in a mode; passed to it by value.
struct PointCloud2Plan {
  uint32_t n;  // height * width, < 2^27
  uint32_t width, point_step, row_step;
  uint32_t off_x, off_y, off_z, off_time, off_intensity;  // inside a record
  int time_kind, intensity_kind;
  int drop_non_finite;   // the SLAM modes
  double rel_time_last;  // what is subtracted from a point's time (0 in the untimed modes)
  uint64_t used_bytes;   // of `data`, up to the last record's end
};

constexpr uint32_t kPc2MaxPoints = uint32_t{1} << 27;  // add_range_data_stage_a's limit

inline uint32_t point_field_size(uint32_t datatype) {
  switch (datatype) {
    case DLIOM_POINT_FIELD_INT8:
    case DLIOM_POINT_FIELD_UINT8:
      return 1;
    case DLIOM_POINT_FIELD_INT16:
    case DLIOM_POINT_FIELD_UINT16:
      return 2;
    case DLIOM_POINT_FIELD_INT32:
    case DLIOM_POINT_FIELD_UINT32:
    case DLIOM_POINT_FIELD_FLOAT32:
      return 4;
    case DLIOM_POINT_FIELD_FLOAT64:
      return 8;
    default:
      return 0;
  }
}

// the first field of that name, as pcl::fromROSMsg's mapping finds it; null: none
inline const dliom_point_field* find_point_field(const dliom_point_cloud2& m, const char* name) {
  for (int32_t k = 0; k < m.num_fields; ++k)
    if (std::strcmp(m.fields[k].name, name) == 0) return &m.fields[k];
  return nullptr;
}

// a field the mode cannot do without: there, of that datatype, one value
inline bool required_point_field(const dliom_point_cloud2& m, const char* name, uint32_t datatype, uint32_t* offset) {
  const dliom_point_field* f = find_point_field(m, name);
  if (f == nullptr || f->datatype != datatype || f->count != 1) return false;
  *offset = f->offset;
  return true;
}

// common::FromSeconds: the duration_cast truncates; undefined (refused) unless the ticks fit
inline bool seconds_to_ticks(double seconds, int64_t* ticks) {
  const double x = seconds * 1e7;
  if (!(std::fabs(x) < 9223372036854775808.0)) return false;
  *ticks = static_cast<int64_t>(x);
  return true;
}

// FromRos(stamp): 100 ns ticks since 0001-01-01, the nanoseconds rounded half up
inline int64_t point_cloud2_stamp(uint32_t sec, uint32_t nsec) {
  return (static_cast<int64_t>(sec) + INT64_C(719162) * 86400) * INT64_C(10000000) + (static_cast<int64_t>(nsec) + 50) / 100;
}

// DLIOM_OK with *plan and *time filled, or DLIOM_ERR_INVALID_ARGUMENT (the list of dliom.h).  Reads no byte of `data`
// but the time field of the last record, and that only once the record is known to lie inside.
inline int point_cloud2_plan(const dliom_point_cloud2* message, int mode, PointCloud2Plan* plan, int64_t* time) {
  if (message == nullptr || plan == nullptr || time == nullptr || mode < DLIOM_POINT_CLOUD2_SLAM_OUSTER ||
      mode > DLIOM_POINT_CLOUD2_EXPORT_RSLIDAR)
    return DLIOM_ERR_INVALID_ARGUMENT;
  const dliom_point_cloud2& m = *message;
  if (m.is_bigendian != 0 || m.num_fields < 0 || (m.num_fields > 0 && m.fields == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  for (int32_t k = 0; k < m.num_fields; ++k) {
    const dliom_point_field& f = m.fields[k];
    const uint64_t size = point_field_size(f.datatype);
    if (f.name == nullptr || size == 0 || f.offset + size * f.count > m.point_step) return DLIOM_ERR_INVALID_ARGUMENT;
  }
  const uint64_t n = static_cast<uint64_t>(m.height) * m.width;
  if (static_cast<uint64_t>(m.width) * m.point_step > m.row_step || static_cast<uint64_t>(m.height) * m.row_step > m.data_size ||
      n >= kPc2MaxPoints || (n > 0 && m.data == nullptr))
    return DLIOM_ERR_INVALID_ARGUMENT;
  PointCloud2Plan p{};
  p.n = static_cast<uint32_t>(n);
  p.width = m.width;
  p.point_step = m.point_step;
  p.row_step = m.row_step;
  if (!required_point_field(m, "x", DLIOM_POINT_FIELD_FLOAT32, &p.off_x) ||
      !required_point_field(m, "y", DLIOM_POINT_FIELD_FLOAT32, &p.off_y) ||
      !required_point_field(m, "z", DLIOM_POINT_FIELD_FLOAT32, &p.off_z))
    return DLIOM_ERR_INVALID_ARGUMENT;
  p.drop_non_finite = mode <= DLIOM_POINT_CLOUD2_SLAM_OTHER ? 1 : 0;
  bool have_time = true;
  switch (mode) {
    case DLIOM_POINT_CLOUD2_SLAM_OUSTER:
      p.time_kind = kPc2TimeUint32Ns;
      have_time = required_point_field(m, "t", DLIOM_POINT_FIELD_UINT32, &p.off_time);
      break;
    case DLIOM_POINT_CLOUD2_SLAM_VELODYNE:
      p.time_kind = kPc2TimeFloat32;
      have_time = required_point_field(m, "time", DLIOM_POINT_FIELD_FLOAT32, &p.off_time);
      break;
    case DLIOM_POINT_CLOUD2_SLAM_ROBOSENSE:
      p.time_kind = kPc2TimeFloat64;
      have_time = required_point_field(m, "timestamp", DLIOM_POINT_FIELD_FLOAT64, &p.off_time);
      break;
    case DLIOM_POINT_CLOUD2_EXPORT: {
      const dliom_point_field* f = find_point_field(m, "intensity");
      p.intensity_kind = kPc2IntensityOne;
      if (f != nullptr) {
        if (f->datatype != DLIOM_POINT_FIELD_FLOAT32 || f->count != 1) return DLIOM_ERR_INVALID_ARGUMENT;
        p.intensity_kind = kPc2IntensityFloat32;
        p.off_intensity = f->offset;
      }
      break;
    }
    case DLIOM_POINT_CLOUD2_EXPORT_RSLIDAR:
      p.intensity_kind = kPc2IntensityUint8;
      if (!required_point_field(m, "intensity", DLIOM_POINT_FIELD_UINT8, &p.off_intensity)) return DLIOM_ERR_INVALID_ARGUMENT;
      break;
    default:
      break;
  }
  if (!have_time) return DLIOM_ERR_INVALID_ARGUMENT;
  if (n > 0) p.used_bytes = static_cast<uint64_t>(m.height - 1) * m.row_step + static_cast<uint64_t>(m.width) * m.point_step;
  int64_t stamp = point_cloud2_stamp(m.stamp_sec, m.stamp_nsec);
  if (p.time_kind != kPc2TimeNone) {
    if (n == 0) return DLIOM_ERR_INVALID_ARGUMENT;  // points.back() of an empty vector
    const uint8_t* last = m.data + static_cast<uint64_t>((n - 1) / m.width) * m.row_step +
                          static_cast<uint64_t>((n - 1) % m.width) * m.point_step + p.off_time;
    if (p.time_kind == kPc2TimeUint32Ns) {
      uint32_t t;
      std::memcpy(&t, last, 4);
      const float seconds = static_cast<float>(t) * 1e-9f;  // (round to nearest; a float product)
      p.rel_time_last = static_cast<double>(seconds);
    } else if (p.time_kind == kPc2TimeFloat32) {
      float t;
      std::memcpy(&t, last, 4);
      p.rel_time_last = static_cast<double>(t);
    } else {
      std::memcpy(&p.rel_time_last, last, 8);
    }
    int64_t ticks;
    if (!std::isfinite(p.rel_time_last) || !seconds_to_ticks(p.rel_time_last, &ticks)) return DLIOM_ERR_INVALID_ARGUMENT;
    // Robosense's stamp is the last point's already (:223-225)
    if (p.time_kind != kPc2TimeFloat64) stamp = static_cast<int64_t>(static_cast<uint64_t>(stamp) + static_cast<uint64_t>(ticks));
  }
  *plan = p;
  *time = stamp;
  return DLIOM_OK;
}

}  // namespace dliom

#endif  // DLIOM_CSRC_POINT_CLOUD2_LAYOUT_H_
