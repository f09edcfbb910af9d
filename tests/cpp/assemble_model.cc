// CPU model of the head of the point-cloud export, restated from the reference's text on a std::vector:
//   transform/transform_interpolation_buffer.{h,cc}   Push, Has, Lookup (std::lower_bound)
//   transform/timestamped_transform.cc:22-37          Interpolate: blended translation, Eigen's Quaterniond::slerp
//   transform/rigid_transform.h                       Rigid3d operator*, cast<float>, Rigid3f * Vector3f
//   cartographer_ros/assets_writer.cc:119-160         HandleMessage's loop over the points of a message
// glibc's sin / acos, -ffp-contract=off, Eigen 3.3's SSE2 evaluation orders (two Packet2d halves for the quaternion
// product, the dot product and the squared norm).  Independent of d-liom_amd/csrc: nothing is shared with the library.
//
// usage: assemble_model ops.bin out.bin [--time]
// ops.bin:  int64 nodes | int64 time[nodes] | double pose7[nodes] (tx ty tz qw qx qy qz), then operations until the end:
//   int32 1 (lookup):   int64 count | int64 time[count]
//   int32 2 (assemble): int64 cloud_time | double sensor_to_tracking[7] | int64 n | float xyzt[4 n]
// out.bin:  int32 status of the pushes (0, -1: a time older than the latest), then per operation
//   lookup:   per time  int32 has | double pose7[7]
//   assemble: int32 status (0, -1: a time FromSeconds leaves undefined) | int64 kept | int32 index[kept] | float xyz[3 kept] |
//             float origin[3] | int64 kept points that took slerp's sin / acos branch | int64 distinct intervals used
// --time: every assemble operation runs five times on this thread; "op <k> <best milliseconds>" per operation on stdout.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Quaterniond {
  double w, x, y, z;
};
struct Rigid3d {
  double t[3];
  Quaterniond q;
};
struct Rigid3f {
  float t[3];
  float w, x, y, z;
};
struct TimestampedTransform {
  int64_t time;
  Rigid3d transform;
};

Quaterniond Product(const Quaterniond& a, const Quaterniond& b) {  // Geometry_SSE.h, double
  const double t1x = a.w * b.x + a.y * b.z, t1y = a.w * b.y + a.y * b.w;
  const double t2x = a.z * b.x - a.x * b.z, t2y = a.z * b.y - a.x * b.w;
  const double u1z = a.w * b.z - a.y * b.x, u1w = a.w * b.w - a.y * b.y;
  const double u2z = a.z * b.z + a.x * b.x, u2w = a.z * b.w + a.x * b.y;
  return Quaterniond{u1w - u2z, t1x - t2y, t1y + t2x, u1z + u2w};
}

Quaterniond Normalized(const Quaterniond& q) {
  const double z2 = (q.x * q.x + q.z * q.z) + (q.y * q.y + q.w * q.w);
  if (z2 > 0.0) {
    const double n = std::sqrt(z2);
    return Quaterniond{q.w / n, q.x / n, q.y / n, q.z / n};
  }
  return q;
}

void Rotate(const Quaterniond& q, const double v[3], double out[3]) {  // QuaternionBase::_transformVector
  double uv[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
  for (double& c : uv) c += c;
  const double c[3] = {q.y * uv[2] - q.z * uv[1], q.z * uv[0] - q.x * uv[2], q.x * uv[1] - q.y * uv[0]};
  for (int i = 0; i < 3; ++i) out[i] = (v[i] + q.w * uv[i]) + c[i];
}

void RotateF(const Rigid3f& r, const float v[3], float out[3]) {
  float uv[3] = {r.y * v[2] - r.z * v[1], r.z * v[0] - r.x * v[2], r.x * v[1] - r.y * v[0]};
  for (float& c : uv) c += c;
  const float c[3] = {r.y * uv[2] - r.z * uv[1], r.z * uv[0] - r.x * uv[2], r.x * uv[1] - r.y * uv[0]};
  for (int i = 0; i < 3; ++i) out[i] = (v[i] + r.w * uv[i]) + c[i];
}

bool g_libm_branch = false;  // the last Slerp took its sin / acos branch

Quaterniond Slerp(const Quaterniond& a, double t, const Quaterniond& b) {  // Eigen/src/Geometry/Quaternion.h
  const double one = 1.0 - 2.220446049250313e-16;
  const double d = (a.x * b.x + a.z * b.z) + (a.y * b.y + a.w * b.w);
  const double absD = std::abs(d);
  double scale0, scale1;
  if (absD >= one) {
    scale0 = 1.0 - t;
    scale1 = t;
    g_libm_branch = false;
  } else {
    const double theta = std::acos(absD);
    const double sinTheta = std::sin(theta);
    scale0 = std::sin((1.0 - t) * theta) / sinTheta;
    scale1 = std::sin(t * theta) / sinTheta;
    g_libm_branch = true;
  }
  if (d < 0.0) scale1 = -scale1;
  return Quaterniond{scale0 * a.w + scale1 * b.w, scale0 * a.x + scale1 * b.x, scale0 * a.y + scale1 * b.y, scale0 * a.z + scale1 * b.z};
}

double ToSeconds(int64_t ticks) { return static_cast<double>(ticks) / 1e7; }  // duration_cast<duration<double>>

Rigid3d Interpolate(const TimestampedTransform& start, const TimestampedTransform& end, int64_t time) {
  const double duration = ToSeconds(end.time - start.time);
  const double factor = ToSeconds(time - start.time) / duration;
  Rigid3d r;
  for (int i = 0; i < 3; ++i) r.t[i] = start.transform.t[i] + (end.transform.t[i] - start.transform.t[i]) * factor;
  r.q = Slerp(start.transform.q, factor, end.transform.q);
  return r;
}

Rigid3d Compose(const Rigid3d& lhs, const Rigid3d& rhs) {  // rigid_transform.h operator*
  Rigid3d r;
  double rt[3];
  Rotate(lhs.q, rhs.t, rt);
  for (int i = 0; i < 3; ++i) r.t[i] = rt[i] + lhs.t[i];
  r.q = Normalized(Product(lhs.q, rhs.q));
  return r;
}

class TransformInterpolationBuffer {
 public:
  bool Push(int64_t time, const Rigid3d& transform) {
    if (!nodes_.empty() && !(time >= nodes_.back().time)) return false;  // CHECK_GE(time, latest_time())
    nodes_.push_back(TimestampedTransform{time, transform});
    return true;
  }
  bool Has(int64_t time) const {
    if (nodes_.empty()) return false;
    return nodes_.front().time <= time && time <= nodes_.back().time;
  }
  Rigid3d Lookup(int64_t time, size_t* interval = nullptr) const {
    const auto end = std::lower_bound(nodes_.begin(), nodes_.end(), time,
                                      [](const TimestampedTransform& node, const int64_t t) { return node.time < t; });
    if (interval != nullptr) *interval = static_cast<size_t>(end - nodes_.begin());
    g_libm_branch = false;
    if (end->time == time) return end->transform;
    return Interpolate(*std::prev(end), *end, time);
  }
  size_t size() const { return nodes_.size(); }

 private:
  std::vector<TimestampedTransform> nodes_;
};

struct Batch {
  int status = 0;
  std::vector<int32_t> index;
  std::vector<float> xyz;
  float origin[3] = {0.f, 0.f, 0.f};
  int64_t libm = 0, intervals = 0;
};

Batch HandleMessage(const TransformInterpolationBuffer& buffer, int64_t cloud_time, const Rigid3d& sensor_to_tracking,
                    const std::vector<float>& xyzt) {
  Batch batch;
  const size_t n = xyzt.size() / 4;
  for (size_t i = 0; i < n; ++i) {  // what the reference leaves undefined is refused before anything is produced
    const double ticks = static_cast<double>(xyzt[4 * i + 3]) * 1e7;
    if (!(std::abs(ticks) < 9223372036854775808.0)) {
      batch.status = -1;
      return batch;
    }
  }
  std::vector<char> used(buffer.size() + 1, 0);  // (instrumentation: which intervals the message touches)
  for (size_t i = 0; i < n; ++i) {
    // common::FromSeconds: duration_cast<Duration>(duration<double>(seconds)), truncating
    const int64_t time = static_cast<int64_t>(static_cast<uint64_t>(cloud_time) +
                                              static_cast<uint64_t>(static_cast<int64_t>(static_cast<double>(xyzt[4 * i + 3]) * 1e7)));
    if (!buffer.Has(time)) continue;
    size_t interval;
    const Rigid3d tracking_to_map = buffer.Lookup(time, &interval);
    if (g_libm_branch) ++batch.libm;
    used[interval] = 1;
    const Rigid3d product = Compose(tracking_to_map, sensor_to_tracking);
    Rigid3f sensor_to_map;  // cast<float>()
    for (int k = 0; k < 3; ++k) sensor_to_map.t[k] = static_cast<float>(product.t[k]);
    sensor_to_map.w = static_cast<float>(product.q.w);
    sensor_to_map.x = static_cast<float>(product.q.x);
    sensor_to_map.y = static_cast<float>(product.q.y);
    sensor_to_map.z = static_cast<float>(product.q.z);
    float out[3];
    RotateF(sensor_to_map, &xyzt[4 * i], out);
    for (int k = 0; k < 3; ++k) batch.xyz.push_back(out[k] + sensor_to_map.t[k]);
    batch.index.push_back(static_cast<int32_t>(i));
    const float zero[3] = {0.f, 0.f, 0.f};  // sensor_to_map * Eigen::Vector3f::Zero()
    RotateF(sensor_to_map, zero, out);
    for (int k = 0; k < 3; ++k) batch.origin[k] = out[k] + sensor_to_map.t[k];
  }
  batch.intervals = std::count(used.begin(), used.end(), 1);
  return batch;
}

template <typename T>
bool Get(FILE* f, T* v, size_t count = 1) {
  return std::fread(v, sizeof(T), count, f) == count;
}
template <typename T>
void Put(FILE* f, const T* v, size_t count = 1) {
  std::fwrite(v, sizeof(T), count, f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const bool timing = argc > 3 && std::strcmp(argv[3], "--time") == 0;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (in == nullptr || out == nullptr) return 2;
  int64_t nodes = 0;
  if (!Get(in, &nodes) || nodes < 0) return 2;
  std::vector<int64_t> times(static_cast<size_t>(nodes));
  std::vector<double> poses(7 * static_cast<size_t>(nodes));
  if (nodes > 0 && (!Get(in, times.data(), times.size()) || !Get(in, poses.data(), poses.size()))) return 2;
  TransformInterpolationBuffer buffer;
  int32_t pushed = 0;
  for (int64_t i = 0; i < nodes; ++i) {
    const double* p = &poses[7 * static_cast<size_t>(i)];
    if (!buffer.Push(times[static_cast<size_t>(i)], Rigid3d{{p[0], p[1], p[2]}, Quaterniond{p[3], p[4], p[5], p[6]}})) pushed = -1;
  }
  Put(out, &pushed);
  if (pushed != 0) {
    std::fclose(out);
    return 0;
  }
  int32_t kind;
  for (int k = 0; Get(in, &kind); ++k) {
    if (kind == 1) {
      int64_t count = 0;
      if (!Get(in, &count) || count < 0) return 2;
      std::vector<int64_t> at(static_cast<size_t>(count));
      if (count > 0 && !Get(in, at.data(), at.size())) return 2;
      for (const int64_t time : at) {
        const int32_t has = buffer.Has(time) ? 1 : 0;
        double pose[7] = {0, 0, 0, 0, 0, 0, 0};
        if (has) {
          const Rigid3d r = buffer.Lookup(time);
          const double v[7] = {r.t[0], r.t[1], r.t[2], r.q.w, r.q.x, r.q.y, r.q.z};
          std::memcpy(pose, v, sizeof pose);
        }
        Put(out, &has);
        Put(out, pose, 7);
      }
    } else if (kind == 2) {
      int64_t cloud_time = 0, n = 0;
      double s[7];
      if (!Get(in, &cloud_time) || !Get(in, s, 7) || !Get(in, &n) || n < 0) return 2;
      std::vector<float> xyzt(4 * static_cast<size_t>(n));
      if (n > 0 && !Get(in, xyzt.data(), xyzt.size())) return 2;
      const Rigid3d sensor_to_tracking{{s[0], s[1], s[2]}, Quaterniond{s[3], s[4], s[5], s[6]}};
      Batch batch = HandleMessage(buffer, cloud_time, sensor_to_tracking, xyzt);
      if (timing) {
        double best = 1e300;
        for (int rep = 0; rep < 5; ++rep) {
          const auto t0 = std::chrono::steady_clock::now();
          const Batch again = HandleMessage(buffer, cloud_time, sensor_to_tracking, xyzt);
          const auto t1 = std::chrono::steady_clock::now();
          if (again.index.size() != batch.index.size()) return 3;
          best = std::min(best, std::chrono::duration<double, std::milli>(t1 - t0).count());
        }
        std::printf("op %d %.6f\n", k, best);
      }
      const int32_t status = batch.status;
      const int64_t kept = static_cast<int64_t>(batch.index.size());
      Put(out, &status);
      Put(out, &kept);
      Put(out, batch.index.data(), batch.index.size());
      Put(out, batch.xyz.data(), batch.xyz.size());
      Put(out, batch.origin, 3);
      Put(out, &batch.libm);
      Put(out, &batch.intervals);
    } else {
      return 2;
    }
  }
  std::fclose(in);
  std::fclose(out);
  return 0;
}
