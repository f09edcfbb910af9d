// Header-only C++ adapters over the C ABI (include/dliom.h) that keep the reference's operator
// surface: same class names, method names, argument meaning and error behaviour (a failed
// CHECK in the reference == std::abort() after printing the status here).
//
//   dliom::mapping::HybridGrid                                mapping/3d/hybrid_grid.h:470-547
//   dliom::mapping::RangeDataInserter3D                       mapping/3d/range_data_inserter_3d.h:35-47
//   dliom::mapping::scan_matching::RealTimeCorrelativeScanMatcher3D
//                                  .../scan_matching/real_time_correlative_scan_matcher_3d.h:34-66
//   dliom::mapping::scan_matching::CeresScanMatcher3D         .../scan_matching/ceres_scan_matcher_3d.h:37-63
//   dliom::mapping::scan_matching::FastCorrelativeScanMatcher3D
//                                  .../scan_matching/fast_correlative_scan_matcher_3d.h:100-132
//   dliom::mapping::ActiveSubmaps3D / Submap3D                mapping/3d/submap_3d.h:43-130
//   dliom::mapping::RangeDataSynchronizer                     mapping/internal/3d/range_data_synchronizer.h
//   dliom::mapping::LocalTrajectoryBuilder3D                  mapping/internal/3d/local_trajectory_builder_3d.h:83-111
//   dliom::io::PointsBatch / PointsProcessor                  io/points_batch.h:36-73, io/points_processor.h:29-52
//   dliom::io::MinMaxRangeFiteringPointsProcessor             io/min_max_range_filtering_points_processor.h:30-53
//   dliom::io::OutlierRemovingPointsProcessor                 io/outlier_removing_points_processor.h:29-82
//   dliom::mapping::constraints::SubmapFeatureMatcher         mapping/internal/constraints/constraint_builder_3d.cc:459-529
//   dliom::io::SubmapSlice / FillSubmapSlice / PaintSubmapSlices  io/submap_painter.h:30-94 (+ CreateOccupancyGrid)
//   dliom::sensor::CompressedPointCloud                       sensor/compressed_point_cloud.h:36-95
//   dliom::registration::IterativeClosestPoint                pcl::IterativeClosestPoint as gen_ground_truth_by_ndt_match.cc:190-205 runs it
//   dliom::mapping::ToProto / FromProto(TrajectoryNode::Data) mapping/trajectory_node.h:39-69 (+ ToProto over a span of nodes)
//
// The value types below are layout-compatible stand-ins for Eigen::Vector3f / transform::Rigid3d
// so that this header builds without Eigen; inside cartographer the same adapters are
// instantiated on the real types: everything is funnelled through
// ToArray()/FromArray() on [tx,ty,tz,qw,qx,qy,qz] and packed float xyz.
#ifndef DLIOM_CPP_DLIOM_CARTOGRAPHER_H_
#define DLIOM_CPP_DLIOM_CARTOGRAPHER_H_

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <deque>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/dliom.h"

// -DDLIOM_ADAPTER_STAGE_TIMES (tools/wref_cpp.py --stages): microseconds between the marks of AddRangeData's single-sensor
// path, summed per mark.  Nothing of it exists in a normal build.
#ifdef DLIOM_ADAPTER_STAGE_TIMES
namespace dliom {
namespace stage_times {
inline double* table() {
  static double t[16] = {0};
  return t;
}
inline std::chrono::steady_clock::time_point& last() {
  static std::chrono::steady_clock::time_point p = std::chrono::steady_clock::now();
  return p;
}
inline void mark(int i) {
  const auto now = std::chrono::steady_clock::now();
  table()[i] += std::chrono::duration<double, std::micro>(now - last()).count();
  last() = now;
}
}  // namespace stage_times
}  // namespace dliom
#define DLIOM_ADAPTER_STAGE(i) ::dliom::stage_times::mark(i)
#else
#define DLIOM_ADAPTER_STAGE(i)
#endif

namespace dliom {

inline void Check(int status, const char* what) {
  if (status != DLIOM_OK) {
    std::fprintf(stderr, "Check failed: %s: %s %s\n", what, dliom_status_string(status),
                 dliom_last_error());
    std::abort();  // glog CHECK semantics of the reference
  }
}

// cartographer/metrics/{gauge,histogram,family_factory}.h: the interfaces LocalTrajectoryBuilder3D::RegisterMetrics
// (local_trajectory_builder_3d.h:113, .cc:624-649) is written against -- stand-ins like the value types below; inside
// cartographer the real headers take their place (same names, same virtuals).
namespace metrics {
class Gauge {
 public:
  static Gauge* Null() {
    struct NullGauge : Gauge {
      void Increment() override {}
      void Increment(double) override {}
      void Decrement() override {}
      void Decrement(double) override {}
      void Set(double) override {}
    };
    static NullGauge null_gauge;
    return &null_gauge;
  }
  virtual ~Gauge() = default;
  virtual void Increment() = 0;
  virtual void Increment(double by_value) = 0;
  virtual void Decrement() = 0;
  virtual void Decrement(double by_value) = 0;
  virtual void Set(double value) = 0;
};
class Histogram {
 public:
  using BucketBoundaries = std::vector<double>;
  static Histogram* Null() {
    struct NullHistogram : Histogram {
      void Observe(double) override {}
    };
    static NullHistogram null_histogram;
    return &null_histogram;
  }
  static BucketBoundaries FixedWidth(double width, int num_finite_buckets) {  // metrics/histogram.cc:37-46
    BucketBoundaries result;
    for (int i = 1; i <= num_finite_buckets; ++i) result.push_back(width * i);
    return result;
  }
  static BucketBoundaries ScaledPowersOf(double base, double scale_factor, double max_value) {  // :48-60
    BucketBoundaries result;
    if (!(base > 1) || !(scale_factor > 0)) Check(DLIOM_ERR_INVALID_ARGUMENT, "Histogram::ScaledPowersOf");
    for (double boundary = scale_factor; boundary < max_value; boundary *= base) result.push_back(boundary);
    return result;
  }
  virtual ~Histogram() = default;
  virtual void Observe(double value) = 0;
};
template <typename MetricType>
class Family {
 public:
  virtual ~Family() = default;
  virtual MetricType* Add(const std::map<std::string, std::string>& labels) = 0;
};
class FamilyFactory {  // (NewCounterFamily is not used on this path)
 public:
  virtual ~FamilyFactory() = default;
  virtual Family<Gauge>* NewGaugeFamily(const std::string& name, const std::string& description) = 0;
  virtual Family<Histogram>* NewHistogramFamily(const std::string& name, const std::string& description,
                                                const Histogram::BucketBoundaries& boundaries) = 0;
};
}  // namespace metrics

namespace common {
// common::optional (common/optional.h), the part the adapters use; T is default-constructible here
template <typename T>
class optional {
 public:
  optional() : has_value_(false), value_() {}
  optional(const T& value) : has_value_(true), value_(value) {}  // NOLINT: converting, like the reference's
  bool has_value() const { return has_value_; }
  const T& value() const {
    if (!has_value_) Check(DLIOM_ERR_INVALID_ARGUMENT, "optional::value: CHECK(has_value())");
    return value_;
  }

 private:
  bool has_value_;
  T value_;
};
// common::FastGzipString (common/port.h:46-53) for what is small and on the host, such as a SerializationHeader: one
// member of dliom.h "gzip on the device" (dliom_gzip_host).  FastGunzipString, or any inflater, reads it; the bytes are
// not zlib's.
inline void FastGzipString(const std::string& uncompressed, std::string* compressed) {
  compressed->assign(static_cast<size_t>(dliom_gzip_bound(static_cast<int64_t>(uncompressed.size()))), '\0');
  int64_t size = 0;
  Check(dliom_gzip_host(reinterpret_cast<const uint8_t*>(uncompressed.data()), static_cast<int64_t>(uncompressed.size()),
                        reinterpret_cast<uint8_t*>(&(*compressed)[0]), static_cast<int64_t>(compressed->size()), &size), "FastGzipString");
  compressed->resize(static_cast<size_t>(size));
}
}  // namespace common

// asks an adapter method for bytes that left the device gzipped (opt-in: the methods without it keep their behaviour)
enum GzipTag { kGzipped };

namespace transform {
struct Vector3d {
  double v[3];
  double x() const { return v[0]; }
  double y() const { return v[1]; }
  double z() const { return v[2]; }
};
struct Quaterniond {
  double wxyz[4];
  double w() const { return wxyz[0]; }
  double x() const { return wxyz[1]; }
  double y() const { return wxyz[2]; }
  double z() const { return wxyz[3]; }
};
class Rigid3d {
 public:
  Rigid3d() : t_{{0, 0, 0}}, q_{{1, 0, 0, 0}} {}
  Rigid3d(const Vector3d& t, const Quaterniond& q) : t_(t), q_(q) {}
  static Rigid3d Translation(const Vector3d& t) { return Rigid3d(t, Quaterniond{{1, 0, 0, 0}}); }
  const Vector3d& translation() const { return t_; }
  const Quaterniond& rotation() const { return q_; }
  std::array<double, 7> ToArray() const {
    return {{t_.v[0], t_.v[1], t_.v[2], q_.wxyz[0], q_.wxyz[1], q_.wxyz[2], q_.wxyz[3]}};
  }
  static Rigid3d FromArray(const double* a) {
    return Rigid3d(Vector3d{{a[0], a[1], a[2]}}, Quaterniond{{a[3], a[4], a[5], a[6]}});
  }

 private:
  Vector3d t_;
  Quaterniond q_;
};
// transform::Rigid3f, the part the X-ray stage uses: [tx, ty, tz] and (w, x, y, z)
struct Rigid3f {
  float t[3] = {0.f, 0.f, 0.f};
  float wxyz[4] = {1.f, 0.f, 0.f, 0.f};
  Rigid3f() {}
  Rigid3f(float tx, float ty, float tz, float w, float x, float y, float z) : t{tx, ty, tz}, wxyz{w, x, y, z} {}
  explicit Rigid3f(const Rigid3d& d)  // Rigid3d::cast<float>()
      : t{static_cast<float>(d.translation().v[0]), static_cast<float>(d.translation().v[1]), static_cast<float>(d.translation().v[2])},
        wxyz{static_cast<float>(d.rotation().wxyz[0]), static_cast<float>(d.rotation().wxyz[1]),
             static_cast<float>(d.rotation().wxyz[2]), static_cast<float>(d.rotation().wxyz[3])} {}
  std::array<float, 7> ToArray() const { return {{t[0], t[1], t[2], wxyz[0], wxyz[1], wxyz[2], wxyz[3]}}; }
};
}  // namespace transform

namespace sensor {
struct Vector3f {
  float x, y, z;
  Vector3f() {}  // uninitialised like Eigen::Vector3f's: resizing a cloud that a download fills does not zero it first
  Vector3f(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};
static_assert(sizeof(Vector3f) == 12, "packed xyz like Eigen::Vector3f");
using PointCloud = std::vector<Vector3f>;
struct RangeData {
  Vector3f origin;
  PointCloud returns;
  PointCloud misses;
};
}  // namespace sensor

// One per calling thread (the reference's matchers are re-entered from pool threads:
// constraint_builder_3d.cc:320).
class Context {
 public:
  explicit Context(int device_id = 0) { Check(dliom_ctx_create(device_id, &ctx_), "dliom_ctx_create"); }
  ~Context() { dliom_ctx_destroy(ctx_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  dliom_ctx* get() const { return ctx_; }
  // The calling thread's own context on `device_id` (created on first use, destroyed with the thread): what the
  // const, concurrently called members of the reference (FastCorrelativeScanMatcher3D::Match from the
  // ConstraintBuilder3D pool threads, constraint_builder_3d.cc:270-275) run on.
  static Context* ForThisThread(int device_id = 0) {
    struct Slot {
      int device = -1;
      Context* ctx = nullptr;
      ~Slot() { delete ctx; }
    };
    static thread_local Slot slots[8];
    for (Slot& s : slots) {
      if (s.ctx != nullptr && s.device == device_id) return s.ctx;
      if (s.ctx == nullptr) {
        s.device = device_id;
        s.ctx = new Context(device_id);
        return s.ctx;
      }
    }
    Check(DLIOM_ERR_INVALID_ARGUMENT, "Context::ForThisThread: more than 8 devices per thread");
    return nullptr;
  }

 private:
  dliom_ctx* ctx_ = nullptr;
};

// The scans the D-LIOM fork keeps for its map cloud and its range-data file (cartographer_ros/map_builder_bridge.cc:591-607
// range_data_local_all_), kept in HBM where the scan matcher left them (dliom.h "node clouds kept in HBM"), and the fork's
// three per-point loops over them as batched device calls.  The static Host* members are the reference's loops, one
// thread: the cross-check of the device calls and the baseline of tools/node_clouds_bench.py.
namespace cartographer_ros {
class NodeCloudCache {
 public:
  // msg.data of several PointCloud2 messages back to back: node nodes[i]'s is data[offsets[i], offsets[i + 1])
  struct CloudData {
    std::vector<uint8_t> data;
    std::vector<int64_t> offsets{0};
    std::vector<int64_t> nodes;
  };
  explicit NodeCloudCache(Context* context) : context_(context) {
    Check(dliom_node_clouds_create(context->get(), &clouds_), "dliom_node_clouds_create");
  }
  ~NodeCloudCache() { dliom_node_clouds_destroy(clouds_); }
  NodeCloudCache(const NodeCloudCache&) = delete;
  NodeCloudCache& operator=(const NodeCloudCache&) = delete;
  dliom_node_clouds* get() const { return clouds_; }
  int64_t size() const { return static_cast<int64_t>(order_.size()); }

  // MapBuilderBridge::OnLocalSlamResult with the scan still on the device: `returns` in the tracking frame and
  // pose_to_local = opt_pose.cast<float>() (TransformRangeData on the way in), or already local and pose_to_local null.
  // One kernel, nothing waited for.  Returns the node's index in the cache.
  int64_t OnLocalSlamResult(int trajectory_id, int64_t time, const transform::Rigid3d& local_pose, const dliom_cloud* returns,
                            const float* pose_to_local, const sensor::Vector3f& origin_in_local, const dliom_cloud* misses = nullptr) {
    dliom_node_cloud_info info;
    info.timestamp = time;
    info.trajectory_id = trajectory_id;
    info.node_index = 0;  // SerializeRangeData never sets it
    const std::array<double, 7> pose = local_pose.ToArray();
    std::copy(pose.begin(), pose.end(), info.local_pose7);
    info.origin_in_local[0] = origin_in_local.x;
    info.origin_in_local[1] = origin_in_local.y;
    info.origin_in_local[2] = origin_in_local.z;
    int64_t index = -1;
    Check(dliom_node_clouds_add(clouds_, &info, returns, misses, pose_to_local, &index), "NodeCloudCache::OnLocalSlamResult");
    by_trajectory_[trajectory_id].push_back(index);
    order_.push_back(info);
    return index;
  }
  // ... with the scan on the host, as the reference's callback receives it (two uploads)
  int64_t OnLocalSlamResult(int trajectory_id, int64_t time, const transform::Rigid3d& local_pose,
                            const sensor::RangeData& range_data_in_local) {
    dliom_cloud *returns = nullptr, *misses = nullptr;
    const sensor::PointCloud &r = range_data_in_local.returns, &m = range_data_in_local.misses;
    Check(dliom_cloud_create(context_->get(), r.empty() ? nullptr : &r[0].x, static_cast<int64_t>(r.size()), &returns), "dliom_cloud_create");
    Check(dliom_cloud_create(context_->get(), m.empty() ? nullptr : &m[0].x, static_cast<int64_t>(m.size()), &misses), "dliom_cloud_create");
    const int64_t index = OnLocalSlamResult(trajectory_id, time, local_pose, returns, nullptr, range_data_in_local.origin, misses);
    Check(dliom_ctx_synchronize(context_->get()), "dliom_ctx_synchronize");  // the kernel reads the two clouds
    dliom_cloud_destroy(returns);
    dliom_cloud_destroy(misses);
    return index;
  }

  // MapBuilderBridge::SerializeRangeData's loop (:177-195): write(data, size) once a NodeRangeData message, trajectories in
  // map order, a trajectory's nodes in insertion order.  The header and the framing stay with the caller's writer.
  template <class WriteProto>
  void SerializeRangeData(WriteProto&& write) const {
    const std::vector<int64_t> nodes = NodesInMapOrder();
    ForRuns(nodes, [&](int64_t first, int64_t count) {
      std::vector<int64_t> offsets(static_cast<size_t>(count) + 1);
      int64_t capacity = 0;  // the bound that needs no size query: one pass over the points, not two
      for (int64_t i = first; i < first + count; ++i) {
        int64_t returns = 0, misses = 0;
        Check(dliom_node_clouds_info(clouds_, i, nullptr, &returns, &misses), "dliom_node_clouds_info");
        capacity += DLIOM_NODE_RANGE_MAX_HEADER + DLIOM_NODE_RANGE_MAX_RECORD * (returns + misses);
      }
      std::vector<uint8_t> bytes(static_cast<size_t>(capacity));
      Check(dliom_node_clouds_to_proto(clouds_, first, count, nullptr, bytes.data(), capacity, offsets.data(), nullptr), "SerializeRangeData");
      for (int64_t i = 0; i < count; ++i) write(bytes.data() + offsets[i], static_cast<size_t>(offsets[i + 1] - offsets[i]));
    });
  }
  // ... with ProtoStreamWriter::WriteProto's framing (proto_stream.cc:50-57) done on the device: write(data, size) once a
  // node with the 8-byte little-endian compressed size and the gzip member behind it -- the bytes WriteProto puts into the
  // file for that message.  The messages never reach the host uncompressed.  Opt-in.
  template <class WriteRecord>
  void SerializeRangeDataFramed(WriteRecord&& write) const {
    const std::vector<int64_t> nodes = NodesInMapOrder();
    ForRuns(nodes, [&](int64_t first, int64_t count) {
      std::vector<int64_t> offsets(static_cast<size_t>(count) + 1);
      int64_t capacity = 0;  // the bound that never fails
      for (int64_t i = first; i < first + count; ++i) {
        int64_t returns = 0, misses = 0;
        Check(dliom_node_clouds_info(clouds_, i, nullptr, &returns, &misses), "dliom_node_clouds_info");
        capacity += 8 + dliom_gzip_bound(DLIOM_NODE_RANGE_MAX_HEADER + DLIOM_NODE_RANGE_MAX_RECORD * (returns + misses));
      }
      std::vector<uint8_t> bytes(static_cast<size_t>(capacity));
      Check(dliom_node_clouds_to_pbstream(clouds_, first, count, nullptr, bytes.data(), capacity, offsets.data(), nullptr, nullptr),
            "SerializeRangeDataFramed");
      for (int64_t i = 0; i < count; ++i) write(bytes.data() + offsets[i], static_cast<size_t>(offsets[i + 1] - offsets[i]));
    });
  }
  // msg.data of the nodes [first, first + count) under num_poses float poses (shared, or node-major per node)
  CloudData ToPointCloud2Data(int64_t first, int64_t count, const float* poses7, int num_poses, bool per_node) const {
    CloudData out;
    Append(first, count, poses7, num_poses, per_node, &out);
    return out;
  }
  // Node::PublishFullMapCloud's loop (node.cc:334-351): every kept scan under local_to_map.cast<float>()
  CloudData FullMapCloud(const transform::Rigid3d& local_to_map) const {
    const std::array<float, 7> pose = transform::Rigid3f(local_to_map).ToArray();
    CloudData out;
    ForRuns(NodesInMapOrder(), [&](int64_t first, int64_t count) { Append(first, count, pose.data(), 1, false, &out); });
    return out;
  }
  // pb_range_data_to_ros_cloud's loop (:153-186): global_pose * (local_pose.inverse() * p), both in float, for every kept
  // scan whose timestamp node_table holds; the others are skipped (:157)
  CloudData GlobalClouds(const std::map<int64_t, transform::Rigid3d>& node_table) const {
    CloudData out;
    std::vector<float> poses;
    int64_t first = 0;
    auto flush = [&](int64_t end) {
      if (!poses.empty()) Append(first, end - first, poses.data(), 2, true, &out);
      poses.clear();
    };
    for (int64_t i = 0; i < size(); ++i) {
      const auto found = node_table.find(order_[static_cast<size_t>(i)].timestamp);
      if (found == node_table.end()) {
        flush(i);
        continue;
      }
      if (poses.empty()) first = i;
      const std::array<float, 7> local = transform::Rigid3f(transform::Rigid3d::FromArray(order_[static_cast<size_t>(i)].local_pose7)).ToArray();
      const std::array<float, 7> global = transform::Rigid3f(found->second).ToArray();
      float inverse[7];
      Check(dliom_rigid3f_inverse(local.data(), inverse), "dliom_rigid3f_inverse");
      poses.insert(poses.end(), inverse, inverse + 7);
      poses.insert(poses.end(), global.begin(), global.end());
    }
    flush(size());
    return out;
  }
  std::vector<int64_t> NodesInMapOrder() const {
    std::vector<int64_t> nodes;
    for (const auto& trajectory : by_trajectory_) nodes.insert(nodes.end(), trajectory.second.begin(), trajectory.second.end());
    return nodes;
  }

  // ---- the reference's loops on the host, one thread ----
  // Rigid3f * Vector3f in Eigen's operation order
  static sensor::Vector3f HostTransform(const float p7[7], const sensor::Vector3f& p) {
    const float w = p7[3], qx = p7[4], qy = p7[5], qz = p7[6];
    float uvx = qy * p.z - qz * p.y, uvy = qz * p.x - qx * p.z, uvz = qx * p.y - qy * p.x;
    uvx += uvx;
    uvy += uvy;
    uvz += uvz;
    const float cx = qy * uvz - qz * uvy, cy = qz * uvx - qx * uvz, cz = qx * uvy - qy * uvx;
    return sensor::Vector3f(((p.x + w * uvx) + cx) + p7[0], ((p.y + w * uvy) + cy) + p7[1], ((p.z + w * uvz) + cz) + p7[2]);
  }
  // the stream.next() loop: x, y, z, kPointCloudComponentFourMagic of every return, moved by the poses in turn
  static void HostPointCloud2Data(const sensor::PointCloud& returns, const float* poses7, int num_poses, std::vector<uint8_t>* data) {
    const size_t at = data->size();
    data->resize(at + 16 * returns.size());
    uint8_t* out = data->data() + at;
    for (const sensor::Vector3f& point : returns) {
      sensor::Vector3f p = point;
      for (int k = 0; k < num_poses; ++k) p = HostTransform(poses7 + 7 * k, p);
      const float record[4] = {p.x, p.y, p.z, 1.0f};
      std::memcpy(out, record, 16);
      out += 16;
    }
  }
  // sensor::ToProto(RangeData) and the message around it, serialised (implicit presence: v == 0 is not written)
  static void HostNodeRangeData(int trajectory_id, int64_t time, const transform::Rigid3d& local_pose, const sensor::RangeData& range_data,
                                std::vector<uint8_t>* out) {
    auto varint = [](std::vector<uint8_t>* o, uint64_t v) {
      for (; v >= 0x80; v >>= 7) o->push_back(static_cast<uint8_t>(v) | 0x80);
      o->push_back(static_cast<uint8_t>(v));
    };
    auto scalar = [](std::vector<uint8_t>* o, int field, int wire, const void* v, size_t n) {
      o->push_back(static_cast<uint8_t>(field << 3 | wire));
      const uint8_t* b = static_cast<const uint8_t*>(v);
      o->insert(o->end(), b, b + n);
    };
    auto message = [&](std::vector<uint8_t>* o, int field, const std::vector<uint8_t>& payload) {
      o->push_back(static_cast<uint8_t>(field << 3 | 2));
      varint(o, payload.size());
      o->insert(o->end(), payload.begin(), payload.end());
    };
    auto vector3f = [&](std::vector<uint8_t>* o, int field, const sensor::Vector3f& p) {
      uint8_t record[17];
      size_t n = 2;
      const float v[3] = {p.x, p.y, p.z};
      for (int i = 0; i < 3; ++i) {
        if (v[i] == 0.f) continue;
        record[n] = static_cast<uint8_t>((i + 1) << 3 | 5);
        std::memcpy(record + n + 1, &v[i], 4);
        n += 5;
      }
      record[0] = static_cast<uint8_t>(field << 3 | 2);
      record[1] = static_cast<uint8_t>(n - 2);
      o->insert(o->end(), record, record + n);
    };
    if (time != 0) {
      out->push_back(1 << 3);
      varint(out, static_cast<uint64_t>(time));
    }
    if (trajectory_id != 0) {
      out->push_back(2 << 3);
      varint(out, static_cast<uint64_t>(static_cast<int64_t>(trajectory_id)));
    }
    std::vector<uint8_t> translation, rotation, pose, range;
    const std::array<double, 7> p = local_pose.ToArray();
    for (int i = 0; i < 3; ++i)
      if (p[i] != 0.0) scalar(&translation, i + 1, 1, &p[i], 8);
    const double xyzw[4] = {p[4], p[5], p[6], p[3]};
    for (int i = 0; i < 4; ++i)
      if (xyzw[i] != 0.0) scalar(&rotation, i + 1, 1, &xyzw[i], 8);
    message(&pose, 1, translation);
    message(&pose, 2, rotation);
    message(out, 4, pose);
    range.reserve(19 + 17 * (range_data.returns.size() + range_data.misses.size()));
    vector3f(&range, 1, range_data.origin);
    for (const sensor::Vector3f& point : range_data.returns) vector3f(&range, 2, point);
    for (const sensor::Vector3f& point : range_data.misses) vector3f(&range, 3, point);
    message(out, 5, range);
  }

 private:
  // maximal runs of consecutive cache indices, in the order given: a single trajectory is one run, one batched call
  template <class F>
  static void ForRuns(const std::vector<int64_t>& nodes, F&& f) {
    for (size_t a = 0; a < nodes.size();) {
      size_t b = a + 1;
      while (b < nodes.size() && nodes[b] == nodes[b - 1] + 1) ++b;
      f(nodes[a], static_cast<int64_t>(b - a));
      a = b;
    }
  }
  void Append(int64_t first, int64_t count, const float* poses7, int num_poses, bool per_node, CloudData* out) const {
    dliom_node_clouds_transform t;
    t.num_poses = num_poses;
    t.per_node = per_node ? 1 : 0;
    t.poses7 = poses7;
    std::vector<int64_t> offsets(static_cast<size_t>(count) + 1);
    Check(dliom_node_clouds_pack_point_cloud2(clouds_, first, count, &t, nullptr, nullptr, 0, offsets.data(), nullptr), "ToPointCloud2Data (sizes)");
    const size_t at = out->data.size();
    out->data.resize(at + static_cast<size_t>(offsets[count]));
    Check(dliom_node_clouds_pack_point_cloud2(clouds_, first, count, &t, nullptr, out->data.data() + at, offsets[count], offsets.data(), nullptr),
          "ToPointCloud2Data");
    for (int64_t i = 0; i < count; ++i) {
      out->nodes.push_back(first + i);
      out->offsets.push_back(static_cast<int64_t>(at) + offsets[i + 1]);
    }
  }
  Context* context_;
  dliom_node_clouds* clouds_ = nullptr;
  std::map<int, std::vector<int64_t>> by_trajectory_;
  std::vector<dliom_node_cloud_info> order_;  // the nodes' infos, by cache index
};
}  // namespace cartographer_ros

namespace mapping {

class HybridGrid {
 public:
  HybridGrid(Context* context, float resolution) : resolution_(resolution) {
    Check(dliom_grid_create(context->get(), resolution, &grid_), "dliom_grid_create");
  }
  ~HybridGrid() { dliom_grid_destroy(grid_); }
  HybridGrid(const HybridGrid&) = delete;
  HybridGrid& operator=(const HybridGrid&) = delete;
  float resolution() const { return resolution_; }
  dliom_grid* get() const { return grid_; }
  // hybrid_grid.h:489-491
  void SetProbability(const std::array<int32_t, 3>& index, float probability) {
    const uint16_t v = dliom_probability_to_value(probability);
    Check(dliom_grid_set_values(grid_, index.data(), &v, 1), "dliom_grid_set_values");
  }
  // hybrid_grid.h:430-435 (host arithmetic: true float division + lround)
  std::array<int32_t, 3> GetCellIndex(const sensor::Vector3f& p) const {
    return {{static_cast<int32_t>(std::lround(p.x / resolution_)),
             static_cast<int32_t>(std::lround(p.y / resolution_)),
             static_cast<int32_t>(std::lround(p.z / resolution_))}};
  }
  // HybridGrid::value for a batch of cell indices (packed int xyz).
  std::vector<uint16_t> values(const std::vector<std::array<int32_t, 3>>& cells) const {
    std::vector<uint16_t> out(cells.size());
    Check(dliom_grid_get_values(grid_, cells.empty() ? nullptr : cells[0].data(),
                                static_cast<int64_t>(cells.size()), out.data()),
          "dliom_grid_get_values");
    return out;
  }

 private:
  float resolution_;
  dliom_grid* grid_ = nullptr;
};

struct RangeDataInserterOptions3D {  // proto/3d/range_data_inserter_options_3d.proto
  double hit_probability;
  double miss_probability;
  int num_free_space_voxels;
};

class RangeDataInserter3D {
 public:
  RangeDataInserter3D(Context* context, const RangeDataInserterOptions3D& options) {
    Check(dliom_inserter_create(context->get(), options.hit_probability, options.miss_probability,
                                options.num_free_space_voxels, &inserter_),
          "dliom_inserter_create (CHECK_GT(hit, 0.5), CHECK_LT(miss, 0.5))");
  }
  ~RangeDataInserter3D() { dliom_inserter_destroy(inserter_); }
  RangeDataInserter3D(const RangeDataInserter3D&) = delete;
  RangeDataInserter3D& operator=(const RangeDataInserter3D&) = delete;
  // range_data_inserter_3d.cc:78-92
  void Insert(const sensor::RangeData& range_data, HybridGrid* hybrid_grid) const {
    if (hybrid_grid == nullptr) Check(DLIOM_ERR_INVALID_ARGUMENT, "CHECK_NOTNULL(hybrid_grid)");
    const float origin[3] = {range_data.origin.x, range_data.origin.y, range_data.origin.z};
    Check(dliom_inserter_insert(inserter_, hybrid_grid->get(), origin,
                                range_data.returns.empty() ? nullptr : &range_data.returns[0].x,
                                static_cast<int64_t>(range_data.returns.size())),
          "dliom_inserter_insert");
  }

 private:
  dliom_inserter* inserter_ = nullptr;
};

namespace scan_matching {

using RealTimeCorrelativeScanMatcherOptions = dliom_rtcsm_options;

class RealTimeCorrelativeScanMatcher3D {
 public:
  RealTimeCorrelativeScanMatcher3D(Context* context,
                                   const RealTimeCorrelativeScanMatcherOptions& options)
      : context_(context), options_(options) {}
  // real_time_correlative_scan_matcher_3d.h:47-50
  float Match(const transform::Rigid3d& initial_pose_estimate, const sensor::PointCloud& point_cloud,
              const HybridGrid& hybrid_grid, transform::Rigid3d* pose_estimate) const {
    if (pose_estimate == nullptr) Check(DLIOM_ERR_INVALID_ARGUMENT, "CHECK_NOTNULL(pose_estimate)");
    const std::array<double, 7> init = initial_pose_estimate.ToArray();
    double out[7];
    float score = 0.f;
    Check(dliom_rtcsm3d_match(context_->get(), &options_, init.data(),
                              point_cloud.empty() ? nullptr : &point_cloud[0].x,
                              static_cast<int64_t>(point_cloud.size()), hybrid_grid.get(), out, &score),
          "RealTimeCorrelativeScanMatcher3D::Match");
    *pose_estimate = transform::Rigid3d::FromArray(out);
    return score;
  }

 private:
  Context* context_;
  const RealTimeCorrelativeScanMatcherOptions options_;
};

struct CeresScanMatcherOptions3D {  // proto/scan_matching/ceres_scan_matcher_options_3d.proto
  std::vector<double> occupied_space_weight;
  double translation_weight = 0;
  double rotation_weight = 0;
  bool only_optimize_yaw = false;
  bool use_nonmonotonic_steps = false;  // ceres_solver_options
  int max_num_iterations = 50;
  int num_threads = 1;
};

using Summary = dliom_csm_summary;  // the fields of ceres::Solver::Summary the path reads

class CeresScanMatcher3D {
 public:
  using PointCloudAndHybridGridPointers = std::pair<const sensor::PointCloud*, const HybridGrid*>;

  CeresScanMatcher3D(Context* context, const CeresScanMatcherOptions3D& options) : context_(context) {
    options_.num_occupied_space_weights = static_cast<int>(options.occupied_space_weight.size());
    for (size_t i = 0; i < options.occupied_space_weight.size() && i < DLIOM_MAX_CLOUDS; ++i)
      options_.occupied_space_weight[i] = options.occupied_space_weight[i];
    options_.translation_weight = options.translation_weight;
    options_.rotation_weight = options.rotation_weight;
    options_.only_optimize_yaw = options.only_optimize_yaw;
    options_.use_nonmonotonic_steps = options.use_nonmonotonic_steps;
    options_.max_num_iterations = options.max_num_iterations;
    options_.num_threads = options.num_threads;
  }
  // ceres_scan_matcher_3d.h:51-56
  void Match(const transform::Vector3d& target_translation,
             const transform::Rigid3d& initial_pose_estimate,
             const std::vector<PointCloudAndHybridGridPointers>& point_clouds_and_hybrid_grids,
             transform::Rigid3d* pose_estimate, Summary* summary) const {
    const int k = static_cast<int>(point_clouds_and_hybrid_grids.size());
    std::vector<const float*> pts(k);
    std::vector<int64_t> n(k);
    std::vector<const dliom_grid*> grids(k);
    for (int i = 0; i < k; ++i) {
      const sensor::PointCloud& c = *point_clouds_and_hybrid_grids[i].first;
      pts[i] = c.empty() ? nullptr : &c[0].x;
      n[i] = static_cast<int64_t>(c.size());
      grids[i] = point_clouds_and_hybrid_grids[i].second->get();
    }
    const std::array<double, 7> init = initial_pose_estimate.ToArray();
    double out[7];
    Check(dliom_csm3d_match(context_->get(), &options_, target_translation.v, init.data(), k, pts.data(),
                            n.data(), grids.data(), out, summary),
          "CeresScanMatcher3D::Match");
    *pose_estimate = transform::Rigid3d::FromArray(out);
  }
  // Match for a list of problems in one call (dliom_csm3d_match_batch): every pose and summary equals Match's.
  struct Problem {
    transform::Vector3d target_translation;
    transform::Rigid3d initial_pose_estimate;
    std::vector<PointCloudAndHybridGridPointers> point_clouds_and_hybrid_grids;
  };
  void MatchBatch(const std::vector<Problem>& problems, std::vector<transform::Rigid3d>* pose_estimates,
                  std::vector<Summary>* summaries, dliom_batch_stats* stats = nullptr) const {
    const int count = static_cast<int>(problems.size());
    std::vector<dliom_csm_problem> p(count);
    for (int i = 0; i < count; ++i) {
      dliom_csm_problem& q = p[i];
      q = dliom_csm_problem{};
      for (int a = 0; a < 3; ++a) q.target_translation[a] = problems[i].target_translation.v[a];
      const std::array<double, 7> init = problems[i].initial_pose_estimate.ToArray();
      for (int a = 0; a < 7; ++a) q.initial_pose_estimate[a] = init[a];
      const auto& pairs = problems[i].point_clouds_and_hybrid_grids;
      q.num_clouds = static_cast<int>(pairs.size());
      for (size_t j = 0; j < pairs.size() && j < DLIOM_MAX_CLOUDS; ++j) {
        const sensor::PointCloud& c = *pairs[j].first;
        q.points_xyz[j] = c.empty() ? nullptr : &c[0].x;
        q.n[j] = static_cast<int64_t>(c.size());
        q.grids[j] = pairs[j].second->get();
      }
    }
    std::vector<double> out(7 * static_cast<size_t>(count));
    std::vector<int> statuses(count);
    summaries->resize(count);
    Check(dliom_csm3d_match_batch(context_->get(), &options_, count, p.data(), out.data(), summaries->data(), statuses.data(), stats),
          "CeresScanMatcher3D::MatchBatch");
    pose_estimates->resize(count);
    for (int i = 0; i < count; ++i) {
      Check(statuses[i], "CeresScanMatcher3D::MatchBatch");
      (*pose_estimates)[i] = transform::Rigid3d::FromArray(&out[7 * static_cast<size_t>(i)]);
    }
  }

 private:
  Context* context_;
  dliom_csm_options options_ = {};
};

// proto/scan_matching/fast_correlative_scan_matcher_options_3d.proto
using FastCorrelativeScanMatcherOptions3D = dliom_fast_csm_options;

// The fields of mapping::TrajectoryNode::Data the loop-closure matcher reads
// (mapping/trajectory_node.h:45-69).
struct TrajectoryNodeData {
  transform::Quaterniond gravity_alignment{{1, 0, 0, 0}};
  sensor::PointCloud high_resolution_point_cloud;
  sensor::PointCloud low_resolution_point_cloud;
  std::vector<float> rotational_scan_matcher_histogram;
};

// fast_correlative_scan_matcher_3d.h:100-132.  `nodes` are passed as the (histogram, yaw) pairs the
// reference's HistogramsAtAnglesFromNodes (fast_correlative_scan_matcher_3d.cc:114-127) extracts.
class FastCorrelativeScanMatcher3D {
 public:
  struct Result {
    float score;
    transform::Rigid3d pose_estimate;
    float rotational_score;
    float low_resolution_score;
  };

  FastCorrelativeScanMatcher3D(Context* context, const HybridGrid& hybrid_grid,
                               const HybridGrid* low_resolution_hybrid_grid,
                               const std::vector<std::pair<std::vector<float>, float>>& histograms_at_angles,
                               const FastCorrelativeScanMatcherOptions3D& options) {
    if (low_resolution_hybrid_grid == nullptr || histograms_at_angles.empty())
      Check(DLIOM_ERR_INVALID_ARGUMENT, "FastCorrelativeScanMatcher3D: nodes.at(0) / low resolution grid");
    histogram_size_ = static_cast<int>(histograms_at_angles[0].first.size());
    std::vector<float> h, a;
    for (const auto& ha : histograms_at_angles) {
      h.insert(h.end(), ha.first.begin(), ha.first.end());
      a.push_back(ha.second);
    }
    device_ = dliom_ctx_device(context->get());
    Check(dliom_fast_csm_create(context->get(), hybrid_grid.get(), low_resolution_hybrid_grid->get(), h.data(), a.data(),
                                static_cast<int>(a.size()), histogram_size_, &options, &matcher_),
          "dliom_fast_csm_create (CHECK_GE(branch_and_bound_depth, 1), CHECK_GE(full_resolution_depth, 1))");
  }
  ~FastCorrelativeScanMatcher3D() { dliom_fast_csm_destroy(matcher_); }
  FastCorrelativeScanMatcher3D(const FastCorrelativeScanMatcher3D&) = delete;
  FastCorrelativeScanMatcher3D& operator=(const FastCorrelativeScanMatcher3D&) = delete;

  // Returns false where the reference returns nullptr.  const and re-entrant like the reference's: every calling
  // thread works on its own context; the matcher (pyramid, histogram) is only read.
  bool Match(const transform::Rigid3d& global_node_pose, const transform::Rigid3d& global_submap_pose,
             const TrajectoryNodeData& constant_data, float min_score, Result* result) const {
    const dliom_fast_csm_node_data d = Data(constant_data);
    dliom_fast_csm_result r;
    Check(dliom_fast_csm_match(Context::ForThisThread(device_)->get(), matcher_, global_node_pose.ToArray().data(), global_submap_pose.ToArray().data(), &d,
                               min_score, &r),
          "FastCorrelativeScanMatcher3D::Match");
    return Store(r, result);
  }
  bool MatchFullSubmap(const transform::Quaterniond& global_node_rotation,
                       const transform::Quaterniond& global_submap_rotation, const TrajectoryNodeData& constant_data,
                       float min_score, Result* result) const {
    const dliom_fast_csm_node_data d = Data(constant_data);
    dliom_fast_csm_result r;
    Check(dliom_fast_csm_match_full_submap(Context::ForThisThread(device_)->get(), matcher_, global_node_rotation.wxyz, global_submap_rotation.wxyz, &d,
                                           min_score, &r),
          "FastCorrelativeScanMatcher3D::MatchFullSubmap");
    return Store(r, result);
  }
  bool MatchWith3DofInitial(const transform::Rigid3d& pose_in_submap_guess, const TrajectoryNodeData& constant_data,
                            float min_score, Result* result) const {
    const dliom_fast_csm_node_data d = Data(constant_data);
    dliom_fast_csm_result r;
    Check(dliom_fast_csm_match_with_3dof_initial(Context::ForThisThread(device_)->get(), matcher_, pose_in_submap_guess.ToArray().data(), &d, min_score, &r),
          "FastCorrelativeScanMatcher3D::MatchWith3DofInitial");
    return Store(r, result);
  }

  // One search of a batch: the matcher (submap) it runs on, its kind and that kind's pose arguments.
  enum class Kind { kMatch = DLIOM_FAST_CSM_MATCH, kMatchFullSubmap = DLIOM_FAST_CSM_MATCH_FULL_SUBMAP,
                    kMatchWith3DofInitial = DLIOM_FAST_CSM_MATCH_WITH_3DOF_INITIAL };
  struct Query {
    const FastCorrelativeScanMatcher3D* matcher;
    Kind kind;
    transform::Rigid3d pose;         // Match: global_node_pose; MatchFullSubmap: its rotation; 3-DoF: the guess
    transform::Rigid3d submap_pose;  // Match: global_submap_pose; MatchFullSubmap: its rotation
    const TrajectoryNodeData* constant_data;
    float min_score;
  };
  // All queries in one call (dliom_fast_csm_match_batch) on the calling thread's context.  found[i] / results[i] =
  // what the single call for queries[i] returns.
  static void MatchBatch(const std::vector<Query>& queries, std::vector<bool>* found, std::vector<Result>* results,
                         dliom_batch_stats* stats = nullptr) {
    const int count = static_cast<int>(queries.size());
    std::vector<dliom_fast_csm_query> q(count);
    int device = 0;
    for (int i = 0; i < count; ++i) {
      const Query& in = queries[i];
      device = in.matcher->device_;
      dliom_fast_csm_query& a = q[i];
      a = dliom_fast_csm_query{};
      a.kind = static_cast<int>(in.kind);
      a.matcher = in.matcher->matcher_;
      const std::array<double, 7> p = in.pose.ToArray(), sp = in.submap_pose.ToArray();
      if (in.kind == Kind::kMatchFullSubmap) {
        for (int k = 0; k < 4; ++k) a.pose[k] = p[3 + k];
        for (int k = 0; k < 4; ++k) a.submap_pose[k] = sp[3 + k];
      } else {
        for (int k = 0; k < 7; ++k) a.pose[k] = p[k];
        for (int k = 0; k < 7; ++k) a.submap_pose[k] = sp[k];
      }
      a.node_data = in.matcher->Data(*in.constant_data);
      a.histogram_size = in.matcher->histogram_size_;
      a.min_score = in.min_score;
    }
    std::vector<dliom_fast_csm_result> r(count);
    std::vector<int> statuses(count);
    Check(dliom_fast_csm_match_batch(Context::ForThisThread(device)->get(), q.data(), count, r.data(), statuses.data(), stats),
          "FastCorrelativeScanMatcher3D::MatchBatch");
    found->assign(count, false);
    results->resize(count);
    for (int i = 0; i < count; ++i) {
      Check(statuses[i], "FastCorrelativeScanMatcher3D::MatchBatch");
      (*found)[i] = Store(r[i], &(*results)[i]);
    }
  }

 private:
  dliom_fast_csm_node_data Data(const TrajectoryNodeData& c) const {
    if (static_cast<int>(c.rotational_scan_matcher_histogram.size()) != histogram_size_)
      Check(DLIOM_ERR_INVALID_ARGUMENT, "rotational_scan_matcher_histogram size");
    dliom_fast_csm_node_data d;
    for (int i = 0; i < 4; ++i) d.gravity_alignment[i] = c.gravity_alignment.wxyz[i];
    d.high_resolution_points = c.high_resolution_point_cloud.empty() ? nullptr : &c.high_resolution_point_cloud[0].x;
    d.num_high_resolution_points = static_cast<int64_t>(c.high_resolution_point_cloud.size());
    d.low_resolution_points = c.low_resolution_point_cloud.empty() ? nullptr : &c.low_resolution_point_cloud[0].x;
    d.num_low_resolution_points = static_cast<int64_t>(c.low_resolution_point_cloud.size());
    d.rotational_scan_matcher_histogram = c.rotational_scan_matcher_histogram.data();
    return d;
  }
  static bool Store(const dliom_fast_csm_result& r, Result* result) {
    if (!r.found) return false;
    result->score = r.score;
    result->pose_estimate = transform::Rigid3d::FromArray(r.pose_estimate);
    result->rotational_score = r.rotational_score;
    result->low_resolution_score = r.low_resolution_score;
    return true;
  }
  dliom_fast_csm* matcher_ = nullptr;
  int histogram_size_ = 0;
  int device_ = 0;
};

// ConstraintBuilder3D::ComputeConstraint's three stages (mapping/internal/constraints/constraint_builder_3d.cc:202-334)
// for a whole list of (submap B, node) pairs: 1. the fast estimate, 2. no constraint when it finds nothing ("prune"),
// 3. CeresScanMatcher3D::Match with target = the match's translation, initial = the match's pose and the clouds
// {node high resolution, B's high resolution grid}, {node low resolution, B's low resolution grid}.  Two calls into
// the library for the whole list.  The policy lives here so that callers do not restate it.
struct ConstraintQuery {
  FastCorrelativeScanMatcher3D::Query search;  // search.matcher is B's matcher
  const HybridGrid* high_resolution_grid;      // B's grids
  const HybridGrid* low_resolution_grid;
};
struct ComputedConstraint {
  bool found = false;                          // false: no constraint (the reference's early return)
  FastCorrelativeScanMatcher3D::Result match;  // score, rotational and low-resolution score (the metrics at :296-302)
  transform::Rigid3d pose;                     // the refined constraint transform (submap B <- node)
};
inline std::vector<ComputedConstraint> ComputeConstraints(const CeresScanMatcher3D& ceres_scan_matcher,
                                                          const std::vector<ConstraintQuery>& queries,
                                                          dliom_batch_stats* fast_stats = nullptr,
                                                          dliom_batch_stats* ceres_stats = nullptr) {
  std::vector<FastCorrelativeScanMatcher3D::Query> searches;
  for (const ConstraintQuery& q : queries) searches.push_back(q.search);
  std::vector<bool> found;
  std::vector<FastCorrelativeScanMatcher3D::Result> matches;
  FastCorrelativeScanMatcher3D::MatchBatch(searches, &found, &matches, fast_stats);
  std::vector<ComputedConstraint> out(queries.size());
  std::vector<CeresScanMatcher3D::Problem> problems;
  std::vector<size_t> index;
  for (size_t i = 0; i < queries.size(); ++i) {
    if (!found[i]) continue;
    out[i].found = true;
    out[i].match = matches[i];
    const TrajectoryNodeData& d = *queries[i].search.constant_data;
    problems.push_back(CeresScanMatcher3D::Problem{
        matches[i].pose_estimate.translation(), matches[i].pose_estimate,
        {{&d.high_resolution_point_cloud, queries[i].high_resolution_grid},
         {&d.low_resolution_point_cloud, queries[i].low_resolution_grid}}});
    index.push_back(i);
  }
  std::vector<transform::Rigid3d> poses;
  std::vector<Summary> unused_summaries;
  ceres_scan_matcher.MatchBatch(problems, &poses, &unused_summaries, ceres_stats);
  for (size_t k = 0; k < index.size(); ++k) out[index[k]].pose = poses[k];
  return out;
}

}  // namespace scan_matching

// ---- sensor data of the LocalTrajectoryBuilder3D surface (sensor/timed_point_cloud_data.h, sensor/imu_data.h) ----
}  // namespace mapping
namespace sensor {
struct TimedPoint {
  float x, y, z, t;  // Eigen::Vector4f: position and time relative to TimedPointCloudData::time (<= 0)
};
using TimedPointCloud = std::vector<TimedPoint>;
struct TimedPointCloudData {
  int64_t time;  // common::Time ticks (100 ns): when the last point was acquired
  Vector3f origin;
  TimedPointCloud ranges;
};
struct ImuData {
  int64_t time;
  double linear_acceleration[3];
  double angular_velocity[3];
};
struct FixedFramePoseData {  // sensor/fixed_frame_pose_data.h:32-35 (GPS): a sample may come without a pose
  int64_t time;
  common::optional<transform::Rigid3d> pose;
};
struct OdometryData {
  int64_t time;
  transform::Rigid3d pose;
};
// TimedPointCloudOriginData (sensor/timed_point_cloud_data.h:37-46)
struct TimedPointCloudOriginData {
  struct RangeMeasurement {
    TimedPoint point_time;
    size_t origin_index;
  };
  int64_t time = 0;
  std::vector<Vector3f> origins;
  std::vector<RangeMeasurement> ranges;
};
}  // namespace sensor

// ---- sensor_msgs/PointCloud2, decoded on the device (dliom.h "PointCloud2 messages decoded on the device") ----------------
// The message as plain data, shaped like the ROS type: a caller with ROS copies nothing but the header fields (data may be
// moved or swapped in).  Parity of the decoding is unpinned against PCL: dliom.h states it.
namespace sensor_msgs {
struct PointField {
  std::string name;
  uint32_t offset = 0;
  uint8_t datatype = 0;  // INT8 = 1 ... FLOAT64 = 8
  uint32_t count = 1;
};
struct PointCloud2 {
  struct {
    struct {
      uint32_t sec = 0, nsec = 0;
    } stamp;
    std::string frame_id;
  } header;
  uint32_t height = 0, width = 0;
  std::vector<PointField> fields;
  bool is_bigendian = false;
  uint32_t point_step = 0, row_step = 0;
  std::vector<uint8_t> data;
};
}  // namespace sensor_msgs
namespace sensor {
// A decoded message in HBM: packed (x, y, z, t) and, from the export modes, one intensity a point.
class TimedCloudOnDevice {
 public:
  // mode: DLIOM_POINT_CLOUD2_*; sensor_to_tracking null: the points stay in the sensor frame (the export's way)
  TimedCloudOnDevice(Context* context, const sensor_msgs::PointCloud2& msg, int mode, const transform::Rigid3d* sensor_to_tracking)
      : context_(context), column_times_(mode != DLIOM_POINT_CLOUD2_SLAM_VELODYNE && mode != DLIOM_POINT_CLOUD2_SLAM_ROBOSENSE) {
    std::vector<dliom_point_field> fields(msg.fields.size());
    for (size_t k = 0; k < fields.size(); ++k)
      fields[k] = dliom_point_field{msg.fields[k].name.c_str(), msg.fields[k].offset, msg.fields[k].datatype, msg.fields[k].count};
    dliom_point_cloud2 m{};
    m.height = msg.height;
    m.width = msg.width;
    m.point_step = msg.point_step;
    m.row_step = msg.row_step;
    m.is_bigendian = msg.is_bigendian ? 1u : 0u;
    m.num_fields = static_cast<int32_t>(fields.size());
    m.fields = fields.data();
    m.data = msg.data.data();
    m.data_size = msg.data.size();
    m.stamp_sec = msg.header.stamp.sec;
    m.stamp_nsec = msg.header.stamp.nsec;
    std::array<double, 7> mount{};
    if (sensor_to_tracking != nullptr) mount = sensor_to_tracking->ToArray();
    float origin[3];
    Check(dliom_point_cloud2_decode(context->get(), &m, mode, sensor_to_tracking != nullptr ? mount.data() : nullptr, &cloud_, &time_,
                                    origin),
          "dliom_point_cloud2_decode");
    origin_ = Vector3f(origin[0], origin[1], origin[2]);
  }
  // takes over an object the library made (dliom_timed_cloud_stamp, dliom_timed_clouds_merge)
  TimedCloudOnDevice(Context* context, dliom_timed_cloud* adopted, int64_t time, const Vector3f& origin, bool column_times)
      : context_(context), cloud_(adopted), time_(time), origin_(origin), column_times_(column_times) {}
  ~TimedCloudOnDevice() {
    if (cloud_ != nullptr) dliom_timed_cloud_destroy(cloud_);
  }
  TimedCloudOnDevice(const TimedCloudOnDevice&) = delete;
  TimedCloudOnDevice& operator=(const TimedCloudOnDevice&) = delete;
  // (moved from: an object without a cloud, good for nothing but its destructor)
  TimedCloudOnDevice(TimedCloudOnDevice&& other)
      : context_(other.context_), cloud_(other.cloud_), time_(other.time_), origin_(other.origin_), column_times_(other.column_times_) {
    other.cloud_ = nullptr;
  }
  // true: many points share a time -- an Ouster's one time a column (64 or 128 points), a cloud without point times.
  // A merge of such a cloud replays std::sort's partitions on every run of equal times (RangeDataSynchronizer).
  bool column_times() const { return column_times_; }
  const dliom_timed_cloud* get() const { return cloud_; }
  Context* context() const { return context_; }
  int64_t time() const { return time_; }  // the stamp HandleRangefinder gets: the last point's
  const Vector3f& origin() const { return origin_; }
  size_t size() const {
    int64_t n = 0;
    Check(dliom_timed_cloud_size(cloud_, &n), "dliom_timed_cloud_size");
    return static_cast<size_t>(n);
  }
  // t of the last kept point, without a download (0 for an empty cloud)
  float back_time() const {
    float front = 0.f, back = 0.f;
    Check(dliom_timed_cloud_front_back_time(cloud_, &front, &back), "dliom_timed_cloud_front_back_time");
    return back;
  }
  float front_time() const {
    float front = 0.f, back = 0.f;
    Check(dliom_timed_cloud_front_back_time(cloud_, &front, &back), "dliom_timed_cloud_front_back_time");
    return front;
  }
  // StampRangeData on the device: a new object with this one's stamp and origin
  std::shared_ptr<const TimedCloudOnDevice> Stamped(double scan_period) const {
    dliom_timed_cloud* stamped = nullptr;
    Check(dliom_timed_cloud_stamp(context_->get(), cloud_, scan_period, &stamped), "dliom_timed_cloud_stamp");
    return std::make_shared<const TimedCloudOnDevice>(context_, stamped, time_, origin_, false);
  }
  // what the general host paths go on with
  TimedPointCloudData Download() const {
    TimedPointCloudData data{time_, origin_, TimedPointCloud(size())};
    static_assert(sizeof(TimedPoint) == 16, "packed x, y, z, t");
    ++Downloads();
    Check(dliom_timed_cloud_download(cloud_, data.ranges.empty() ? nullptr : &data.ranges[0].x, nullptr), "dliom_timed_cloud_download");
    return data;
  }
  // Download() calls of this process so far: what a caller who set up a device-only path checks it against
  static std::atomic<int64_t>& Downloads() {
    static std::atomic<int64_t> count(0);
    return count;
  }

 private:
  Context* context_;
  dliom_timed_cloud* cloud_ = nullptr;
  int64_t time_ = 0;
  Vector3f origin_;
  bool column_times_ = false;
};
}  // namespace sensor
namespace mapping {

// Host logic restated from mapping/internal/3d/range_data_synchronizer.cc:29-130: the prior lidar's cloud is passed
// on, with the part of a secondary lidar's cloud that overlaps it in time merged in (second origin, times re-based,
// ranges sorted by time).  `descrew` stamps the ranges linearly over the scan period (StampRangeData, :115-130).
class RangeDataSynchronizer {
 public:
  explicit RangeDataSynchronizer(const std::vector<std::string>& expected_range_sensor_ids)
      : expected_sensor_ids_(expected_range_sensor_ids.begin(), expected_range_sensor_ids.end()),
        prior_sensor_id_(expected_range_sensor_ids.empty() ? std::string() : expected_range_sensor_ids.front()) {}

  // true: `sensor_id` is the only expected range sensor (no secondary cloud can be pending)
  bool SingleSensor(const std::string& sensor_id) const {
    return expected_sensor_ids_.size() == 1 && sensor_id == prior_sensor_id_ && secondary_cloud_.empty() &&
           secondary_on_device_.empty();
  }
  // The same on decoded messages that stay in HBM (dliom.h "Two range sensors' clouds merged on the device"): the
  // decisions below are the host overload's, taken from the stamps and first times the objects carry; stamping and the
  // merge are the library's.  The pending secondary clouds are kept as device objects, so one synchronizer is fed either
  // through this overload or through the host one, not both.
  struct OnDevice {
    int64_t time = 0;
    std::vector<sensor::Vector3f> origins;
    std::shared_ptr<const sensor::TimedCloudOnDevice> ranges;  // null: nothing yet (a secondary cloud was queued)
    // this scan was merged by the host overload from downloads and `host` holds the result: the device merge refused it
    // (DLIOM_ERR_CAPACITY: device_refused), or it was not asked (max_column_time_points)
    bool merged_on_host = false, device_refused = false;
    sensor::TimedPointCloudOriginData host;
  };
  // max_column_time_points: where the prior cloud or the pending one has column times (TimedCloudOnDevice::column_times),
  // primary + secondary points above which the merge is left to the host overload (< 0: never)
  OnDevice AddRangeData(const std::string& sensor_id, const std::shared_ptr<const sensor::TimedCloudOnDevice>& data, bool descrew,
                        int64_t max_column_time_points = -1) {
    if (expected_sensor_ids_.count(sensor_id) == 0)
      Check(DLIOM_ERR_INVALID_ARGUMENT, "CHECK_NE(expected_sensor_ids_.count(sensor_id), 0)");
    OnDevice result;
    const std::shared_ptr<const sensor::TimedCloudOnDevice> cloud = descrew ? data->Stamped(0.1) : data;
    if (sensor_id != prior_sensor_id_) {
      secondary_on_device_.push_back(cloud);
      return result;
    }
    const double current_end = Seconds(cloud->time());
    const double current_start = cloud->size() == 0 ? current_end : current_end + cloud->front_time();
    while (!secondary_on_device_.empty() && Seconds(secondary_on_device_.front()->time()) < current_start)
      secondary_on_device_.pop_front();
    result.time = cloud->time();
    if (secondary_on_device_.empty() || secondary_on_device_.front()->size() == 0 ||
        Seconds(secondary_on_device_.front()->time()) + secondary_on_device_.front()->front_time() > current_end) {
      result.origins.assign(1, cloud->origin());
      result.ranges = cloud;
      return result;
    }
    const sensor::TimedCloudOnDevice& sec = *secondary_on_device_.front();
    dliom_timed_cloud* merged = nullptr;
    int status = DLIOM_ERR_CAPACITY;
    const bool ask = max_column_time_points < 0 || !(data->column_times() || sec.column_times()) ||
                     static_cast<int64_t>(data->size() + sec.size()) <= max_column_time_points;
    if (ask)
      status = dliom_timed_clouds_merge(data->context()->get(), data->get(), descrew ? cloud->get() : nullptr, cloud->time(), sec.get(),
                                        sec.time(), &merged);
    if (status == DLIOM_ERR_CAPACITY) {
      result.device_refused = ask;
      // this scan the host's way: the pending cloud (stamped already) and the prior one come down, the host overload merges
      secondary_cloud_.assign(1, sec.Download());
      try {
        result.host = AddRangeData(sensor_id, data->Download(), descrew);
      } catch (...) {
        secondary_cloud_.clear();
        throw;
      }
      secondary_cloud_.clear();
      result.merged_on_host = true;
      return result;
    }
    Check(status, "dliom_timed_clouds_merge (CHECK(i_start != -1) range_data_synchronizer.cc:84)");
    result.origins.push_back(cloud->origin());
    result.origins.push_back(sec.origin());
    result.ranges = std::make_shared<const sensor::TimedCloudOnDevice>(data->context(), merged, cloud->time(), cloud->origin(),
                                                                       data->column_times() || sec.column_times());
    return result;
  }
  sensor::TimedPointCloudOriginData AddRangeData(const std::string& sensor_id, const sensor::TimedPointCloudData& data,
                                                 bool descrew) {
    if (expected_sensor_ids_.count(sensor_id) == 0)
      Check(DLIOM_ERR_INVALID_ARGUMENT, "CHECK_NE(expected_sensor_ids_.count(sensor_id), 0)");
    sensor::TimedPointCloudOriginData result;
    sensor::TimedPointCloudData cloud = data;
    if (descrew) StampRangeData(&cloud, 0.1);
    if (sensor_id != prior_sensor_id_) {
      secondary_cloud_.push_back(cloud);
      return result;
    }
    const double current_end = Seconds(cloud.time);
    const double current_start = cloud.ranges.empty() ? current_end : current_end + cloud.ranges.front().t;
    while (!secondary_cloud_.empty() && Seconds(secondary_cloud_.front().time) < current_start) secondary_cloud_.pop_front();
    if (secondary_cloud_.empty() || secondary_cloud_.front().ranges.empty() ||
        Seconds(secondary_cloud_.front().time) + secondary_cloud_.front().ranges.front().t > current_end) {
      ToOriginData(cloud, &result);  // no secondary cloud, or "the secondary lidar may be too fast"
      return result;
    }
    const sensor::TimedPointCloudData& sec = secondary_cloud_.front();
    const double sec_time = Seconds(sec.time);
    int i_start = -1, i_end = -1;
    for (int i = 0; i < static_cast<int>(sec.ranges.size()); ++i) {
      const double t = sec_time + sec.ranges[i].t;
      if (t >= current_start && t <= current_end && i_start == -1) i_start = i;
      if (i_start != -1 && t > current_end) {
        i_end = i - 1;
        break;
      }
    }
    if (i_start == -1) Check(DLIOM_ERR_INVALID_ARGUMENT, "CHECK(i_start != -1) range_data_synchronizer.cc:84");
    if (i_end == -1) i_end = static_cast<int>(sec.ranges.size()) - 1;
    result.time = cloud.time;
    result.origins.push_back(cloud.origin);
    for (const sensor::TimedPoint& p : data.ranges) result.ranges.push_back({p, 0});  // the UNSTAMPED input, as :97
    result.origins.push_back(sec.origin);
    for (int i = i_start; i <= i_end; ++i) {
      sensor::TimedPoint p = sec.ranges[i];
      p.t = static_cast<float>(static_cast<double>(sec.ranges[i].t) + sec_time - current_end);
      result.ranges.push_back({p, 1});
    }
    std::sort(result.ranges.begin(), result.ranges.end(),
              [](const sensor::TimedPointCloudOriginData::RangeMeasurement& a,
                 const sensor::TimedPointCloudOriginData::RangeMeasurement& b) { return a.point_time.t < b.point_time.t; });
    return result;
  }

 private:
  // common::ToSecondsStamp (common/time.cc:48-56), operation by operation: universal-time ticks (100 ns since 0001-01-01)
  // minus the Unix epoch, in nanoseconds as an integer, times 1e-9.  (ticks * 1e-7 on raw ~6.3e17 ticks would round
  // to 12.8 us; this resolves ~0.25 us like the reference and picks the same overlap indices.)
  static double Seconds(int64_t ticks) {
    constexpr int64_t kUtsEpochOffsetFromUnixEpochInSeconds = 719162ll * 24ll * 60ll * 60ll;  // common/time.h:29-30
    const int64_t ns_since_unix_epoch = (ticks - kUtsEpochOffsetFromUnixEpochInSeconds * 10000000ll) * 100ll;
    return static_cast<double>(ns_since_unix_epoch) * 1e-9;
  }
  static void ToOriginData(const sensor::TimedPointCloudData& c, sensor::TimedPointCloudOriginData* out) {
    out->time = c.time;
    out->origins.assign(1, c.origin);
    out->ranges.clear();
    for (const sensor::TimedPoint& p : c.ranges) out->ranges.push_back({p, 0});
  }
  static void StampRangeData(sensor::TimedPointCloudData* cloud, double scan_period) {
    const int n = static_cast<int>(cloud->ranges.size());
    if (n < 2) return;
    const double duration = scan_period / (n - 1);
    for (int i = 0; i < n; ++i) cloud->ranges[i].t = static_cast<float>(-scan_period + i * duration);
    cloud->ranges.back().t = 0.f;
  }
  std::set<std::string> expected_sensor_ids_;
  std::string prior_sensor_id_;
  std::deque<sensor::TimedPointCloudData> secondary_cloud_;
  std::deque<std::shared_ptr<const sensor::TimedCloudOnDevice>> secondary_on_device_;
};

// proto::LocalTrajectoryBuilderOptions3D: the front end's options plus the AddRangeData / IMU fields
struct LocalTrajectoryBuilderOptions3D {
  // The IMU options start from the library's defaults (trajectory_builder_3d.lua's imu block): a caller overrides fields,
  // it never has to know every field -- a struct filled by hand would leave fields added later (round 4:
  // imu.tangent_preintegration, which selects the integrator) indeterminate, and dliom_imu_window_create refuses those.
  LocalTrajectoryBuilderOptions3D() : front_end() {
    dliom_imu_window_default_options(&imu);
    imu.graph_reset_every = -1;  // like the reference: reset at submaps.num_range_data, every key kept until then
  }
  dliom_front_end_options front_end;     // adaptive filters, matchers, motion filter, submaps (the caller fills it: no defaults)
  dliom_imu_window_options imu;          // imu block + WindowOptimize; imu.graph_reset_every < 0: follow
                                         // front_end.num_range_data like the reference (.cc:750), 0: never reset
  bool keep_imu_window_size = false;     // false: graph reset on => imu.window_size = 0 (the reference's rule: every key
                                         // until the reset); true: the fixed-lag smoother of imu.window_size states
  float min_range = 1.f, max_range = 100.f;
  int num_accumulated_range_data = 1;
  float voxel_filter_size = 0.15f;
  double scan_period = 0.1;
  bool enable_manual_descrew = false;    // eable_mannually_discrew_
  int rotational_histogram_size = 120;   // trajectory_builder_3d.lua: rotational_histogram_size
  // The initialisation (.cc:164-176, 203-330, 372-381).  false, the default: the state comes from SetInitialState() and
  // everything before it is dropped.  true: the builder initialises itself from its first messages as the reference does
  // -- InitilizeByNDT if enable_ndt_initialization, else InitializeStatic -- and every call returns nullptr until then.
  bool internal_initialization = false;
  bool enable_ndt_initialization = false;
  int frames_for_dynamic_initialization = 7;
  int frames_for_static_initialization = 7;
  transform::Rigid3d transform_lb;       // AlignWithWorld's T_lb (identity)
};

// proto::SubmapQuery::Response (mapping/proto/submap_visualization.proto) as plain structs.  `cells` is the texture's
// UNCOMPRESSED (value, alpha) bytes: the caller applies common::FastGzipString before it sets the proto field.
struct SubmapTexture {
  std::string cells;
  int width = 0;
  int height = 0;
  double resolution = 0.;
  transform::Rigid3d slice_pose;
};
struct SubmapQueryResponse {
  int submap_version = 0;
  std::vector<SubmapTexture> textures;  // high resolution, then low resolution
};

// AddToTextureProto (mapping/3d/submap_3d.cc:53-177) for one grid, without the gzip step (dliom_grid_xray_texture).
inline SubmapTexture XrayTexture(const dliom_grid* grid, const transform::Rigid3d& global_submap_pose) {
  const std::array<double, 7> pose = global_submap_pose.ToArray();
  SubmapTexture t;
  int32_t w = 0, h = 0;
  double slice[7];
  Check(dliom_grid_xray_texture(grid, pose.data(), nullptr, 0, &w, &h, &t.resolution, slice), "dliom_grid_xray_texture");
  t.cells.resize(static_cast<size_t>(w) * h * 2);
  if (!t.cells.empty())
    Check(dliom_grid_xray_texture(grid, pose.data(), reinterpret_cast<uint8_t*>(&t.cells[0]), static_cast<int64_t>(t.cells.size()),
                                  &w, &h, &t.resolution, slice), "dliom_grid_xray_texture");
  t.width = w;
  t.height = h;
  t.slice_pose = transform::Rigid3d::FromArray(slice);
  return t;
}

// AddToTextureProto with its gzip step on the device (dliom_grid_xray_texture_gzip): `cells` is what the proto field takes.
inline SubmapTexture XrayTextureGzipped(const dliom_grid* grid, const transform::Rigid3d& global_submap_pose) {
  const std::array<double, 7> pose = global_submap_pose.ToArray();
  SubmapTexture t;
  int32_t w = 0, h = 0;
  int64_t size = 0;
  double slice[7];
  Check(dliom_grid_xray_texture_gzip(grid, pose.data(), nullptr, 0, &size, &w, &h, &t.resolution, slice, nullptr), "dliom_grid_xray_texture_gzip");
  t.cells.resize(static_cast<size_t>(size));
  Check(dliom_grid_xray_texture_gzip(grid, pose.data(), reinterpret_cast<uint8_t*>(&t.cells[0]), size, &size, &w, &h, &t.resolution, slice,
                                     nullptr), "dliom_grid_xray_texture_gzip");
  t.cells.resize(static_cast<size_t>(size));
  t.width = w;
  t.height = h;
  t.slice_pose = transform::Rigid3d::FromArray(slice);
  return t;
}

// ProjectToCvMat's image (D-LIOM mapping/3d/submap_3d.cc:381-443) without OpenCV: `data` is rows x cols CV_8UC1,
// row-major -- cv::Mat(rows, cols, CV_8UC1, data.data()) wraps it.  Pixel values are the reference's, reduced modulo 256
// (empty pixels 224); an empty projection is 0 x 0.
struct ProjectedImage {
  int rows = 0;
  int cols = 0;
  std::vector<uint8_t> data;
};

// A submap of the active pair; the grids stay owned by the front end (borrowed handles).
class Submap3D {
 public:
  Submap3D(const transform::Rigid3d& local_pose, int num_range_data, bool finished, dliom_grid* hi, dliom_grid* lo)
      : local_pose_(local_pose), num_range_data_(num_range_data), finished_(finished), hi_(hi), lo_(lo) {}
  const transform::Rigid3d& local_pose() const { return local_pose_; }
  int num_range_data() const { return num_range_data_; }
  bool finished() const { return finished_; }
  dliom_grid* high_resolution_hybrid_grid() const { return hi_; }
  dliom_grid* low_resolution_hybrid_grid() const { return lo_; }
  // Submap3D::ToProto(proto::Submap*, include_probability_grid_data) (mapping/3d/submap_3d.cc:217-230) as the
  // serialized bytes of proto::Submap{submap_3d}: proto.ParseFromString(submap.ToProtoBytes(true)) on the caller's side.
  std::string ToProtoBytes(bool include_probability_grid_data) const {
    std::string grids[2];
    if (include_probability_grid_data) {
      dliom_grid* const g[2] = {hi_, lo_};
      for (int k = 0; k < 2; ++k) {
        int64_t n = 0;
        Check(dliom_grid_to_proto(g[k], nullptr, 0, &n), "dliom_grid_to_proto");
        grids[k].resize(static_cast<size_t>(n));
        Check(dliom_grid_to_proto(g[k], reinterpret_cast<uint8_t*>(&grids[k][0]), n, &n), "dliom_grid_to_proto");
      }
    }
    const uint8_t dummy = 0;
    auto ptr = [&](const std::string& b) {
      return include_probability_grid_data ? (b.empty() ? &dummy : reinterpret_cast<const uint8_t*>(b.data())) : nullptr;
    };
    const std::array<double, 7> pose = local_pose_.ToArray();
    int64_t n = 0;
    Check(dliom_submap3d_to_proto(pose.data(), num_range_data_, finished_ ? 1 : 0, ptr(grids[0]),
                                  static_cast<int64_t>(grids[0].size()), ptr(grids[1]), static_cast<int64_t>(grids[1].size()), 1,
                                  nullptr, 0, &n), "dliom_submap3d_to_proto");
    std::string out(static_cast<size_t>(n), '\0');
    Check(dliom_submap3d_to_proto(pose.data(), num_range_data_, finished_ ? 1 : 0, ptr(grids[0]),
                                  static_cast<int64_t>(grids[0].size()), ptr(grids[1]), static_cast<int64_t>(grids[1].size()), 1,
                                  reinterpret_cast<uint8_t*>(&out[0]), n, &n), "dliom_submap3d_to_proto");
    return out;
  }
  // Submap3D::ToResponseProto (submap_3d.cc:253-262): submap_version = num_range_data, then one X-ray texture per grid,
  // computed on the device.  The textures' cells are uncompressed (see SubmapTexture).
  SubmapQueryResponse ToResponseProto(const transform::Rigid3d& global_submap_pose) const {
    SubmapQueryResponse r;
    r.submap_version = num_range_data_;
    r.textures.push_back(XrayTexture(hi_, global_submap_pose));
    r.textures.push_back(XrayTexture(lo_, global_submap_pose));
    return r;
  }
  // ... with the textures' cells gzipped on the device, ready for the proto (dliom::kGzipped); opt-in
  SubmapQueryResponse ToResponseProto(const transform::Rigid3d& global_submap_pose, GzipTag) const {
    SubmapQueryResponse r;
    r.submap_version = num_range_data_;
    r.textures.push_back(XrayTextureGzipped(hi_, global_submap_pose));
    r.textures.push_back(XrayTextureGzipped(lo_, global_submap_pose));
    return r;
  }

 private:
  transform::Rigid3d local_pose_;
  int num_range_data_;
  bool finished_;
  dliom_grid* hi_;
  dliom_grid* lo_;
};

// ProjectToCvMat(hybrid_grid, transform, ox, oy, resolution) (submap_3d.cc:381-443) on the device
// (dliom_grid_project_to_image); the caller wraps the result in a cv::Mat, see ProjectedImage.
inline ProjectedImage ProjectToCvMat(const dliom_grid* hybrid_grid, const transform::Rigid3d& transform, double& ox,
                                     double& oy, double& resolution) {
  const std::array<double, 7> pose = transform.ToArray();
  ProjectedImage img;
  int32_t w = 0, h = 0;
  Check(dliom_grid_project_to_image(hybrid_grid, pose.data(), nullptr, 0, &w, &h, &ox, &oy, &resolution),
        "dliom_grid_project_to_image");
  img.data.resize(static_cast<size_t>(w) * h);
  if (!img.data.empty())
    Check(dliom_grid_project_to_image(hybrid_grid, pose.data(), img.data.data(), static_cast<int64_t>(img.data.size()), &w, &h,
                                      &ox, &oy, &resolution), "dliom_grid_project_to_image");
  img.rows = h;
  img.cols = w;
  return img;
}

// ActiveSubmaps3D (mapping/3d/submap_3d.h:95-122) over the front end's submap pair.
class ActiveSubmaps3D {
 public:
  ActiveSubmaps3D(Context* context, const dliom_front_end_options& options) : context_(context) {
    Check(dliom_front_end_create(context->get(), &options, &fe_), "dliom_front_end_create");
  }
  ~ActiveSubmaps3D() { dliom_front_end_destroy(fe_); }
  ActiveSubmaps3D(const ActiveSubmaps3D&) = delete;
  ActiveSubmaps3D& operator=(const ActiveSubmaps3D&) = delete;

  int matching_index() const {
    int i = 0;
    Check(dliom_front_end_matching_index(fe_, &i), "ActiveSubmaps3D::matching_index");
    return i;
  }
  void InsertRangeData(const sensor::RangeData& range_data, const transform::Quaterniond& gravity_alignment) {
    dliom_cloud* cloud = nullptr;
    Check(dliom_cloud_create(context_->get(), range_data.returns.empty() ? nullptr : &range_data.returns[0].x,
                             static_cast<int64_t>(range_data.returns.size()), &cloud),
          "ActiveSubmaps3D::InsertRangeData (upload)");
    dliom_insertion_result r;
    Check(dliom_front_end_insert_range_data(fe_, &range_data.origin.x, cloud, gravity_alignment.wxyz, &r),
          "ActiveSubmaps3D::InsertRangeData");
    dliom_cloud_destroy(cloud);
  }
  std::vector<std::shared_ptr<Submap3D>> submaps() const {
    int n = 0;
    Check(dliom_front_end_num_active_submaps(fe_, &n), "ActiveSubmaps3D::submaps");
    std::vector<std::shared_ptr<Submap3D>> out;
    for (int i = 0; i < n; ++i) {
      double pose[7];
      int num = 0, fin = 0;
      dliom_grid *hi = nullptr, *lo = nullptr;
      Check(dliom_front_end_active_submap(fe_, i, pose, &num, &fin, &hi, &lo), "ActiveSubmaps3D::submaps");
      out.push_back(std::make_shared<Submap3D>(transform::Rigid3d::FromArray(pose), num, fin != 0, hi, lo));
    }
    return out;
  }
  dliom_front_end* get() const { return fe_; }

 private:
  Context* context_;
  dliom_front_end* fe_ = nullptr;
};

// LocalTrajectoryBuilder3D (mapping/internal/3d/local_trajectory_builder_3d.h:83-111).  By default the state after the
// reference's IMU-lidar initialisation is supplied through SetInitialState() and everything before it is dropped; with
// options.internal_initialization the builder is fed from its first message and initialises itself as the reference does
// (InitializeStatic, or InitilizeByNDT with AlignWithWorld: DESIGN 3.24).  AddOdometryData is accepted and ignored like in
// the reference's D-LIOM path, whose extrapolator is never created (.cc:324-333).
class LocalTrajectoryBuilder3D {
 public:
  struct InsertionResult {
    int64_t time;
    transform::Quaterniond gravity_alignment;
    transform::Rigid3d local_pose;
    std::vector<int> insertion_submap_indices;  // trajectory-wide indices of the submaps inserted into
    bool submap_finished;                        // take it with dliom_front_end_take_finished_submap
    // TrajectoryNode::Data::rotational_scan_matcher_histogram (.cc:605-610): what the loop-closure matcher's
    // RotationalScanMatcher is built from (FastCorrelativeScanMatcher3D's `nodes`)
    std::vector<float> rotational_scan_matcher_histogram;
    // TrajectoryNode::Data::high_resolution_point_cloud / low_resolution_point_cloud (.cc:613-619): the adaptively
    // filtered clouds in the tracking frame, what ConstraintBuilder3D matches against finished submaps
    sensor::PointCloud high_resolution_point_cloud, low_resolution_point_cloud;
  };
  struct MatchingResult {
    int64_t time;
    transform::Rigid3d local_pose;
    sensor::RangeData range_data_in_local;
    std::unique_ptr<const InsertionResult> insertion_result;  // nullptr if dropped by the motion filter
    // the scan's index in the cache given to SetNodeCloudCache (-1: none): range_data_in_local's returns were kept there
    // straight from the device cloud, the bits of the host vector above
    int64_t node_cloud_index = -1;
  };
  // MapBuilderBridge::OnLocalSlamResult's keeping of every scan (-save_range_data, the map cloud), without the host vector's
  // round trip: each matched scan is added to `cache` (null: none, the default) by one kernel that nothing waits for.
  void SetNodeCloudCache(cartographer_ros::NodeCloudCache* cache, int trajectory_id) {
    node_cloud_cache_ = cache;
    node_cloud_trajectory_id_ = trajectory_id;
  }

  LocalTrajectoryBuilder3D(Context* context, const LocalTrajectoryBuilderOptions3D& options,
                           const std::vector<std::string>& expected_range_sensor_ids)
      : context_(context), options_(options), active_submaps_(context, options.front_end),
        synchronizer_(expected_range_sensor_ids) {
    dliom_imu_window_options imu = options.imu;
    if (imu.graph_reset_every < 0) imu.graph_reset_every = options.front_end.num_range_data >= 2 ? options.front_end.num_range_data : 0;
    // with the graph reset on, WindowOptimize follows the reference's rule: every key stays in the problem until the reset
    // (window_size 0; .cc:749-797), linearisation points move by ISAM2's threshold (imu.relinearize_threshold, 0.1).  A
    // caller who wants the fixed-lag smoother between resets sets imu.window_size and keep_imu_window_size.
    if (imu.graph_reset_every >= 2 && !options.keep_imu_window_size) imu.window_size = 0;
    Check(dliom_imu_window_create(&imu, &window_), "dliom_imu_window_create");
    Check(dliom_range_accumulator_create(context->get(), &accumulator_), "dliom_range_accumulator_create");
    if (options.internal_initialization && options.enable_ndt_initialization) {
      if (options.frames_for_dynamic_initialization < 1 || options.frames_for_dynamic_initialization + 1 > DLIOM_INIT_MAX_FRAMES)
        Check(DLIOM_ERR_INVALID_ARGUMENT, "frames_for_dynamic_initialization");
      const double zero[3] = {0., 0., 0.};
      const dliom_imu_noise noise{imu.acc_noise, imu.gyr_noise, imu.acc_bias_noise, imu.gyr_bias_noise};
      Check(dliom_imu_integrator_create(zero, zero, &noise, &init_integrator_), "dliom_imu_integrator_create");
      dliom_ndt_options ndt;
      Check(dliom_ndt_default_options(&ndt), "dliom_ndt_default_options");  // .cc:252-259: 0.01, 0.1, 1.0, 35
      Check(dliom_ndt_scan_matcher_create(context->get(), &ndt, 0.2f, &init_matcher_), "dliom_ndt_scan_matcher_create");
    }
  }
  ~LocalTrajectoryBuilder3D() {
    if (init_integrator_ != nullptr) dliom_imu_integrator_destroy(init_integrator_);
    dliom_ndt_scan_matcher_destroy(init_matcher_);
    dliom_range_accumulator_destroy(accumulator_);
    dliom_imu_window_destroy(window_);
  }
  LocalTrajectoryBuilder3D(const LocalTrajectoryBuilder3D&) = delete;
  LocalTrajectoryBuilder3D& operator=(const LocalTrajectoryBuilder3D&) = delete;

  // prev_state_ / prev_bias_ as InitializeIMU() leaves them (.cc:322-345)
  // start_graph: the reference starts its factor graph at the FIRST WindowOptimize call after InitializeIMU (.cc:712-745),
  // i.e. the first scan after the initialisation only starts the graph and is reported (and inserted) at the initial pose --
  // harmless on the platform at rest D-LIOM's static initialisation assumes, and what this adapter does by default.  true
  // starts the graph here instead: for a caller whose initial state IS the state at the time of the call (a replay that
  // begins in motion), so that the first scan is fused like every later one.
  void SetInitialState(const transform::Rigid3d& pose, const transform::Vector3d& velocity, const double bias6[6],
                       bool start_graph = false) {
    Check(dliom_imu_window_initialize(window_, pose.ToArray().data(), velocity.v, bias6), "dliom_imu_window_initialize");
    if (start_graph) {
      double p[7], v[3], b[6];
      Check(dliom_imu_window_window_optimize(window_, pose.ToArray().data(), 0, p, v, b), "WindowOptimize (graph start)");
    }
    last_imu_time_ = -1;
    imu_initialized_ = true;
    have_prediction_ = false;
    const std::array<double, 7> p = pose.ToArray();
    for (int k = 0; k < 7; ++k) initial_state_[k] = p[k];
    for (int k = 0; k < 3; ++k) initial_state_[7 + k] = velocity.v[k];
    for (int k = 0; k < 6; ++k) initial_state_[10 + k] = bias6[k];
  }
  // The state the last SetInitialState() took (what InitializeIMU starts from): pose7, velocity3, bias6.  false before it.
  bool InitialState(double state16[16]) const {
    if (!imu_initialized_) return false;
    for (int k = 0; k < 16; ++k) state16[k] = initial_state_[k];
    return true;
  }
  // InitilizeByNDT's frames held (buffered_scan_count_) and the AlignWithWorld calls that failed and started over
  int initialization_frames() const { return static_cast<int>(init_frames_.size()); }
  int64_t initialization_failures() const { return initialization_failures_; }
  void AddImuData(const sensor::ImuData& imu) {
    if (!imu_initialized_) {  // .cc:165-176; without internal_initialization the data is dropped
      if (!options_.internal_initialization) return;
      if (init_integrator_ != nullptr) {
        const double dt = last_imu_time_ini_ < 0 ? 1.0 / 500.0 : static_cast<double>(imu.time - last_imu_time_ini_) * 1e-7;
        last_imu_time_ini_ = imu.time;
        Check(dliom_imu_integrator_push_back(init_integrator_, dt, imu.linear_acceleration, imu.angular_velocity), "AddImuData (initialisation)");
      } else {
        init_imu_buffer_.push_back(imu);
      }
      return;
    }
    const double dt = last_imu_time_ < 0 ? 1.0 / 500.0 : static_cast<double>(imu.time - last_imu_time_) * 1e-7;  // .cc:183-185
    last_imu_time_ = imu.time;
    if (!(dt > 0)) return;
    Check(dliom_imu_window_add_imu(window_, imu.linear_acceleration, imu.angular_velocity, dt), "AddImuData");
    have_prediction_ = true;
  }
  void AddOdometryData(const sensor::OdometryData&) {}

  std::unique_ptr<MatchingResult> AddRangeData(const std::string& sensor_id, const sensor::TimedPointCloudData& unsynchronized) {
    // One range sensor, its own time stamps, one scan per result -- D-LIOM's configurations: the synchronizer would hand
    // the scan back as it came (range_data_synchronizer.cc: no secondary cloud -> ToOriginData) and the accumulation holds
    // one scan.  The scan goes to the device as it lies in the caller's vector (TimedPoint = packed x, y, z, t) and
    // AddRangeData is ONE library call; the copies the general path makes (the synchronizer's cloud, its origin-tagged
    // ranges, the packed staging vector: ~3 MB of host traffic and two reallocating push_back loops per 64 x 1024 scan)
    // were a quarter of the adapter's time per scan (round 6, tools/wref_cpp.cc).
    if (synchronizer_.SingleSensor(sensor_id) && !options_.enable_manual_descrew && options_.num_accumulated_range_data == 1) {
      if (!unsynchronized.ranges.empty() && !imu_initialized_)
        return Initialize(unsynchronized.time, [&] { return UploadPoints(&unsynchronized.ranges[0].x, 4, unsynchronized.ranges.size()); });
      if (unsynchronized.ranges.empty() || !imu_initialized_ || !have_prediction_) return nullptr;
      if (unsynchronized.ranges.back().t > 0.1f) Check(DLIOM_ERR_INVALID_ARGUMENT, "CHECK_LE(ranges.back().point_time[3], 0.1f)");
      static_assert(sizeof(sensor::TimedPoint) == 16, "packed x, y, z, t");
      DLIOM_ADAPTER_STAGE(0);  // since the last result: the caller, AddImuData
      double prev[7], vel[3], bias[6], predicted[7], pvel[3];
      Check(dliom_imu_window_state(window_, 0, prev, vel, bias), "dliom_imu_window_state");
      Check(dliom_imu_window_predict(window_, predicted, pvel), "dliom_imu_window_predict");
      accumulation_started_ = std::chrono::steady_clock::now();
      const float origin[3] = {unsynchronized.origin.x, unsynchronized.origin.y, unsynchronized.origin.z};
      dliom_cloud* cloud = nullptr;
      float origin_in_tracking[3], current_pose[7];
      Check(dliom_add_range_data(context_->get(), prev, predicted, options_.scan_period, &unsynchronized.ranges[0].x,
                                 static_cast<int64_t>(unsynchronized.ranges.size()), origin, options_.min_range, options_.max_range,
                                 options_.voxel_filter_size, &cloud, origin_in_tracking, current_pose),
            "AddRangeData (de-skew, filters, tracking frame)");
      DLIOM_ADAPTER_STAGE(1);
      return AddAccumulatedRangeData(unsynchronized.time, current_pose, origin_in_tracking, cloud);
    }
    return AddSynchronizedRangeData(synchronizer_.AddRangeData(sensor_id, unsynchronized, options_.enable_manual_descrew));
  }

 private:
  // the general host path behind the synchronizer: pack, upload, de-skew + accumulate
  std::unique_ptr<MatchingResult> AddSynchronizedRangeData(const sensor::TimedPointCloudOriginData& sync) {
    if (!sync.ranges.empty() && !imu_initialized_) {
      static_assert(sizeof(sensor::TimedPointCloudOriginData::RangeMeasurement) % sizeof(float) == 0, "a stride in floats");
      return Initialize(sync.time, [&] {
        return UploadPoints(&sync.ranges[0].point_time.x, sizeof(sensor::TimedPointCloudOriginData::RangeMeasurement) / sizeof(float),
                            sync.ranges.size());
      });
    }
    if (sync.ranges.empty() || !imu_initialized_ || !have_prediction_) return nullptr;
    if (sync.ranges.back().point_time.t > 0.1f) Check(DLIOM_ERR_INVALID_ARGUMENT, "CHECK_LE(ranges.back().point_time[3], 0.1f)");
    // prev_state_ and predicted_states_.back() (.cc:424-427)
    double prev[7], vel[3], bias[6], predicted[7], pvel[3];
    Check(dliom_imu_window_state(window_, 0, prev, vel, bias), "dliom_imu_window_state");
    Check(dliom_imu_window_predict(window_, predicted, pvel), "dliom_imu_window_predict");
    std::vector<float> xyzt(4 * sync.ranges.size()), index(sync.ranges.size()), origins(3 * sync.origins.size());
    for (size_t i = 0; i < sync.ranges.size(); ++i) {
      xyzt[4 * i] = sync.ranges[i].point_time.x;
      xyzt[4 * i + 1] = sync.ranges[i].point_time.y;
      xyzt[4 * i + 2] = sync.ranges[i].point_time.z;
      xyzt[4 * i + 3] = sync.ranges[i].point_time.t;
      index[i] = static_cast<float>(sync.ranges[i].origin_index);
    }
    for (size_t k = 0; k < sync.origins.size(); ++k) {
      origins[3 * k] = sync.origins[k].x;
      origins[3 * k + 1] = sync.origins[k].y;
      origins[3 * k + 2] = sync.origins[k].z;
    }
    float current_pose[7];
    int accumulated = 0;
    if (!accumulating_) {  // num_accumulated_ == 0 (.cc:389-391)
      accumulation_started_ = std::chrono::steady_clock::now();
      accumulating_ = true;
    }
    Check(dliom_range_accumulator_add(accumulator_, prev, predicted, options_.scan_period, xyzt.data(),
                                      sync.origins.size() > 1 ? index.data() : nullptr,
                                      static_cast<int64_t>(sync.ranges.size()), origins.data(),
                                      static_cast<int>(sync.origins.size()), options_.min_range, options_.max_range,
                                      options_.voxel_filter_size, current_pose, &accumulated),
          "AddRangeData (de-skew + accumulate)");
    if (accumulated < options_.num_accumulated_range_data) return nullptr;
    accumulating_ = false;
    dliom_cloud* cloud = nullptr;
    float origin_in_tracking[3];
    Check(dliom_range_accumulator_finish(accumulator_, options_.voxel_filter_size, &cloud, origin_in_tracking),
          "AddRangeData (voxel filter + tracking frame)");
    return AddAccumulatedRangeData(sync.time, current_pose, origin_in_tracking, cloud);
  }

 public:
  // The single-sensor path above on a message decoded on the device (SensorBridge::HandlePointCloud2Message): the ranges are
  // in HBM already, in the tracking frame, and stay there; the two checks on them read what the decode brought back.
  // Several sensors, manual de-skew and accumulation need an object they may keep (a secondary lidar's cloud waits for the
  // prior one's): from a caller who keeps his, they download the cloud and go on through the host synchronizer;
  // the overload below takes the object over and stays on the device.
  std::unique_ptr<MatchingResult> AddRangeData(const std::string& sensor_id, const sensor::TimedCloudOnDevice& ranges) {
    if (!FastPath(sensor_id)) return AddRangeData(sensor_id, ranges.Download());
    return AddSingleSensorRangeData(ranges);
  }
  // ... on an object handed over.  Several sensors, manual de-skew or accumulation: the synchronizer's device overload
  // (stamp, merge and std::sort's order on the device) and the accumulator's device input, without a download.  A merge the
  // device refuses (DLIOM_ERR_CAPACITY: an arrangement of equal times the sort's replay does not take) goes the host's way
  // for that scan and is counted (merge_host_fallbacks()); so does, counted apart (merges_left_to_host()), a merge of
  // clouds with column times above kMaxColumnTimePointsOnDevice.
  std::unique_ptr<MatchingResult> AddRangeData(const std::string& sensor_id, sensor::TimedCloudOnDevice&& ranges) {
    if (FastPath(sensor_id)) return AddSingleSensorRangeData(ranges);
    const RangeDataSynchronizer::OnDevice sync =
        synchronizer_.AddRangeData(sensor_id, std::make_shared<const sensor::TimedCloudOnDevice>(std::move(ranges)),
                                   options_.enable_manual_descrew, kMaxColumnTimePointsOnDevice);
    if (sync.merged_on_host) {
      ++(sync.device_refused ? merge_host_fallbacks_ : merges_left_to_host_);
      return AddSynchronizedRangeData(sync.host);
    }
    if (sync.origins.size() > 1) ++device_merges_;
    if (sync.ranges != nullptr && sync.ranges->size() != 0 && !imu_initialized_)
      return Initialize(sync.time, [&] { return DevicePoints(*sync.ranges); });
    if (sync.ranges == nullptr || sync.ranges->size() == 0 || !imu_initialized_ || !have_prediction_) return nullptr;
    if (sync.ranges->back_time() > 0.1f) Check(DLIOM_ERR_INVALID_ARGUMENT, "CHECK_LE(ranges.back().point_time[3], 0.1f)");
    double prev[7], vel[3], bias[6], predicted[7], pvel[3];
    Check(dliom_imu_window_state(window_, 0, prev, vel, bias), "dliom_imu_window_state");
    Check(dliom_imu_window_predict(window_, predicted, pvel), "dliom_imu_window_predict");
    std::vector<float> origins(3 * sync.origins.size());
    for (size_t k = 0; k < sync.origins.size(); ++k) {
      origins[3 * k] = sync.origins[k].x;
      origins[3 * k + 1] = sync.origins[k].y;
      origins[3 * k + 2] = sync.origins[k].z;
    }
    float current_pose[7];
    int accumulated = 0;
    if (!accumulating_) {
      accumulation_started_ = std::chrono::steady_clock::now();
      accumulating_ = true;
    }
    Check(dliom_range_accumulator_add_timed_cloud(accumulator_, prev, predicted, options_.scan_period, sync.ranges->get(), origins.data(),
                                                  static_cast<int>(sync.origins.size()), options_.min_range, options_.max_range,
                                                  options_.voxel_filter_size, current_pose, &accumulated),
          "AddRangeData (de-skew + accumulate)");
    if (accumulated < options_.num_accumulated_range_data) return nullptr;
    accumulating_ = false;
    dliom_cloud* cloud = nullptr;
    float origin_in_tracking[3];
    Check(dliom_range_accumulator_finish(accumulator_, options_.voxel_filter_size, &cloud, origin_in_tracking),
          "AddRangeData (voxel filter + tracking frame)");
    return AddAccumulatedRangeData(sync.time, current_pose, origin_in_tracking, cloud);
  }
  // scans whose merge the device refused and the host synchronizer served
  int64_t merge_host_fallbacks() const { return merge_host_fallbacks_; }
  // scans the synchronizer merged with a secondary lidar's on the device
  int64_t device_merges() const { return device_merges_; }
  // scans with column times (an Ouster's, a cloud without point times) whose merge was left to the host synchronizer
  int64_t merges_left_to_host() const { return merges_left_to_host_; }
  // Primary + secondary points up to which clouds with column times are merged on the device.  0: never -- the replay of
  // std::sort's partitions on runs of equal times is one workgroup's work and lost to download + host std::sort + upload
  // at every size measured, 0.25 ms against 0.19 ms at 768 merged points, 13.4 ms against 2.0 ms at 98 304 (64 x 1024 +
  // half of a second one) and 77.9 ms against 16.9 ms at 393 216 (profiles/range_sync_bench.json, DESIGN.md section
  // 3.21).  Clouds with distinct times (Velodyne, Robosense) are not limited: 0.41 ms against 4.2 ms and 0.94 ms against
  // 25.7 ms at the same sizes.
  static constexpr int64_t kMaxColumnTimePointsOnDevice = 0;

 private:
  bool FastPath(const std::string& sensor_id) const {
    return synchronizer_.SingleSensor(sensor_id) && !options_.enable_manual_descrew && options_.num_accumulated_range_data == 1;
  }
  std::unique_ptr<MatchingResult> AddSingleSensorRangeData(const sensor::TimedCloudOnDevice& ranges) {
    if (ranges.size() != 0 && !imu_initialized_) return Initialize(ranges.time(), [&] { return DevicePoints(ranges); });
    if (ranges.size() == 0 || !imu_initialized_ || !have_prediction_) return nullptr;
    if (ranges.back_time() > 0.1f) Check(DLIOM_ERR_INVALID_ARGUMENT, "CHECK_LE(ranges.back().point_time[3], 0.1f)");
    DLIOM_ADAPTER_STAGE(0);
    double prev[7], vel[3], bias[6], predicted[7], pvel[3];
    Check(dliom_imu_window_state(window_, 0, prev, vel, bias), "dliom_imu_window_state");
    Check(dliom_imu_window_predict(window_, predicted, pvel), "dliom_imu_window_predict");
    accumulation_started_ = std::chrono::steady_clock::now();
    const float origin[3] = {ranges.origin().x, ranges.origin().y, ranges.origin().z};
    dliom_cloud* cloud = nullptr;
    float origin_in_tracking[3], current_pose[7];
    Check(dliom_add_range_data_timed_cloud(context_->get(), prev, predicted, options_.scan_period, ranges.get(), origin,
                                           options_.min_range, options_.max_range, options_.voxel_filter_size, &cloud,
                                           origin_in_tracking, current_pose),
          "AddRangeData (de-skew, filters, tracking frame)");
    DLIOM_ADAPTER_STAGE(1);
    return AddAccumulatedRangeData(ranges.time(), current_pose, origin_in_tracking, cloud);
  }

 public:
  const ActiveSubmaps3D& active_submaps() const { return active_submaps_; }
  // local_trajectory_builder_3d.h:113, .cc:624-649: the same five metrics under the same family names, labels and bucket
  // boundaries; they are process-wide like the reference's file-scope statics and observe nothing until this is called
  static void RegisterMetrics(metrics::FamilyFactory* family_factory) {
    Metrics& m = metrics_();
    m.latency = family_factory->NewGaugeFamily("mapping_internal_3d_local_trajectory_builder_latency",
                                               "Duration from first incoming point cloud in accumulation to local slam result")
                    ->Add({});
    auto* scores = family_factory->NewHistogramFamily("mapping_internal_3d_local_trajectory_builder_scores",
                                                      "Local scan matcher scores", metrics::Histogram::FixedWidth(0.05, 20));
    m.rtcsm_score = scores->Add({{"scan_matcher", "real_time_correlative"}});
    auto* costs = family_factory->NewHistogramFamily("mapping_internal_3d_local_trajectory_builder_costs",
                                                     "Local scan matcher costs", metrics::Histogram::ScaledPowersOf(2, 0.01, 100));
    m.ceres_cost = costs->Add({{"scan_matcher", "ceres"}});
    auto* residuals = family_factory->NewHistogramFamily("mapping_internal_3d_local_trajectory_builder_residuals",
                                                         "Local scan matcher residuals", metrics::Histogram::ScaledPowersOf(2, 0.01, 10));
    m.residual_distance = residuals->Add({{"component", "distance"}});
    m.residual_angle = residuals->Add({{"component", "angle"}});
  }
  // g_vec_est_G_ of the last EstimateGravity() (.cc:1106-1154), whether it passed the gates, gravity factors added so far
  // (options.imu.enable_gravity_factor: WindowOptimize adds the Pose3GravityFactor itself, .cc:819-831)
  bool GravityEstimate(transform::Vector3d* gravity_in_global, int64_t* factors_added = nullptr) const {
    int valid = 0;
    Check(dliom_imu_window_gravity_estimate(window_, gravity_in_global->v, &valid, factors_added), "EstimateGravity");
    return valid != 0;
  }

 private:
  cartographer_ros::NodeCloudCache* node_cloud_cache_ = nullptr;
  int node_cloud_trajectory_id_ = 0;
  struct Metrics {  // kLocalSlamLatencyMetric ... kScanMatcherResidualAngleMetric (.cc:36-41)
    metrics::Gauge* latency = metrics::Gauge::Null();
    metrics::Histogram* rtcsm_score = metrics::Histogram::Null();
    metrics::Histogram* ceres_cost = metrics::Histogram::Null();
    metrics::Histogram* residual_distance = metrics::Histogram::Null();
    metrics::Histogram* residual_angle = metrics::Histogram::Null();
  };
  static Metrics& metrics_() {
    static Metrics m;
    return m;
  }
  // .cc:493-572
  std::unique_ptr<MatchingResult> AddAccumulatedRangeData(int64_t time, const float current_pose[7], const float origin[3],
                                                          dliom_cloud* cloud) {
    struct Owner {
      dliom_cloud* c;
      ~Owner() { dliom_cloud_destroy(c); }
    } owner{cloud};
    int64_t n = 0;
    Check(dliom_cloud_size(cloud, &n), "dliom_cloud_size");
    if (n == 0) return nullptr;  // "Dropped empty range data."
    double prediction[7];
    for (int i = 0; i < 7; ++i) prediction[i] = static_cast<double>(current_pose[i]);  // current_pose.cast<double>()
    dliom_match_result m;
    Check(dliom_front_end_match_cloud(active_submaps_.get(), prediction, origin, cloud, &m), "AddAccumulatedRangeData (match)");
    DLIOM_ADAPTER_STAGE(2);
    if (m.dropped) return nullptr;
    if (options_.front_end.use_online_correlative_scan_matching) metrics_().rtcsm_score->Observe(m.rtcsm_score);  // :520
    metrics_().ceres_cost->Observe(m.summary.final_cost);                                                         // :543
    metrics_().residual_distance->Observe(m.residual_distance);                                                   // :547
    metrics_().residual_angle->Observe(m.residual_angle);                                                         // :551
    // WindowOptimize(pose_estimate, false) and opt_pose = PoseFromGtsamNavState(prev_state_)
    double opt[7], vel[3], bias[6];
    // (its first call after SetInitialState only starts the graph and returns the initial state, like the reference's)
    const int ws = dliom_imu_window_window_optimize(window_, m.pose_estimate, 0, opt, vel, bias);
    // FailureDetection (.cc:856-859): ResetParams() and on with the scan -- opt_pose is what the diverged solve left in
    // prev_state_, and the next WindowOptimize starts a new graph there (the library does; failure_detections() counts)
    if (ws == DLIOM_ERR_DIVERGED)
      ++failure_detections_;
    else
      Check(ws, "WindowOptimize");
    DLIOM_ADAPTER_STAGE(3);
    have_prediction_ = false;
    std::unique_ptr<MatchingResult> result(new MatchingResult);
    result->time = time;
    result->local_pose = transform::Rigid3d::FromArray(opt);
    // filtered_range_data_in_local = TransformRangeData(in_tracking, opt_pose.cast<float>())
    // (on the device, where the cloud is: one kernel writes the moved points into pinned memory -- a download followed by
    // a host loop over ~30 000 returns was a third of the adapter's time per scan, round 6)
    float pf[7];
    for (int i = 0; i < 7; ++i) pf[i] = static_cast<float>(opt[i]);
    result->range_data_in_local.origin = TransformPoint(pf, origin[0], origin[1], origin[2]);
    result->range_data_in_local.returns.resize(static_cast<size_t>(n));
    static_assert(sizeof(sensor::Vector3f) == 12, "packed xyz");
    if (node_cloud_cache_ != nullptr)
      result->node_cloud_index = node_cloud_cache_->OnLocalSlamResult(node_cloud_trajectory_id_, time, result->local_pose, cloud, pf,
                                                                      result->range_data_in_local.origin);
    DLIOM_ADAPTER_STAGE(4);
    // ComputeHistogram (.cc:605-610) reads the same filtered cloud as the insertion and writes nothing the insertion
    // reads: its kernels are started first, on the context's auxiliary stream, and run beside the insertion's
    const float rot_wxyz[4] = {pf[3], pf[4], pf[5], pf[6]};
    const bool histogram_on_device = options_.rotational_histogram_size > 0 && options_.rotational_histogram_size <= 255;
    bool histogram_pending = false;
    if (histogram_on_device) {
      const int hb = dliom_cloud_rotational_histogram_begin(context_->get(), cloud, rot_wxyz, options_.rotational_histogram_size);
      if (hb != DLIOM_ERR_CAPACITY) Check(hb, "RotationalScanMatcher::ComputeHistogram (begin)");
      histogram_pending = hb == DLIOM_OK;
    }
    struct PendingHistogram {  // never leave one pending on the context, whatever path leaves this function
      dliom_ctx* c;
      bool* pending;
      ~PendingHistogram() {
        float discard[256];
        if (*pending) (void)dliom_cloud_rotational_histogram_finish(c, discard);
      }
    } pending_guard{context_->get(), &histogram_pending};
    DLIOM_ADAPTER_STAGE(5);
    // (the returns come down while the histogram's kernels run on their stream: in front of them this wait was exposed)
    Check(dliom_cloud_download_transformed(cloud, pf, &result->range_data_in_local.returns[0].x), "TransformRangeData");
    DLIOM_ADAPTER_STAGE(6);
    // InsertIntoSubmap (.cc:584-622): gravity_alignment = opt_pose.rotation()
    dliom_insertion_result ins;
    Check(dliom_front_end_insert(active_submaps_.get(), time, opt, opt + 3, &ins), "InsertIntoSubmap");
    DLIOM_ADAPTER_STAGE(7);
    if (ins.inserted) {
      std::unique_ptr<InsertionResult> ir(new InsertionResult);
      ir->time = time;
      ir->gravity_alignment = transform::Quaterniond{{opt[3], opt[4], opt[5], opt[6]}};
      ir->local_pose = result->local_pose;
      for (int i = 0; i < ins.num_insertion_submaps; ++i) ir->insertion_submap_indices.push_back(ins.insertion_submap_index[i]);
      ir->submap_finished = ins.submap_finished != 0;
      // (the two adaptively filtered clouds first: their downloads overlap what is left of the histogram)
      const dliom_cloud* filtered[2] = {nullptr, nullptr};
      Check(dliom_front_end_matched_clouds(active_submaps_.get(), &filtered[0], &filtered[1]), "matched clouds");
      sensor::PointCloud* const dst[2] = {&ir->high_resolution_point_cloud, &ir->low_resolution_point_cloud};
      for (int k = 0; k < 2; ++k) {
        int64_t m_points = 0;
        if (filtered[k] == nullptr) continue;
        Check(dliom_cloud_size(filtered[k], &m_points), "dliom_cloud_size");
        dst[k]->resize(static_cast<size_t>(m_points));
        if (m_points > 0) Check(dliom_cloud_download(filtered[k], &(*dst[k])[0].x), "dliom_cloud_download");
      }
      DLIOM_ADAPTER_STAGE(8);
      // ComputeHistogram(TransformPointCloud(filtered_range_data_in_tracking.returns, Rotation(gravity_alignment.cast<float>())), size)
      // on the device, where the filtered cloud already is (rotation fused; slices of any size -- the floor of a real scan
      // puts 15 000 returns into one 0.2 m slice); the host version only for what the device one refuses (|z| beyond
      // 409 m, non-finite coordinates, more than 63 slices above 4096 points): histogram_host_fallbacks() counts them
      if (options_.rotational_histogram_size > 0) {
        ir->rotational_scan_matcher_histogram.resize(static_cast<size_t>(options_.rotational_histogram_size));
        int hs = DLIOM_ERR_CAPACITY;
        if (histogram_pending) {
          histogram_pending = false;
          hs = dliom_cloud_rotational_histogram_finish(context_->get(), ir->rotational_scan_matcher_histogram.data());
        }
        if (hs == DLIOM_ERR_CAPACITY) {
          ++histogram_host_fallbacks_;
          const float rot[7] = {0.f, 0.f, 0.f, pf[3], pf[4], pf[5], pf[6]};
          std::vector<float> aligned(3 * static_cast<size_t>(n));  // (rare path: the rotation on the device all the same)
          Check(dliom_cloud_download_transformed(cloud, rot, aligned.data()), "TransformPointCloud (gravity alignment)");
          hs = dliom_rotational_histogram(aligned.data(), n, options_.rotational_histogram_size,
                                          ir->rotational_scan_matcher_histogram.data());
        }
        Check(hs, "RotationalScanMatcher::ComputeHistogram");
      }
      DLIOM_ADAPTER_STAGE(9);
      result->insertion_result = std::move(ir);
    }
    DLIOM_ADAPTER_STAGE(10);
    // .cc:566-568 (whole seconds, as the reference casts it)
    metrics_().latency->Set(static_cast<double>(
        std::chrono::duration_cast<std::chrono::seconds>(std::chrono::steady_clock::now() - accumulation_started_).count()));
    return result;
  }
  // Rigid3f * Vector3f with Eigen's operation order (rotation * p + translation)
  static sensor::Vector3f TransformPoint(const float p7[7], float x, float y, float z) {
    const float w = p7[3], qx = p7[4], qy = p7[5], qz = p7[6];
    float uvx = qy * z - qz * y, uvy = qz * x - qx * z, uvz = qx * y - qy * x;
    uvx += uvx;
    uvy += uvy;
    uvz += uvz;
    const float cx = qy * uvz - qz * uvy, cy = qz * uvx - qx * uvz, cz = qx * uvy - qy * uvx;
    return sensor::Vector3f{((x + w * uvx) + cx) + p7[0], ((y + w * uvy) + cy) + p7[1], ((z + w * uvz) + cz) + p7[2]};
  }

  // ---- the reference's initialisation (.cc:372-381): every scan before the state is known ends here; nullptr, always ----
  template <class MakeCloud>
  std::unique_ptr<MatchingResult> Initialize(int64_t time, MakeCloud&& make_cloud) {
    if (!options_.internal_initialization) return nullptr;  // dropped: the state comes from SetInitialState()
    if (options_.enable_ndt_initialization) {
      InitilizeByNDT(time, make_cloud);
    } else if (accumulated_frame_num_++ > options_.frames_for_static_initialization) {
      InitializeStatic();
    }
    return nullptr;
  }
  // cvtPointCloud: the xyz of the scan as a cloud of the context (owned by the caller)
  dliom_cloud* UploadPoints(const float* first_x, size_t stride_floats, size_t n) {
    std::vector<float> xyz(3 * n);
    for (size_t i = 0; i < n; ++i)
      for (int a = 0; a < 3; ++a) xyz[3 * i + a] = first_x[stride_floats * i + a];
    dliom_cloud* cloud = nullptr;
    Check(dliom_cloud_create(context_->get(), xyz.data(), static_cast<int64_t>(n), &cloud), "dliom_cloud_create");
    return cloud;
  }
  dliom_cloud* DevicePoints(const sensor::TimedCloudOnDevice& ranges) {
    dliom_cloud* cloud = nullptr;
    Check(dliom_timed_cloud_points(context_->get(), ranges.get(), &cloud), "dliom_timed_cloud_points");
    return cloud;
  }
  // InitializeStatic (.cc:203-229) on the buffered IMU samples; without one the scan is only counted
  void InitializeStatic() {
    if (init_imu_buffer_.empty()) return;
    std::vector<double> acc(3 * init_imu_buffer_.size()), gyr(3 * init_imu_buffer_.size());
    for (size_t i = 0; i < init_imu_buffer_.size(); ++i)
      for (int a = 0; a < 3; ++a) {
        acc[3 * i + a] = init_imu_buffer_[i].linear_acceleration[a];
        gyr[3 * i + a] = init_imu_buffer_[i].angular_velocity[a];
      }
    double R[9], bias[6], P[3], V[3];
    Check(dliom_imu_static_initialization(static_cast<int64_t>(init_imu_buffer_.size()), acc.data(), gyr.data(), options_.imu.gravity, R,
                                          bias, bias + 3, P, V),
          "dliom_imu_static_initialization");
    init_imu_buffer_.clear();
    SetInitialState(transform::Rigid3d(transform::Vector3d{{P[0], P[1], P[2]}}, QuaternionOfMatrix(R)), transform::Vector3d{{V[0], V[1], V[2]}},
                    bias);
  }
  // InitilizeByNDT (.cc:231-330), including what looks odd: a frame's translation is the pair's own t, not an accumulated
  // one.  The guess and the velocity are float arithmetic, as the reference's Matrix4f / Vector3f: init_q = (float)deltaQ,
  // init_R its matrix by toRotationMatrix's formula in float, dt = (float)(seconds between the scans),
  // init_t = linear_velocity * dt, linear_velocity = t / dt.
  template <class MakeCloud>
  void InitilizeByNDT(int64_t time, MakeCloud&& make_cloud) {
    const double zero[3] = {0., 0., 0.};
    const dliom_imu_noise noise{options_.imu.acc_noise, options_.imu.gyr_noise, options_.imu.acc_bias_noise, options_.imu.gyr_bias_noise};
    struct Scan {  // destroyed on every way out
      dliom_cloud* cloud;
      ~Scan() { dliom_cloud_destroy(cloud); }
    };
    if (init_frames_.empty()) {
      if (last_imu_time_ini_ < 0) return;  // still no IMU sample
      const Scan scan{make_cloud()};
      Check(dliom_ndt_scan_matcher_match(init_matcher_, scan.cloud, nullptr, nullptr), "MatchByNDT (first scan)");
      last_scan_time_ = time;
      linear_velocity_[0] = linear_velocity_[1] = linear_velocity_[2] = 0.f;
      dliom_init_frame first = {};
      first.pose[3] = 1.0;  // the identity, no preintegration
      init_frames_.push_back(first);
      Check(dliom_imu_integrator_reset(init_integrator_, zero, zero, &noise), "resetIntegration");
      return;
    }
    const float dt = static_cast<float>(static_cast<double>(time - last_scan_time_) * 1e-7);
    dliom_imu_preintegration running;
    Check(dliom_imu_integrator_get(init_integrator_, &running), "dliom_imu_integrator_get");
    const float w = static_cast<float>(running.delta_q[0]), x = static_cast<float>(running.delta_q[1]),
                y = static_cast<float>(running.delta_q[2]), z = static_cast<float>(running.delta_q[3]);
    const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const float guess[16] = {1.f - (tyy + tzz), txy - twz, txz + twy, linear_velocity_[0] * dt,
                             txy + twz, 1.f - (txx + tzz), tyz - twx, linear_velocity_[1] * dt,
                             txz - twy, tyz + twx, 1.f - (txx + tyy), linear_velocity_[2] * dt,
                             0.f, 0.f, 0.f, 1.f};
    double guess16[16];
    for (int k = 0; k < 16; ++k) guess16[k] = static_cast<double>(guess[k]);
    dliom_ndt_result result = {};
    {
      const Scan scan{make_cloud()};
      Check(dliom_ndt_scan_matcher_match(init_matcher_, scan.cloud, guess16, &result), "MatchByNDT");
    }
    float R[9], t[3];  // MatchByNDT's Matrix3f and Vector3f
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) R[3 * r + c] = static_cast<float>(result.transform[4 * r + c]);
      t[r] = static_cast<float>(result.transform[4 * r + 3]);
    }
    // Rigid3d(t, Quaterniond(R_previous_frame * R))
    const dliom_init_frame& previous = init_frames_.back();
    double Rp[9], Rf[9];
    MatrixOfQuaternion(&previous.pose[3], Rp);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)
        Rf[3 * r + c] = (Rp[3 * r] * static_cast<double>(R[c]) + Rp[3 * r + 1] * static_cast<double>(R[3 + c])) +
                        Rp[3 * r + 2] * static_cast<double>(R[6 + c]);
    const transform::Quaterniond q = QuaternionOfMatrix(Rf);
    dliom_init_frame frame = {};
    for (int a = 0; a < 3; ++a) {
      frame.pose[a] = static_cast<double>(t[a]);
      frame.delta_p[a] = running.delta_p[a];
      frame.delta_v[a] = running.delta_v[a];
      linear_velocity_[a] = t[a] / dt;
    }
    for (int a = 0; a < 4; ++a) frame.pose[3 + a] = q.wxyz[a];
    frame.has_preintegration = 1;
    frame.sum_dt = running.sum_dt;
    init_frames_.push_back(frame);
    Check(dliom_imu_integrator_reset(init_integrator_, zero, zero, &noise), "resetIntegration");
    last_scan_time_ = time;
    const int frames = options_.frames_for_dynamic_initialization + 1;
    if (static_cast<int>(init_frames_.size()) != frames) return;
    std::vector<double> P(3 * frames), Rs(9 * frames), V(3 * frames);
    double g_laser[3], Rw[9], excitation = 0.;
    int outcome = -1;
    const std::array<double, 7> lb = options_.transform_lb.ToArray();
    Check(dliom_imu_lidar_align_with_world(init_frames_.data(), frames, lb.data(), options_.imu.gravity, P.data(), Rs.data(), V.data(),
                                           g_laser, Rw, &excitation, &outcome),
          "AlignWithWorld");
    if (outcome != DLIOM_INIT_OK) {  // re-initialisation: one frame, the last scan stays the matcher's
      ++initialization_failures_;
      init_frames_.resize(1);
      return;
    }
    const int last = frames - 1;
    const double bias[6] = {0., 0., 0., 0., 0., 0.};
    SetInitialState(transform::Rigid3d(transform::Vector3d{{P[3 * last], P[3 * last + 1], P[3 * last + 2]}}, QuaternionOfMatrix(&Rs[9 * last])),
                    transform::Vector3d{{V[3 * last], V[3 * last + 1], V[3 * last + 2]}}, bias);
  }
  // Eigen's Quaternion::toRotationMatrix and Quaterniond(Matrix3d), operation for operation (row-major matrices)
  static void MatrixOfQuaternion(const double wxyz[4], double R[9]) {
    const double w = wxyz[0], x = wxyz[1], y = wxyz[2], z = wxyz[3];
    const double tx = 2. * x, ty = 2. * y, tz = 2. * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                 tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double m[9] = {1. - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1. - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1. - (txx + tyy)};
    for (int k = 0; k < 9; ++k) R[k] = m[k];
  }
  static transform::Quaterniond QuaternionOfMatrix(const double m[9]) {
    transform::Quaterniond q{{1., 0., 0., 0.}};
    double t = (m[0] + m[4]) + m[8];
    if (t > 0.) {
      t = std::sqrt(t + 1.0);
      q.wxyz[0] = 0.5 * t;
      t = 0.5 / t;
      q.wxyz[1] = (m[7] - m[5]) * t;
      q.wxyz[2] = (m[2] - m[6]) * t;
      q.wxyz[3] = (m[3] - m[1]) * t;
    } else {
      int i = 0;
      if (m[4] > m[0]) i = 1;
      if (m[8] > m[4 * i]) i = 2;
      const int j = (i + 1) % 3, k = (j + 1) % 3;
      t = std::sqrt(((m[4 * i] - m[4 * j]) - m[4 * k]) + 1.0);
      q.wxyz[1 + i] = 0.5 * t;
      t = 0.5 / t;
      q.wxyz[0] = (m[3 * k + j] - m[3 * j + k]) * t;
      q.wxyz[1 + j] = (m[3 * j + i] + m[3 * i + j]) * t;
      q.wxyz[1 + k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
    return q;
  }
  std::vector<dliom_init_frame> init_frames_;  // all_laser_transforms_[0 .. buffered_scan_count_)
  dliom_imu_integrator* init_integrator_ = nullptr;
  dliom_ndt_scan_matcher* init_matcher_ = nullptr;  // holds last_scan_
  std::vector<sensor::ImuData> init_imu_buffer_;
  int64_t last_imu_time_ini_ = -1, last_scan_time_ = 0, initialization_failures_ = 0;
  float linear_velocity_[3] = {0.f, 0.f, 0.f};
  int accumulated_frame_num_ = 0;
  double initial_state_[16] = {};

  Context* context_;
  LocalTrajectoryBuilderOptions3D options_;
  ActiveSubmaps3D active_submaps_;
  RangeDataSynchronizer synchronizer_;
  dliom_imu_window* window_ = nullptr;
  dliom_range_accumulator* accumulator_ = nullptr;
  int64_t last_imu_time_ = -1;
  bool imu_initialized_ = false;
  bool have_prediction_ = false;
  int64_t failure_detections_ = 0;
  bool accumulating_ = false;  // num_accumulated_ > 0
  std::chrono::steady_clock::time_point accumulation_started_ = std::chrono::steady_clock::now();
  int64_t histogram_host_fallbacks_ = 0;
  int64_t merge_host_fallbacks_ = 0, merges_left_to_host_ = 0, device_merges_ = 0;

 public:
  // ComputeHistogram calls that the device entry point refused and the host one served
  int64_t histogram_host_fallbacks() const { return histogram_host_fallbacks_; }
  // scans after which FailureDetection fired (large velocity / bias: "reset IMU-preintegration!")
  int64_t failure_detections() const { return failure_detections_; }
};

}  // namespace mapping

// ---- cartographer_ros/sensor_bridge.cc:176-240, 286-299: a PointCloud2 message into the local trajectory builder ---------
// HandlePointCloud2Message's per-point code -- the gather of the sensor's fields, the finite test, the times re-based to
// the last point, the stamp moved there -- and HandleRangefinder's change into the tracking frame run on the device in one
// pass over the message's bytes, and the result feeds LocalTrajectoryBuilder3D::AddRangeData without coming back.  tf is the
// caller's: sensor_to_tracking is what tf_bridge_.LookupToTracking(time, frame_id) returned (a null lookup drops the
// message before this is called).  LaserScan and MultiEchoLaserScan messages are not handled here.
class SensorBridge {
 public:
  SensorBridge(Context* context, mapping::LocalTrajectoryBuilder3D* trajectory_builder)
      : context_(context), trajectory_builder_(trajectory_builder) {}
  // sensor_type: "ouster", "velodyne", "robosense"; anything else is a pcl::PointXYZI cloud without point times
  static int ModeOf(const std::string& sensor_type) {
    return sensor_type == "ouster"      ? DLIOM_POINT_CLOUD2_SLAM_OUSTER
           : sensor_type == "velodyne"  ? DLIOM_POINT_CLOUD2_SLAM_VELODYNE
           : sensor_type == "robosense" ? DLIOM_POINT_CLOUD2_SLAM_ROBOSENSE
                                        : DLIOM_POINT_CLOUD2_SLAM_OTHER;
  }
  std::unique_ptr<mapping::LocalTrajectoryBuilder3D::MatchingResult> HandlePointCloud2Message(
      const std::string& sensor_id, const sensor_msgs::PointCloud2& msg, const std::string& sensor_type,
      const transform::Rigid3d& sensor_to_tracking) {
    sensor::TimedCloudOnDevice ranges(context_, msg, ModeOf(sensor_type), &sensor_to_tracking);
    return trajectory_builder_->AddRangeData(sensor_id, std::move(ranges));
  }

 private:
  Context* context_;
  mapping::LocalTrajectoryBuilder3D* trajectory_builder_;
};

// ---- pose graph optimisation (mapping/internal/optimization/optimization_problem_3d.h) --------------------------------
namespace mapping {
struct SubmapId {  // mapping/id.h
  int trajectory_id;
  int submap_index;
  bool operator<(const SubmapId& o) const { return trajectory_id != o.trajectory_id ? trajectory_id < o.trajectory_id : submap_index < o.submap_index; }
  bool operator==(const SubmapId& o) const { return trajectory_id == o.trajectory_id && submap_index == o.submap_index; }
};
struct NodeId {
  int trajectory_id;
  int node_index;
  bool operator<(const NodeId& o) const { return trajectory_id != o.trajectory_id ? trajectory_id < o.trajectory_id : node_index < o.node_index; }
  bool operator==(const NodeId& o) const { return trajectory_id == o.trajectory_id && node_index == o.node_index; }
};
namespace optimization {
struct NodeSpec3D {  // optimization_problem_3d.h:44-48
  int64_t time;
  transform::Rigid3d local_pose;
  transform::Rigid3d global_pose;
};
struct SubmapSpec3D {  // :50-52
  transform::Rigid3d global_pose;
};
struct OptimizationProblemOptions {  // proto/optimization_problem_options.proto: the fields the fork's Solve reads
  bool fix_z_in_3d = false;
  bool use_nonmonotonic_steps = false;
  int max_num_iterations = 50;
  int num_threads = 1;
  double fixed_frame_pose_translation_weight = 1e1;  // pose_graph.lua:81-82
  double fixed_frame_pose_rotation_weight = 1e2;
  // The fork's binary ignores its configurations' huber_scale (it builds TrivialLoss, optimization_problem_3d.cc:
  // 335-338): 0 is that.  Upstream's behaviour is huber_scale > 0 (basic_config_3d.lua:108 sets 1e2, campus.lua:20
  // 1e5): HuberLoss on the INTER_SUBMAP constraints.
  double huber_scale = 0.;
  // Landmarks are opt-in: false keeps the refusal of a non-empty landmark_nodes that callers of the earlier adapter
  // rely on; true adds AddLandmarkCostFunctions (optimization_problem_3d.cc:124-186).
  bool use_landmarks = false;
};
struct LandmarkNode {  // pose_graph_interface.h:57-67; times in ticks of 100 ns
  struct LandmarkObservation {
    int trajectory_id;
    int64_t time;
    transform::Rigid3d landmark_to_tracking_transform;
    double translation_weight;
    double rotation_weight;
  };
  std::vector<LandmarkObservation> landmark_observations;
  common::optional<transform::Rigid3d> global_landmark_pose;
};
struct TrajectoryData {  // pose_graph_interface.h:76-80; the first two are stored and unused, as in the fork
  double gravity_constant = 9.8;
  std::array<double, 4> imu_calibration{{1., 0., 0., 0.}};
  common::optional<transform::Rigid3d> fixed_frame_origin_in_map;
};

// The host arithmetic of the fixed-frame terms (optimization_problem_3d.cc:78-102, 491-548), as Eigen does it.
namespace fixed_frame {
inline std::array<double, 3> Rotate(const transform::Quaterniond& q, const double v[3]) {  // QuaternionBase::_transformVector
  const double uv[3] = {2. * (q.y() * v[2] - q.z() * v[1]), 2. * (q.z() * v[0] - q.x() * v[2]), 2. * (q.x() * v[1] - q.y() * v[0])};
  return {{v[0] + q.w() * uv[0] + (q.y() * uv[2] - q.z() * uv[1]), v[1] + q.w() * uv[1] + (q.z() * uv[0] - q.x() * uv[2]),
           v[2] + q.w() * uv[2] + (q.x() * uv[1] - q.y() * uv[0])}};
}
inline transform::Rigid3d Inverse(const transform::Rigid3d& a) {  // Rigid3::inverse
  const transform::Quaterniond q{{a.rotation().w(), -a.rotation().x(), -a.rotation().y(), -a.rotation().z()}};
  const std::array<double, 3> t = Rotate(q, a.translation().v);
  return transform::Rigid3d(transform::Vector3d{{-t[0], -t[1], -t[2]}}, q);
}
inline transform::Rigid3d Multiply(const transform::Rigid3d& a, const transform::Rigid3d& b) {  // operator*(Rigid3, Rigid3)
  const std::array<double, 3> t = Rotate(a.rotation(), b.translation().v);
  const transform::Quaterniond &p = a.rotation(), &q = b.rotation();
  const double w = p.w() * q.w() - p.x() * q.x() - p.y() * q.y() - p.z() * q.z(), x = p.w() * q.x() + p.x() * q.w() + p.y() * q.z() - p.z() * q.y(),
               y = p.w() * q.y() + p.y() * q.w() + p.z() * q.x() - p.x() * q.z(), z = p.w() * q.z() + p.z() * q.w() + p.x() * q.y() - p.y() * q.x();
  const double norm = std::sqrt(w * w + x * x + y * y + z * z);
  return transform::Rigid3d(transform::Vector3d{{t[0] + a.translation().v[0], t[1] + a.translation().v[1], t[2] + a.translation().v[2]}},
                            transform::Quaterniond{{w / norm, x / norm, y / norm, z / norm}});
}
// Rigid3d(translation, AngleAxisd(GetYaw(rotation), UnitZ)) (:529-533, transform.h:43-47)
inline transform::Rigid3d YawOnly(const transform::Rigid3d& a) {
  const double unit_x[3] = {1., 0., 0.};
  const std::array<double, 3> direction = Rotate(a.rotation(), unit_x);
  const double yaw = std::atan2(direction[1], direction[0]);
  return transform::Rigid3d(a.translation(), transform::Quaterniond{{std::cos(yaw / 2.), 0., 0., std::sin(yaw / 2.)}});
}
// transform::Interpolate (timestamped_transform.cc:23-39) with Eigen's slerp; times in ticks of 100 ns
inline transform::Rigid3d Interpolate(int64_t start_time, const transform::Rigid3d& start, int64_t end_time, const transform::Rigid3d& end,
                                      int64_t time) {
  const double duration = static_cast<double>(end_time - start_time) / 1e7;
  const double factor = static_cast<double>(time - start_time) / 1e7 / duration;
  transform::Vector3d origin;
  for (int k = 0; k < 3; ++k) origin.v[k] = start.translation().v[k] + (end.translation().v[k] - start.translation().v[k]) * factor;
  const transform::Quaterniond &p = start.rotation(), &q = end.rotation();
  const double d = p.w() * q.w() + p.x() * q.x() + p.y() * q.y() + p.z() * q.z(), abs_d = std::fabs(d);
  double scale0 = 1. - factor, scale1 = factor;
  if (!(abs_d >= 1. - 2.220446049250313e-16)) {
    const double theta = std::acos(abs_d), sin_theta = std::sin(theta);
    scale0 = std::sin((1. - factor) * theta) / sin_theta;
    scale1 = std::sin(factor * theta) / sin_theta;
  }
  if (d < 0.) scale1 = -scale1;
  transform::Quaterniond rotation;
  for (int k = 0; k < 4; ++k) rotation.wxyz[k] = scale0 * p.wxyz[k] + scale1 * q.wxyz[k];
  return transform::Rigid3d(origin, rotation);
}
}  // namespace fixed_frame

// OptimizationProblem3D (optimization_problem_3d.h:54-132, .cc:196-589) over dliom_pose_graph_solve_landmarks.  MapById is a
// std::map ordered like it (trajectory, index); Append continues a trajectory's indices; MapByTime is a std::map by time
// a trajectory.  The IMU, odometry and local-SLAM terms are commented out in the fork's Solve (:350-489), so that data
// is stored and unused.  The fixed-frame pose constraints (:491-548) are live code there and are built here; so is the
// loss the fork left out (options.huber_scale).  Landmarks (:124-186) are built with options.use_landmarks; without it
// Solve refuses a non-empty landmark_nodes.
class OptimizationProblem3D {
 public:
  struct Constraint {  // PoseGraphInterface::Constraint
    struct Pose {
      transform::Rigid3d zbar_ij;
      double translation_weight;
      double rotation_weight;
    };
    SubmapId submap_id;
    NodeId node_id;
    Pose pose;
    enum Tag { INTRA_SUBMAP, INTER_SUBMAP } tag = INTRA_SUBMAP;
  };

  OptimizationProblem3D(Context* context, const OptimizationProblemOptions& options) : context_(context), options_(options) {}
  OptimizationProblem3D(const OptimizationProblem3D&) = delete;
  OptimizationProblem3D& operator=(const OptimizationProblem3D&) = delete;

  void AddImuData(int trajectory_id, const sensor::ImuData& imu_data) { imu_data_[trajectory_id].push_back(imu_data); }  // stored, unused, as in the fork
  void AddFixedFramePoseData(int trajectory_id, const sensor::FixedFramePoseData& fixed_frame_pose_data) {  // MapByTime::Append
    std::map<int64_t, sensor::FixedFramePoseData>& trajectory = fixed_frame_pose_data_[trajectory_id];
    if (!trajectory.empty() && !(fixed_frame_pose_data.time > trajectory.rbegin()->first))
      Check(DLIOM_ERR_INVALID_ARGUMENT, "AddFixedFramePoseData: CHECK_GT(data.time, the last time)");
    trajectory.emplace(fixed_frame_pose_data.time, fixed_frame_pose_data);
  }
  void SetTrajectoryData(int trajectory_id, const TrajectoryData& trajectory_data) { trajectory_data_[trajectory_id] = trajectory_data; }
  void AddTrajectoryNode(int trajectory_id, const NodeSpec3D& node_data) {
    node_data_.emplace(NodeId{trajectory_id, NextIndex(node_data_, NodeId{trajectory_id, 0}, &NodeId::node_index)}, node_data);
    trajectory_data_[trajectory_id];
  }
  void InsertTrajectoryNode(const NodeId& node_id, const NodeSpec3D& node_data) {
    if (!node_data_.emplace(node_id, node_data).second) Check(DLIOM_ERR_INVALID_ARGUMENT, "InsertTrajectoryNode: the id exists");
    trajectory_data_[node_id.trajectory_id];
  }
  void TrimTrajectoryNode(const NodeId& node_id) {  // :229-237
    const auto node_it = node_data_.find(node_id);
    if (node_it == node_data_.end()) Check(DLIOM_ERR_INVALID_ARGUMENT, "TrimTrajectoryNode: no such id");
    TrimFixedFramePoseData(node_it);
    node_data_.erase(node_it);
    const auto rest = node_data_.lower_bound(NodeId{node_id.trajectory_id, 0});
    if (rest == node_data_.end() || rest->first.trajectory_id != node_id.trajectory_id) trajectory_data_.erase(node_id.trajectory_id);
  }
  void AddSubmap(int trajectory_id, const transform::Rigid3d& global_submap_pose) {
    submap_data_.emplace(SubmapId{trajectory_id, NextIndex(submap_data_, SubmapId{trajectory_id, 0}, &SubmapId::submap_index)},
                         SubmapSpec3D{global_submap_pose});
  }
  void InsertSubmap(const SubmapId& submap_id, const transform::Rigid3d& global_submap_pose) {
    if (!submap_data_.emplace(submap_id, SubmapSpec3D{global_submap_pose}).second) Check(DLIOM_ERR_INVALID_ARGUMENT, "InsertSubmap: the id exists");
  }
  void TrimSubmap(const SubmapId& submap_id) {
    if (submap_data_.erase(submap_id) != 1) Check(DLIOM_ERR_INVALID_ARGUMENT, "TrimSubmap: no such id");
  }
  void SetMaxNumIterations(int32_t max_num_iterations) { options_.max_num_iterations = max_num_iterations; }

  // optimization_problem_3d.cc:259-589: ids are compacted to indices in MapById order, the first submap is the
  // gravity-aligned one, the poses of a frozen trajectory are constant; the solved poses go back into the maps.
  void Solve(const std::vector<Constraint>& constraints, const std::set<int>& frozen_trajectories,
             const std::map<std::string, LandmarkNode>& landmark_nodes) {
    if (node_data_.empty()) return;  // nothing to optimize
    if (!landmark_nodes.empty() && !options_.use_landmarks)
      Check(DLIOM_ERR_INVALID_ARGUMENT, "OptimizationProblem3D::Solve: landmarks are not supported");
    if (submap_data_.empty()) Check(DLIOM_ERR_INVALID_ARGUMENT, "OptimizationProblem3D::Solve: CHECK(!submap_data_.empty())");
    std::map<SubmapId, int32_t> submap_index;
    std::map<NodeId, int32_t> node_index;
    std::vector<double> submap_poses, node_poses;
    std::vector<unsigned char> submap_constant, node_constant;
    for (const auto& id_data : submap_data_) {
      submap_index.emplace(id_data.first, static_cast<int32_t>(submap_index.size()));
      const std::array<double, 7> pose = id_data.second.global_pose.ToArray();
      submap_poses.insert(submap_poses.end(), pose.begin(), pose.end());
      submap_constant.push_back(frozen_trajectories.count(id_data.first.trajectory_id) != 0);
    }
    for (const auto& id_data : node_data_) {
      node_index.emplace(id_data.first, static_cast<int32_t>(node_index.size()));
      const std::array<double, 7> pose = id_data.second.global_pose.ToArray();
      node_poses.insert(node_poses.end(), pose.begin(), pose.end());
      node_constant.push_back(frozen_trajectories.count(id_data.first.trajectory_id) != 0);
    }
    std::vector<dliom_pose_graph_constraint> compact(constraints.size());
    for (size_t i = 0; i < constraints.size(); ++i) {
      const auto a = submap_index.find(constraints[i].submap_id);
      const auto n = node_index.find(constraints[i].node_id);
      if (a == submap_index.end() || n == node_index.end()) Check(DLIOM_ERR_INVALID_ARGUMENT, "OptimizationProblem3D::Solve: MapById::at");
      compact[i].submap = a->second;
      compact[i].node = n->second;
      const std::array<double, 7> zbar = constraints[i].pose.zbar_ij.ToArray();
      for (int k = 0; k < 7; ++k) compact[i].zbar[k] = zbar[k];
      compact[i].translation_weight = constraints[i].pose.translation_weight;
      compact[i].rotation_weight = constraints[i].pose.rotation_weight;
    }
    std::vector<unsigned char> inter_submap(constraints.size());
    for (size_t i = 0; i < constraints.size(); ++i) inter_submap[i] = constraints[i].tag == Constraint::INTER_SUBMAP;
    // :491-548: one block a trajectory that has fixed-frame data and at least one node that interpolates -- also on a
    // frozen trajectory, which the fork does not skip here
    std::vector<int> frame_trajectories;
    std::vector<double> frame_poses;
    std::vector<dliom_pose_graph_constraint> frame_constraints;
    for (const auto& id_data : node_data_) {
      const int trajectory_id = id_data.first.trajectory_id;
      if (fixed_frame_pose_data_.count(trajectory_id) == 0) continue;
      const std::unique_ptr<transform::Rigid3d> fixed_frame_pose = Interpolate(trajectory_id, id_data.second.time);
      if (fixed_frame_pose == nullptr) continue;
      if (frame_trajectories.empty() || frame_trajectories.back() != trajectory_id) {
        const TrajectoryData& trajectory_data = trajectory_data_.at(trajectory_id);
        const transform::Rigid3d fixed_frame_pose_in_map =
            trajectory_data.fixed_frame_origin_in_map.has_value()
                ? trajectory_data.fixed_frame_origin_in_map.value()
                : fixed_frame::Multiply(id_data.second.global_pose, fixed_frame::Inverse(*fixed_frame_pose));
        const std::array<double, 7> start = fixed_frame::YawOnly(fixed_frame_pose_in_map).ToArray();
        frame_trajectories.push_back(trajectory_id);
        frame_poses.insert(frame_poses.end(), start.begin(), start.end());
      }
      dliom_pose_graph_constraint c;
      c.submap = static_cast<int32_t>(frame_trajectories.size()) - 1;
      c.node = node_index.at(id_data.first);
      const std::array<double, 7> zbar = fixed_frame_pose->ToArray();
      for (int k = 0; k < 7; ++k) c.zbar[k] = zbar[k];
      c.translation_weight = options_.fixed_frame_pose_translation_weight;
      c.rotation_weight = options_.fixed_frame_pose_rotation_weight;
      frame_constraints.push_back(c);
    }
    LandmarkBlocks blocks = CompactLandmarks(frozen_trajectories, landmark_nodes);
    const std::vector<std::string>& landmark_ids = blocks.ids;
    std::vector<double>& landmark_poses = blocks.poses;
    const std::vector<unsigned char>& landmark_constant = blocks.constant;
    const std::vector<dliom_pose_graph_landmark_observation>& observations = blocks.observations;
    const dliom_pose_graph_landmarks landmarks = {static_cast<int>(landmark_ids.size()), landmark_poses.data(), landmark_constant.data(),
                                                  static_cast<int64_t>(observations.size()), observations.data()};
    const dliom_pose_graph_terms terms = {static_cast<int>(frame_trajectories.size()), frame_poses.data(),
                                          static_cast<int64_t>(frame_constraints.size()), frame_constraints.data(),
                                          options_.huber_scale, inter_submap.data()};
    const dliom_pose_graph_options options = {options_.fix_z_in_3d ? 1 : 0, options_.use_nonmonotonic_steps ? 1 : 0,
                                              options_.max_num_iterations, options_.num_threads};
    Check(dliom_pose_graph_solve_landmarks(context_->get(), &options, static_cast<int>(submap_index.size()), submap_poses.data(),
                                           submap_constant.data(), 0, static_cast<int>(node_index.size()), node_poses.data(),
                                           node_constant.data(), static_cast<int64_t>(compact.size()), compact.data(), &terms,
                                           &landmarks, &summary_),
          "dliom_pose_graph_solve_landmarks");
    size_t at = 0;  // :578-588: store the result
    for (auto& id_data : submap_data_) id_data.second.global_pose = transform::Rigid3d::FromArray(&submap_poses[7 * at++]);
    at = 0;
    for (auto& id_data : node_data_) id_data.second.global_pose = transform::Rigid3d::FromArray(&node_poses[7 * at++]);
    for (size_t f = 0; f < frame_trajectories.size(); ++f)
      trajectory_data_.at(frame_trajectories[f]).fixed_frame_origin_in_map = transform::Rigid3d::FromArray(&frame_poses[7 * f]);
    for (size_t l = 0; l < landmark_ids.size(); ++l) landmark_data_[landmark_ids[l]] = transform::Rigid3d::FromArray(&landmark_poses[7 * l]);
  }

  // :124-186 AddLandmarkCostFunctions on the host: the landmarks that are used, their start values and constant flags,
  // and the observations that have a node before and a node after them, on node indices in MapById order.  Touches no
  // device.
  struct LandmarkBlocks {
    std::vector<std::string> ids;
    std::vector<double> poses;  // 7 a landmark
    std::vector<unsigned char> constant;
    std::vector<dliom_pose_graph_landmark_observation> observations;
  };
  LandmarkBlocks CompactLandmarks(const std::set<int>& frozen_trajectories, const std::map<std::string, LandmarkNode>& landmark_nodes) const {
    LandmarkBlocks blocks;
    std::vector<std::string>& landmark_ids = blocks.ids;
    std::vector<double>& landmark_poses = blocks.poses;
    std::vector<unsigned char>& landmark_constant = blocks.constant;
    std::vector<dliom_pose_graph_landmark_observation>& observations = blocks.observations;
    std::map<NodeId, int32_t> node_index;
    std::vector<double> node_poses;
    for (const auto& id_data : node_data_) {
      node_index.emplace(id_data.first, static_cast<int32_t>(node_index.size()));
      const std::array<double, 7> pose = id_data.second.global_pose.ToArray();
      node_poses.insert(node_poses.end(), pose.begin(), pose.end());
    }
    const bool freeze_landmarks = !frozen_trajectories.empty();  // :169-174 with :343-345
    for (const auto& landmark_node : landmark_nodes) {
      // landmarks that were not optimized for localization are not used (:131-134)
      if (!landmark_node.second.global_landmark_pose.has_value() && freeze_landmarks) continue;
      bool added = false;
      for (const LandmarkNode::LandmarkObservation& observation : landmark_node.second.landmark_observations) {
        const auto begin_of_trajectory = node_data_.lower_bound(NodeId{observation.trajectory_id, 0});
        const auto end_of_trajectory = node_data_.lower_bound(NodeId{observation.trajectory_id + 1, 0});
        if (begin_of_trajectory == end_of_trajectory) continue;  // no node at all (the reference dereferences end() here)
        if (observation.time < begin_of_trajectory->second.time) continue;  // made before the trajectory was created
        auto next = begin_of_trajectory;  // MapById::lower_bound(trajectory, time): the first node not before the observation
        while (next != end_of_trajectory && next->second.time < observation.time) ++next;
        if (next == end_of_trajectory) continue;  // the next node has not been added yet
        if (next == begin_of_trajectory) next = std::next(next);
        if (next == end_of_trajectory) continue;  // a trajectory of one node has no pair (the reference dereferences end())
        const auto prev = std::prev(next);
        dliom_pose_graph_landmark_observation o = {};
        o.landmark = static_cast<int32_t>(landmark_ids.size()) - (added ? 1 : 0);
        o.prev_node = node_index.at(prev->first);
        o.next_node = node_index.at(next->first);
        // common::ToSeconds of both differences (landmark_cost_function_3d.h:85-87)
        o.interpolation_parameter = (static_cast<double>(observation.time - prev->second.time) / 1e7) /
                                    (static_cast<double>(next->second.time - prev->second.time) / 1e7);
        const std::array<double, 7> z = observation.landmark_to_tracking_transform.ToArray();
        for (int k = 0; k < 7; ++k) o.landmark_to_tracking7[k] = z[k];
        o.translation_weight = observation.translation_weight;
        o.rotation_weight = observation.rotation_weight;
        if (!added) {  // the block's start value: the stored pose, or the first used observation's (:158-168)
          std::array<double, 7> start;
          if (landmark_node.second.global_landmark_pose.has_value()) {
            start = landmark_node.second.global_landmark_pose.value().ToArray();
          } else {
            Check(dliom_pose_graph_initial_landmark_pose(&node_poses[7 * static_cast<size_t>(o.prev_node)],
                                                         &node_poses[7 * static_cast<size_t>(o.next_node)], o.interpolation_parameter,
                                                         o.landmark_to_tracking7, start.data()),
                  "dliom_pose_graph_initial_landmark_pose");
          }
          landmark_ids.push_back(landmark_node.first);
          landmark_poses.insert(landmark_poses.end(), start.begin(), start.end());
          landmark_constant.push_back(freeze_landmarks ? 1 : 0);
          added = true;
        }
        observations.push_back(o);
      }
    }
    return blocks;
  }

  const std::map<NodeId, NodeSpec3D>& node_data() const { return node_data_; }
  const std::map<SubmapId, SubmapSpec3D>& submap_data() const { return submap_data_; }
  const std::map<int, std::vector<sensor::ImuData>>& imu_data() const { return imu_data_; }
  const std::map<int, std::map<int64_t, sensor::FixedFramePoseData>>& fixed_frame_pose_data() const { return fixed_frame_pose_data_; }
  const std::map<int, TrajectoryData>& trajectory_data() const { return trajectory_data_; }
  const std::map<std::string, transform::Rigid3d>& landmark_data() const { return landmark_data_; }
  const dliom_pose_graph_summary& summary() const { return summary_; }  // of the last Solve (ceres::Solver::Summary there)

 private:
  template <typename Map, typename Id>
  static int NextIndex(const Map& map, const Id& first_of_trajectory, int Id::*index) {  // MapById::Append
    auto it = map.lower_bound(Id{first_of_trajectory.trajectory_id + 1, 0});
    if (it == map.begin()) return 0;
    --it;
    return it->first.trajectory_id == first_of_trajectory.trajectory_id ? it->first.*index + 1 : 0;
  }

  // :78-102: the fixed-frame pose at `time`, between the samples around it if both have a pose
  std::unique_ptr<transform::Rigid3d> Interpolate(int trajectory_id, int64_t time) const {
    const std::map<int64_t, sensor::FixedFramePoseData>& trajectory = fixed_frame_pose_data_.at(trajectory_id);
    const auto it = trajectory.lower_bound(time);
    if (it == trajectory.end() || !it->second.pose.has_value()) return nullptr;
    if (it == trajectory.begin()) {
      if (it->second.time == time) return std::unique_ptr<transform::Rigid3d>(new transform::Rigid3d(it->second.pose.value()));
      return nullptr;
    }
    const auto prev_it = std::prev(it);
    if (!prev_it->second.pose.has_value()) return nullptr;
    return std::unique_ptr<transform::Rigid3d>(new transform::Rigid3d(
        fixed_frame::Interpolate(prev_it->second.time, prev_it->second.pose.value(), it->second.time, it->second.pose.value(), time)));
  }
  // sensor::MapByTime::Trim (map_by_time.h:48-97): the data between the trimmed node's neighbours goes, but for the
  // first and the last of it, which interpolation with the data outside still needs
  void TrimFixedFramePoseData(std::map<NodeId, NodeSpec3D>::const_iterator node_it) {
    const int trajectory_id = node_it->first.trajectory_id;
    const auto found = fixed_frame_pose_data_.find(trajectory_id);
    if (found == fixed_frame_pose_data_.end()) return;
    const bool has_previous = node_it != node_data_.begin() && std::prev(node_it)->first.trajectory_id == trajectory_id;
    const auto next_it = std::next(node_it);
    const bool has_next = next_it != node_data_.end() && next_it->first.trajectory_id == trajectory_id;
    const int64_t gap_start = has_previous ? std::prev(node_it)->second.time : INT64_MIN;
    const int64_t gap_end = has_next ? next_it->second.time : INT64_MAX;
    if (!(gap_start < gap_end)) Check(DLIOM_ERR_INVALID_ARGUMENT, "TrimTrajectoryNode: CHECK_LT(gap_start, gap_end)");
    std::map<int64_t, sensor::FixedFramePoseData>& trajectory = found->second;
    auto data_it = trajectory.lower_bound(gap_start);
    auto data_end = trajectory.upper_bound(gap_end);
    if (data_it == data_end) return;
    if (has_next) {
      data_end = std::prev(data_end);
      if (data_it == data_end) return;
    }
    if (has_previous) data_it = std::next(data_it);
    while (data_it != data_end) data_it = trajectory.erase(data_it);
    if (trajectory.empty()) fixed_frame_pose_data_.erase(found);
  }

  Context* context_;
  OptimizationProblemOptions options_;
  std::map<int, std::map<int64_t, sensor::FixedFramePoseData>> fixed_frame_pose_data_;
  std::map<int, TrajectoryData> trajectory_data_;
  std::map<NodeId, NodeSpec3D> node_data_;
  std::map<SubmapId, SubmapSpec3D> submap_data_;
  std::map<int, std::vector<sensor::ImuData>> imu_data_;
  std::map<std::string, transform::Rigid3d> landmark_data_;
  dliom_pose_graph_summary summary_ = {};
};
}  // namespace optimization
}  // namespace mapping

// ---- submap feature matching (mapping/internal/constraints/constraint_builder_3d.cc:459-529) ----------------------------
namespace transform {
// transform::Embed3D(Rigid2d(translation, Rotation2D(theta))) (transform/transform.h): (x, y, 0) and a turn about z
inline Rigid3d Embed3D(double x, double y, double theta) {
  return Rigid3d(Vector3d{{x, y, 0.0}}, Quaterniond{{std::cos(0.5 * theta), 0.0, 0.0, std::sin(0.5 * theta)}});
}
}  // namespace transform
namespace mapping {
namespace constraints {
struct KeyPoint {  // cv::KeyPoint::pt, pixels
  float x, y;
};
static_assert(sizeof(KeyPoint) == 8, "packed xy like cv::Point2f");
struct FeatureMatchOptions {  // proto/constraint_builder_options.proto, the fields :485-513 read; seed: dliom.h
  double good_match_ratio_of_distance;
  int minimum_good_match_num;
  double ransac_thresh_of_2d_transform_estimate;
  double scale_estimated_tolerance;
  uint64_t seed = 0;
};
// The second half of ExtractFeaturesForSubmap: the submaps' key points and descriptors (what surf_detector_ produced, a
// continuous CV_32F cv::Mat's rows) stay on the device; AddSubmap returns the new submap's `matched_submaps`, the
// submap_to_submap_2D of the constraint queries.  Parity unpinned against OpenCV (dliom.h).
class SubmapFeatureMatcher {
 public:
  SubmapFeatureMatcher(Context* context, int descriptor_size) {
    Check(dliom_feature_index_create(context->get(), descriptor_size, &index_), "dliom_feature_index_create");
  }
  ~SubmapFeatureMatcher() { dliom_feature_index_destroy(index_); }
  SubmapFeatureMatcher(const SubmapFeatureMatcher&) = delete;
  SubmapFeatureMatcher& operator=(const SubmapFeatureMatcher&) = delete;

  // descriptors: key_points.size() rows of descriptor_size floats.  Matches against every stored submap but those of the
  // same trajectory within two submap indices (:470-473); a submap that was never added has no features and is not
  // matched (:467).  `results`, when given, receives every searched submap's dliom_submap_match.
  std::map<SubmapId, transform::Rigid3d> AddSubmap(const SubmapId& submap_id, const std::vector<KeyPoint>& key_points,
                                                   const float* descriptors, double ox, double oy, double resolution,
                                                   const FeatureMatchOptions& options,
                                                   std::map<SubmapId, dliom_submap_match>* results = nullptr) {
    const std::vector<SubmapId> searched = Searched(submap_id);
    Check(dliom_feature_index_add(index_, Key(submap_id), descriptors, key_points.empty() ? nullptr : &key_points[0].x,
                                  static_cast<int32_t>(key_points.size()), ox, oy, resolution),
          "dliom_feature_index_add");
    return MatchStored(submap_id, searched, options, results);
  }
  // The whole of ExtractFeaturesForSubmap (:436-532) from the finished submap's high resolution grid: ProjectToCvMat,
  // cv::threshold, cv::erode and SURF (dliom.h "submap image features") run on the device and the features go straight
  // into the index (dliom_feature_index_add_from_grid); the matcher must have descriptor size 64 and the grid's context.
  // Replaces :442-458 and the overload above at the call site.  Parity unpinned against OpenCV (dliom.h).
  std::map<SubmapId, transform::Rigid3d> AddSubmap(const SubmapId& submap_id, const HybridGrid& high_resolution_hybrid_grid,
                                                   const transform::Rigid3d& global_submap_pose,
                                                   const dliom_surf_options& surf_options, const FeatureMatchOptions& options,
                                                   std::map<SubmapId, dliom_submap_match>* results = nullptr) {
    const std::vector<SubmapId> searched = Searched(submap_id);
    const std::array<double, 7> pose = global_submap_pose.ToArray();
    Check(dliom_feature_index_add_from_grid(index_, Key(submap_id), high_resolution_hybrid_grid.get(), pose.data(), &surf_options,
                                            nullptr, nullptr, nullptr, nullptr),
          "dliom_feature_index_add_from_grid");
    return MatchStored(submap_id, searched, options, results);
  }
  // ConstraintBuilder3D::DeleteScanMatcher: the submap's features leave the device
  void DeleteSubmap(const SubmapId& submap_id) {
    if (stored_.erase(submap_id) != 0) Check(dliom_feature_index_remove(index_, Key(submap_id)), "dliom_feature_index_remove");
  }
  const dliom_feature_match_stats& stats() const { return stats_; }  // of the last AddSubmap

 private:
  static int64_t Key(const SubmapId& id) {
    return static_cast<int64_t>((static_cast<uint64_t>(static_cast<uint32_t>(id.trajectory_id)) << 32) |
                                static_cast<uint32_t>(id.submap_index));
  }
  // every stored submap but those of the same trajectory within two submap indices (:470-473)
  std::vector<SubmapId> Searched(const SubmapId& submap_id) const {
    std::vector<SubmapId> searched;
    for (const SubmapId& id : stored_) {
      if (id.trajectory_id == submap_id.trajectory_id && std::abs(submap_id.submap_index - id.submap_index) <= 2) continue;
      searched.push_back(id);
    }
    return searched;
  }
  // the submap's set is in the index: record it and match it against `searched`
  std::map<SubmapId, transform::Rigid3d> MatchStored(const SubmapId& submap_id, const std::vector<SubmapId>& searched,
                                                     const FeatureMatchOptions& options,
                                                     std::map<SubmapId, dliom_submap_match>* results) {
    std::vector<int64_t> keys;
    for (const SubmapId& id : searched) keys.push_back(Key(id));
    stored_.insert(submap_id);
    const dliom_feature_match_options o{options.good_match_ratio_of_distance, options.minimum_good_match_num, 0,
                                        options.ransac_thresh_of_2d_transform_estimate, options.scale_estimated_tolerance,
                                        options.seed};
    std::vector<dliom_submap_match> matches(searched.size());
    Check(dliom_feature_index_match(index_, Key(submap_id), keys.data(), static_cast<int>(keys.size()), &o, matches.data(),
                                    &stats_),
          "dliom_feature_index_match");
    std::map<SubmapId, transform::Rigid3d> matched_submaps;
    for (size_t k = 0; k < searched.size(); ++k) {
      if (results != nullptr) (*results)[searched[k]] = matches[k];
      if (matches[k].status == DLIOM_FEATURE_MATCHED)
        matched_submaps.insert({searched[k], transform::Embed3D(matches[k].tx, matches[k].ty, matches[k].theta)});
    }
    return matched_submaps;
  }
  dliom_feature_index* index_ = nullptr;
  std::set<SubmapId> stored_;
  dliom_feature_match_stats stats_ = {};
};
}  // namespace constraints
}  // namespace mapping

namespace mapping {
struct Timespan {  // mapping/detect_floors.h:27-30, common::Time as ticks
  int64_t start = 0, end = 0;
};
struct Floor {  // mapping/detect_floors.h:32-40
  std::vector<Timespan> timespans;
  double z = 0.0;
};
}  // namespace mapping

namespace transform {
// transform/transform_interpolation_buffer.{h,cc}, common::Time as ticks: the class surface of the reference.  Has and
// the time getters read the pushed times; Lookup goes through a host-only dliom_trajectory, so that a buffer that is only
// asked on the host opens no device context.  io::AssemblePointsBatch reads trajectory(), the same nodes on the buffer's
// context (the calling thread's, unless one was given), created on first use.  Both are immutable arrays that a Push
// drops and the next use makes again -- with acos / sin per interval, O(n) each time: push the trajectory first, then
// look up or assemble, as the assets writer does; interleaving Push with Lookup costs O(n^2).
class TransformInterpolationBuffer {
 public:
  explicit TransformInterpolationBuffer(Context* context = nullptr) : context_(context) {}
  ~TransformInterpolationBuffer() { Drop(); }
  TransformInterpolationBuffer(const TransformInterpolationBuffer&) = delete;
  TransformInterpolationBuffer& operator=(const TransformInterpolationBuffer&) = delete;

  void Push(int64_t time, const Rigid3d& transform) {
    if (!times_.empty() && time < times_.back()) {
      std::fprintf(stderr, "Check failed: time >= latest_time() New transform is older than latest.\n");
      std::abort();
    }
    times_.push_back(time);
    const std::array<double, 7> pose = transform.ToArray();
    poses_.insert(poses_.end(), pose.begin(), pose.end());
    Drop();
  }
  bool Has(int64_t time) const { return !times_.empty() && times_.front() <= time && time <= times_.back(); }
  Rigid3d Lookup(int64_t time) const {
    int has = 0;
    double pose[7];
    if (host_ == nullptr) Create(nullptr, &host_);
    Check(dliom_trajectory_lookup(host_, time, &has, pose), "dliom_trajectory_lookup");
    if (has == 0) {
      std::fprintf(stderr, "Check failed: Has(time) Missing transform for: %lld\n", static_cast<long long>(time));
      std::abort();
    }
    return Rigid3d::FromArray(pose);
  }
  int64_t earliest_time() const {
    CheckNotEmpty();
    return times_.front();
  }
  int64_t latest_time() const {
    CheckNotEmpty();
    return times_.back();
  }
  bool empty() const { return times_.empty(); }

  Context* context() const {
    if (context_ == nullptr) context_ = Context::ForThisThread();
    return context_;
  }
  // the nodes pushed so far as a dliom_trajectory of context() (valid until the next Push)
  dliom_trajectory* trajectory() const {
    if (device_ == nullptr) Create(context()->get(), &device_);
    return device_;
  }

 private:
  void Create(dliom_ctx* ctx, dliom_trajectory** out) const {
    Check(dliom_trajectory_create(ctx, times_.data(), poses_.data(), static_cast<int64_t>(times_.size()), out),
          "dliom_trajectory_create");
  }
  void CheckNotEmpty() const {
    if (!times_.empty()) return;
    std::fprintf(stderr, "Check failed: !empty() Empty buffer.\n");
    std::abort();
  }
  void Drop() {
    if (host_ != nullptr) dliom_trajectory_destroy(host_);
    if (device_ != nullptr) dliom_trajectory_destroy(device_);
    host_ = device_ = nullptr;
  }
  mutable Context* context_;
  std::vector<int64_t> times_;
  std::vector<double> poses_;
  mutable dliom_trajectory* host_ = nullptr;
  mutable dliom_trajectory* device_ = nullptr;
};
}  // namespace transform

// The points-processor pipeline's stages with compute in them (cartographer/io), on the device.  A batch that arrives as
// host vectors goes to the device once per stage and phase, its intensities and colors stay on the host and are filtered
// with the survivors' indices, as RemovePoints does (io/points_batch.cc:22-49).  A batch that carries a device_batch
// (AssemblePointsBatch(kOnDevice, ...), or any stage that made one) lives in HBM with its attributes: the stages rewrite it
// there and pass it on; the host vectors are refreshed only by internal::SyncToHost.
namespace io {

using FloatColor = std::array<float, 3>;  // io/color.h:30

namespace internal {
struct DeviceCloud;
struct DeviceBatch;
}
struct PointsBatch {  // io/points_batch.h:36-73: the fields the stages here touch
  sensor::Vector3f origin{0.f, 0.f, 0.f};
  std::vector<sensor::Vector3f> points;  // in the map frame
  std::vector<float> intensities;        // optional
  std::vector<FloatColor> colors;        // optional
  int64_t start_time = 0;                // common::Time (ticks) of the batch's first point (:41)
  std::string frame_id;                  // the sensor's frame, or empty (:49)
  // Not in the reference: `points` as a stage left them on the device (the range filter and the outlier remover set it),
  // so that the next device stage does not upload them again.  Whoever changes `points` resets it (KeepPoints does).
  std::shared_ptr<internal::DeviceCloud> device_points;
  // Not in the reference: the whole batch (points, intensities, colors) in HBM.  While its host_stale is set it alone is
  // the batch and the three vectors above are out of date (internal::SyncToHost brings them back); otherwise it mirrors
  // them and is valid like device_points: same context, same size.  A stage that rewrites a host vector resets it.
  std::shared_ptr<internal::DeviceBatch> device_batch;
};

class PointsProcessor {  // io/points_processor.h:29-52
 public:
  enum class FlushResult { kRestartStream, kFinished };
  PointsProcessor() {}
  virtual ~PointsProcessor() {}
  PointsProcessor(const PointsProcessor&) = delete;
  PointsProcessor& operator=(const PointsProcessor&) = delete;
  virtual void Process(std::unique_ptr<PointsBatch> points_batch) = 0;
  virtual FlushResult Flush() = 0;
};

namespace internal {
struct DeviceCloud {
  // clouds this process has uploaded from host points so far (a stage that reuses device_points adds nothing)
  static std::atomic<int64_t>& Uploads() {
    static std::atomic<int64_t> uploads{0};
    return uploads;
  }
  DeviceCloud(Context* context, const std::vector<sensor::Vector3f>& points) : context(context) {
    ++Uploads();
    Check(dliom_cloud_create(context->get(), points.empty() ? nullptr : &points[0].x, static_cast<int64_t>(points.size()), &cloud),
          "dliom_cloud_create");
  }
  DeviceCloud(Context* context, dliom_cloud* owned) : context(context), cloud(owned) {}  // takes a cloud a filter made
  ~DeviceCloud() { dliom_cloud_destroy(cloud); }
  DeviceCloud(const DeviceCloud&) = delete;
  DeviceCloud& operator=(const DeviceCloud&) = delete;
  Context* const context;  // the context the cloud lives on
  dliom_cloud* cloud = nullptr;
};
struct DeviceBatch {
  // bytes of batch contents brought back to the host so far: SyncToHost's vectors and the writers' packed records
  static std::atomic<int64_t>& DownloadedBytes() {
    static std::atomic<int64_t> bytes{0};
    return bytes;
  }
  DeviceBatch(Context* context, dliom_points_batch* owned, bool host_stale) : context(context), batch(owned), host_stale(host_stale) {}
  ~DeviceBatch() { dliom_points_batch_destroy(batch); }
  DeviceBatch(const DeviceBatch&) = delete;
  DeviceBatch& operator=(const DeviceBatch&) = delete;
  int64_t size() const {
    int64_t n = 0;
    Check(dliom_points_batch_size(batch, &n), "dliom_points_batch_size");
    return n;
  }
  const dliom_cloud* cloud() const {
    const dliom_cloud* c = nullptr;
    Check(dliom_points_batch_cloud(batch, &c), "dliom_points_batch_cloud");
    return c;
  }
  Context* const context;
  dliom_points_batch* batch = nullptr;
  bool host_stale;  // the PointsBatch's vectors do not hold what the device batch holds
};
// The batch's device_batch if a stage on `context` may use it, else null
inline DeviceBatch* BatchOnDevice(Context* context, const PointsBatch& batch) {
  DeviceBatch* d = batch.device_batch.get();
  if (d == nullptr || d->context != context) return nullptr;
  if (!d->host_stale && d->size() != static_cast<int64_t>(batch.points.size())) return nullptr;
  return d;
}
// points, intensities and colors := the device batch's (one download each); a no-op unless they are stale
inline void SyncToHost(PointsBatch* batch) {
  DeviceBatch* d = batch->device_batch.get();
  if (d == nullptr || !d->host_stale) return;
  const size_t n = static_cast<size_t>(d->size());
  int has_intensities = 0, has_colors = 0;
  Check(dliom_points_batch_has_intensities(d->batch, &has_intensities), "dliom_points_batch_has_intensities");
  Check(dliom_points_batch_has_colors(d->batch, &has_colors), "dliom_points_batch_has_colors");
  batch->points.assign(n, sensor::Vector3f(0.f, 0.f, 0.f));
  batch->intensities.assign(has_intensities ? n : 0, 0.f);
  batch->colors.assign(has_colors ? n : 0, FloatColor{{0.f, 0.f, 0.f}});
  if (n > 0)
    Check(dliom_points_batch_download(d->batch, &batch->points[0].x, has_intensities ? batch->intensities.data() : nullptr,
                                      has_colors ? batch->colors[0].data() : nullptr),
          "dliom_points_batch_download");
  DeviceBatch::DownloadedBytes() += static_cast<int64_t>(n * (12 + (has_intensities ? 4 : 0) + (has_colors ? 12 : 0)));
  batch->device_points.reset();
  d->host_stale = false;
}
// What a stage that works on the host vectors calls first: they are brought up to date and the device batch is dropped
inline void UseHostVectors(PointsBatch* batch) {
  SyncToHost(batch);
  batch->device_batch.reset();
}
// The batch in HBM on `context`: what it carries, else made from the host vectors (one upload of each)
inline DeviceBatch* EnsureOnDevice(Context* context, PointsBatch* batch) {
  if (DeviceBatch* d = BatchOnDevice(context, *batch)) return d;
  UseHostVectors(batch);
  if ((!batch->intensities.empty() && batch->intensities.size() != batch->points.size()) ||
      (!batch->colors.empty() && batch->colors.size() != batch->points.size()))
    Check(DLIOM_ERR_INVALID_ARGUMENT, "PointsBatch: an attribute vector that is neither empty nor of the points' size");
  const float origin[3] = {batch->origin.x, batch->origin.y, batch->origin.z};
  dliom_points_batch* made = nullptr;
  Check(dliom_points_batch_create(context->get(), batch->points.empty() ? nullptr : &batch->points[0].x,
                                  static_cast<int64_t>(batch->points.size()), origin,
                                  batch->intensities.empty() ? nullptr : batch->intensities.data(),
                                  batch->colors.empty() ? nullptr : batch->colors[0].data(), static_cast<int64_t>(batch->colors.size()),
                                  &made),
        "dliom_points_batch_create");
  batch->device_batch = std::make_shared<DeviceBatch>(context, made, false);
  return batch->device_batch.get();
}
// RemovePoints with the complement: the batch keeps the points of `kept` (a device cloud of kept_index.size() points)
inline void KeepPoints(dliom_cloud* kept, const std::vector<int32_t>& kept_index, PointsBatch* batch) {
  std::vector<sensor::Vector3f> points(kept_index.size());
  if (!points.empty()) Check(dliom_cloud_download(kept, &points[0].x), "dliom_cloud_download");
  std::vector<float> intensities;
  std::vector<FloatColor> colors;
  if (!batch->intensities.empty())
    for (const int32_t i : kept_index) intensities.push_back(batch->intensities[i]);
  if (!batch->colors.empty())
    for (const int32_t i : kept_index) colors.push_back(batch->colors[i]);
  batch->points = std::move(points);
  batch->intensities = std::move(intensities);
  batch->colors = std::move(colors);
  batch->device_points.reset();
  batch->device_batch.reset();
}
// The batch's points on the device: what the stage before left there -- on this context, and of the batch's size --, else
// one upload.  (A stage that rewrites `points` in place without changing their number must reset device_points itself.)
inline std::shared_ptr<DeviceCloud> PointsOnDevice(Context* context, const PointsBatch& batch) {
  int64_t n = -1;
  if (batch.device_points != nullptr && batch.device_points->context == context &&
      dliom_cloud_size(batch.device_points->cloud, &n) == DLIOM_OK &&
      n == static_cast<int64_t>(batch.points.size()))
    return batch.device_points;
  return std::make_shared<DeviceCloud>(context, batch.points);
}
}  // namespace internal

// io/min_max_range_filtering_points_processor.{h,cc}
class MinMaxRangeFiteringPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "min_max_range_filter";
  MinMaxRangeFiteringPointsProcessor(double min_range, double max_range, PointsProcessor* next, Context* context = nullptr)
      : min_range_(min_range), max_range_(max_range), next_(next), context_(context != nullptr ? context : Context::ForThisThread()) {}

  void Process(std::unique_ptr<PointsBatch> batch) override {
    if (internal::DeviceBatch* d = internal::BatchOnDevice(context_, *batch)) {  // compacted where it is: one count comes back
      Check(dliom_points_batch_min_max_range_filter(d->batch, min_range_, max_range_), "dliom_points_batch_min_max_range_filter");
      d->host_stale = true;
      next_->Process(std::move(batch));
      return;
    }
    internal::UseHostVectors(batch.get());
    const std::shared_ptr<internal::DeviceCloud> in = internal::PointsOnDevice(context_, *batch);
    std::vector<int32_t> kept_index(batch->points.size());
    dliom_cloud* kept = nullptr;
    int64_t num_kept = 0;
    const float origin[3] = {batch->origin.x, batch->origin.y, batch->origin.z};
    Check(dliom_cloud_min_max_range_filter(context_->get(), in->cloud, origin, min_range_, max_range_, &kept, kept_index.data(),
                                           static_cast<int64_t>(kept_index.size()), &num_kept),
          "dliom_cloud_min_max_range_filter");
    kept_index.resize(static_cast<size_t>(num_kept));
    internal::KeepPoints(kept, kept_index, batch.get());
    batch->device_points = std::make_shared<internal::DeviceCloud>(context_, kept);  // the next device stage reads them there
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override { return next_->Flush(); }

 private:
  const double min_range_, max_range_;
  PointsProcessor* const next_;
  Context* const context_;
};

// HandleMessage (cartographer_ros/assets_writer.cc:119-160) behind the message decoding: the batch of one message from its
// points in the sensor frame (x, y, z, time relative to cloud_time), assembled on the device.  Null when no point's time
// lies on the trajectory, as in the reference.  `points` are downloaded once; the assembled cloud stays in device_points,
// so that the device stages behind upload nothing.  sensor_to_tracking: one transform for the message (the reference asks
// a tf buffer per point, which holds the URDF's static transforms only).
inline std::unique_ptr<PointsBatch> AssemblePointsBatch(const transform::TransformInterpolationBuffer& buffer, int64_t cloud_time,
                                                        const sensor::TimedPointCloud& points_xyzt,
                                                        const std::vector<float>& intensities,
                                                        const transform::Rigid3d& sensor_to_tracking, const std::string& frame_id,
                                                        Context* context = nullptr) {
  if (context == nullptr) context = buffer.context();
  if (!intensities.empty() && intensities.size() != points_xyzt.size())
    Check(DLIOM_ERR_INVALID_ARGUMENT, "AssemblePointsBatch: CHECK_EQ(intensities.size(), points.size())");
  std::vector<int32_t> kept_index(points_xyzt.size());
  dliom_cloud* cloud = nullptr;
  int64_t num_kept = 0;
  float origin[3] = {0.f, 0.f, 0.f};
  const std::array<double, 7> mount = sensor_to_tracking.ToArray();
  Check(dliom_cloud_from_sensor_points(context->get(), buffer.trajectory(), cloud_time,
                                       points_xyzt.empty() ? nullptr : &points_xyzt[0].x, static_cast<int64_t>(points_xyzt.size()),
                                       mount.data(), &cloud, origin, kept_index.data(), static_cast<int64_t>(kept_index.size()),
                                       &num_kept),
        "dliom_cloud_from_sensor_points");
  if (cloud == nullptr) return nullptr;
  std::unique_ptr<PointsBatch> batch(new PointsBatch);
  batch->start_time = cloud_time;
  batch->frame_id = frame_id;
  batch->origin = sensor::Vector3f(origin[0], origin[1], origin[2]);
  batch->points.resize(static_cast<size_t>(num_kept));
  Check(dliom_cloud_download(cloud, &batch->points[0].x), "dliom_cloud_download");
  if (!intensities.empty())
    for (int64_t i = 0; i < num_kept; ++i) batch->intensities.push_back(intensities[kept_index[static_cast<size_t>(i)]]);
  batch->device_points = std::make_shared<internal::DeviceCloud>(context, cloud);
  return batch;
}

// The same batch left in HBM: points and intensities never visit the host (batch->points stays empty until
// internal::SyncToHost; batch->device_batch is the batch).  The message's intensities are uploaded once.
struct OnDevice {};
constexpr OnDevice kOnDevice{};
inline std::unique_ptr<PointsBatch> AssemblePointsBatch(OnDevice, const transform::TransformInterpolationBuffer& buffer,
                                                        int64_t cloud_time, const sensor::TimedPointCloud& points_xyzt,
                                                        const std::vector<float>& intensities,
                                                        const transform::Rigid3d& sensor_to_tracking, const std::string& frame_id,
                                                        Context* context = nullptr) {
  if (context == nullptr) context = buffer.context();
  if (!intensities.empty() && intensities.size() != points_xyzt.size())
    Check(DLIOM_ERR_INVALID_ARGUMENT, "AssemblePointsBatch: CHECK_EQ(intensities.size(), points.size())");
  const std::array<double, 7> mount = sensor_to_tracking.ToArray();
  dliom_points_batch* made = nullptr;
  Check(dliom_points_batch_from_sensor_points(context->get(), buffer.trajectory(), cloud_time,
                                              points_xyzt.empty() ? nullptr : &points_xyzt[0].x,
                                              intensities.empty() ? nullptr : intensities.data(),
                                              static_cast<int64_t>(points_xyzt.size()), mount.data(), &made),
        "dliom_points_batch_from_sensor_points");
  if (made == nullptr) return nullptr;
  std::unique_ptr<PointsBatch> batch(new PointsBatch);
  batch->start_time = cloud_time;
  batch->frame_id = frame_id;
  float origin[3];
  Check(dliom_points_batch_origin(made, origin), "dliom_points_batch_origin");
  batch->origin = sensor::Vector3f(origin[0], origin[1], origin[2]);
  batch->device_batch = std::make_shared<internal::DeviceBatch>(context, made, true);
  return batch;
}

// HandleMessage (assets_writer.cc:119-160) from the message itself: ToPointCloudWithIntensities, or with rslidar
// ToPointCloudWithIntensitiesRsLiDAR (msg_conversion.cc:185-226), decoded on the device in the sensor frame and assembled
// there -- points and intensities are uploaded once, as the message's bytes, and never visit the host.  Null when no point's
// time lies on the trajectory.
inline std::unique_ptr<PointsBatch> HandleMessage(const sensor_msgs::PointCloud2& message, bool rslidar,
                                                  const transform::TransformInterpolationBuffer& buffer,
                                                  const transform::Rigid3d& sensor_to_tracking, Context* context = nullptr) {
  if (context == nullptr) context = buffer.context();
  const sensor::TimedCloudOnDevice decoded(context, message, rslidar ? DLIOM_POINT_CLOUD2_EXPORT_RSLIDAR : DLIOM_POINT_CLOUD2_EXPORT,
                                           nullptr);
  const std::array<double, 7> mount = sensor_to_tracking.ToArray();
  dliom_points_batch* made = nullptr;
  Check(dliom_points_batch_from_timed_cloud(context->get(), buffer.trajectory(), decoded.time(), decoded.get(), mount.data(), &made),
        "dliom_points_batch_from_timed_cloud");
  if (made == nullptr) return nullptr;
  std::unique_ptr<PointsBatch> batch(new PointsBatch);
  batch->start_time = decoded.time();
  batch->frame_id = message.header.frame_id;
  float origin[3];
  Check(dliom_points_batch_origin(made, origin), "dliom_points_batch_origin");
  batch->origin = sensor::Vector3f(origin[0], origin[1], origin[2]);
  batch->device_batch = std::make_shared<internal::DeviceBatch>(context, made, true);
  return batch;
}

// io/fixed_ratio_sampling_points_processor.{h,cc} over common::FixedRatioSampler: "fixed_ratio_sampler".  One sampler
// state whichever way a batch arrives: host vectors go to the device for the call and come back.
class FixedRatioSamplingPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "fixed_ratio_sampler";
  FixedRatioSamplingPointsProcessor(double sampling_ratio, PointsProcessor* next, Context* context = nullptr)
      : next_(next), context_(context != nullptr ? context : Context::ForThisThread()) {
    Check(dliom_fixed_ratio_sampler_create(sampling_ratio, &sampler_), "dliom_fixed_ratio_sampler_create");
  }
  ~FixedRatioSamplingPointsProcessor() override { dliom_fixed_ratio_sampler_destroy(sampler_); }

  void Process(std::unique_ptr<PointsBatch> batch) override {  // .cc:43-53
    const bool arrived_on_host = internal::BatchOnDevice(context_, *batch) == nullptr || !batch->device_batch->host_stale;
    internal::DeviceBatch* d = internal::EnsureOnDevice(context_, batch.get());
    Check(dliom_points_batch_fixed_ratio_sample(sampler_, d->batch), "dliom_points_batch_fixed_ratio_sample");
    d->host_stale = true;
    if (arrived_on_host) internal::SyncToHost(batch.get());  // a host-vector caller finds its vectors sampled
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override {  // .cc:55-66
    switch (next_->Flush()) {
      case FlushResult::kFinished:
        return FlushResult::kFinished;
      case FlushResult::kRestartStream:
        Check(dliom_fixed_ratio_sampler_reset(sampler_), "dliom_fixed_ratio_sampler_reset");  // a new FixedRatioSampler
        return FlushResult::kRestartStream;
    }
    std::abort();
  }
  const dliom_fixed_ratio_sampler* sampler() const { return sampler_; }

 private:
  PointsProcessor* const next_;
  Context* const context_;
  dliom_fixed_ratio_sampler* sampler_ = nullptr;
};

// io/outlier_removing_points_processor.{h,cc}: "voxel_filter_and_remove_moving_objects"
class OutlierRemovingPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "voxel_filter_and_remove_moving_objects";
  OutlierRemovingPointsProcessor(double voxel_size, PointsProcessor* next, Context* context = nullptr)
      : next_(next), context_(context != nullptr ? context : Context::ForThisThread()) {
    Check(dliom_outlier_remover_create(context_->get(), voxel_size, &remover_), "dliom_outlier_remover_create");
  }
  ~OutlierRemovingPointsProcessor() override { dliom_outlier_remover_destroy(remover_); }

  void Process(std::unique_ptr<PointsBatch> batch) override {  // .cc:45-61
    const float origin[3] = {batch->origin.x, batch->origin.y, batch->origin.z};
    if (internal::DeviceBatch* d = internal::BatchOnDevice(context_, *batch)) {
      switch (state_) {
        case State::kPhase1:
          Check(dliom_outlier_remover_mark_hits(remover_, d->cloud()), "dliom_outlier_remover_mark_hits");
          break;
        case State::kPhase2:
          Check(dliom_outlier_remover_count_rays(remover_, origin, d->cloud()), "dliom_outlier_remover_count_rays");
          break;
        case State::kPhase3:
          Check(dliom_outlier_remover_filter_batch(remover_, d->batch), "dliom_outlier_remover_filter_batch");
          d->host_stale = true;
          next_->Process(std::move(batch));
          break;
      }
      return;
    }
    internal::UseHostVectors(batch.get());
    const std::shared_ptr<internal::DeviceCloud> points = internal::PointsOnDevice(context_, *batch);
    const internal::DeviceCloud& in = *points;
    switch (state_) {
      case State::kPhase1:
        Check(dliom_outlier_remover_mark_hits(remover_, in.cloud), "dliom_outlier_remover_mark_hits");
        break;
      case State::kPhase2:
        Check(dliom_outlier_remover_count_rays(remover_, origin, in.cloud), "dliom_outlier_remover_count_rays");
        break;
      case State::kPhase3: {
        std::vector<int32_t> kept_index(batch->points.size());
        dliom_cloud* kept = nullptr;
        int64_t num_kept = 0;
        Check(dliom_outlier_remover_filter(remover_, in.cloud, &kept, kept_index.data(), static_cast<int64_t>(kept_index.size()),
                                           &num_kept),
              "dliom_outlier_remover_filter");
        kept_index.resize(static_cast<size_t>(num_kept));
        internal::KeepPoints(kept, kept_index, batch.get());
        batch->device_points = std::make_shared<internal::DeviceCloud>(context_, kept);
        next_->Process(std::move(batch));
        break;
      }
    }
  }

  FlushResult Flush() override {  // .cc:63-82
    switch (state_) {
      case State::kPhase1:
        state_ = State::kPhase2;
        return FlushResult::kRestartStream;
      case State::kPhase2:
        state_ = State::kPhase3;
        return FlushResult::kRestartStream;
      case State::kPhase3:
        if (next_->Flush() != FlushResult::kFinished) {
          std::fprintf(stderr, "Check failed: Voxel filtering and outlier removal must be configured to occur after any "
                               "stages that require multiple passes.\n");
          std::abort();
        }
        return FlushResult::kFinished;
    }
    std::abort();
  }

  const dliom_outlier_remover* remover() const { return remover_; }

 private:
  enum class State { kPhase1, kPhase2, kPhase3 };
  PointsProcessor* const next_;
  Context* const context_;
  State state_ = State::kPhase1;
  dliom_outlier_remover* remover_ = nullptr;
};

// io/file_writer.h:31-50, the part the map writers use
class FileWriter {
 public:
  FileWriter() {}
  virtual ~FileWriter() {}
  FileWriter(const FileWriter&) = delete;
  FileWriter& operator=(const FileWriter&) = delete;
  virtual bool Write(const char* data, size_t len) = 0;
  // Overwrites the start of the file (io/file_writer.h:43: the PLY / PCD writers' placeholder header and its final form).
  // Not pure, unlike the reference's: the map writers' FileWriters never needed it.
  virtual bool WriteHeader(const char* /*data*/, size_t /*len*/) { return false; }
  virtual bool Close() = 0;
  virtual std::string GetFilename() = 0;
};
using FileWriterFactory = std::function<std::unique_ptr<FileWriter>(const std::string& filename)>;

struct ProbabilityGridRangeDataInserterOptions2D {  // proto/2d/probability_grid_range_data_inserter_options_2d.proto
  double hit_probability = 0.55;
  double miss_probability = 0.49;
  bool insert_free_space = true;
};

namespace internal {
// What both map stages hold: CreateProbabilityGrid(resolution) (io/probability_grid_points_processor.cc:150-158) and a
// ProbabilityGridRangeDataInserter2D, on the device.
class ProbabilityGridOnDevice {
 public:
  ProbabilityGridOnDevice(double resolution, const ProbabilityGridRangeDataInserterOptions2D& options, Context* context)
      : context_(context) {
    Check(dliom_probability_grid_create(context_->get(), resolution, 0, &grid_), "dliom_probability_grid_create");
    Check(dliom_inserter2d_create(context_->get(), options.hit_probability, options.miss_probability,
                                  options.insert_free_space ? 1 : 0, &inserter_),
          "dliom_inserter2d_create");
  }
  ~ProbabilityGridOnDevice() {
    dliom_inserter2d_destroy(inserter_);
    dliom_probability_grid_destroy(grid_);
  }
  ProbabilityGridOnDevice(const ProbabilityGridOnDevice&) = delete;
  ProbabilityGridOnDevice& operator=(const ProbabilityGridOnDevice&) = delete;

  // range_data_inserter_.Insert({batch->origin, batch->points, {}}, &probability_grid_)
  void Insert(const PointsBatch& batch) {
    const float origin[3] = {batch.origin.x, batch.origin.y, batch.origin.z};
    if (const DeviceBatch* d = BatchOnDevice(context_, batch)) {
      Check(dliom_inserter2d_insert_cloud(inserter_, grid_, origin, d->cloud()), "dliom_inserter2d_insert_cloud");
      return;
    }
    PointsBatch synced;  // (a device batch of another context: its points by way of the host)
    const PointsBatch* host = &batch;
    if (batch.device_batch != nullptr && batch.device_batch->host_stale) {
      synced.device_batch = batch.device_batch;
      SyncToHost(&synced);
      synced.device_batch.reset();
      host = &synced;
    }
    const std::shared_ptr<DeviceCloud> points = PointsOnDevice(context_, *host);
    Check(dliom_inserter2d_insert_cloud(inserter_, grid_, origin, points->cloud), "dliom_inserter2d_insert_cloud");
  }
  // DrawProbabilityGrid (:127-148), rotated by Image::Rotate90DegreesClockwise if asked: the gray bytes, row-major
  std::vector<uint8_t> Draw(bool rotate_cw, int32_t offset[2], int32_t size[2]) const {
    Check(dliom_probability_grid_draw(grid_, nullptr, 0, offset, size, rotate_cw ? 1 : 0), "dliom_probability_grid_draw");
    std::vector<uint8_t> gray(static_cast<size_t>(size[0]) * static_cast<size_t>(size[1]));
    Check(dliom_probability_grid_draw(grid_, gray.data(), static_cast<int64_t>(gray.size()), offset, size, rotate_cw ? 1 : 0),
          "dliom_probability_grid_draw");
    return gray;
  }
  const dliom_probability_grid* grid() const { return grid_; }

 private:
  Context* const context_;
  dliom_probability_grid* grid_ = nullptr;
  dliom_inserter2d* inserter_ = nullptr;
};

inline PointsProcessor::FlushResult FlushLastStage(PointsProcessor* next, const char* message) {
  switch (next->Flush()) {
    case PointsProcessor::FlushResult::kRestartStream:
      std::fprintf(stderr, "Check failed: %s\n", message);  // LOG(FATAL)
      std::abort();
    case PointsProcessor::FlushResult::kFinished:
      return PointsProcessor::FlushResult::kFinished;
  }
  std::abort();
}
}  // namespace internal

// io/probability_grid_points_processor.{h,cc}: "write_probability_grid".  Flush hands the gray image of
// DrawProbabilityGrid to `sink` (row-major, one byte a pixel, with its width, height and the offset of its first pixel in
// the grid); PNG encoding and cairo's trajectory drawing stay with the caller (DrawTrajectories::kNo).
class ProbabilityGridPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "write_probability_grid";
  using ImageSink = std::function<void(const std::vector<uint8_t>& gray, int width, int height, const int32_t offset[2])>;
  ProbabilityGridPointsProcessor(double resolution, const ProbabilityGridRangeDataInserterOptions2D& options, ImageSink sink,
                                 PointsProcessor* next, Context* context = nullptr)
      : sink_(std::move(sink)), next_(next), grid_(resolution, options, context != nullptr ? context : Context::ForThisThread()) {}

  void Process(std::unique_ptr<PointsBatch> batch) override {  // .cc:92-97
    grid_.Insert(*batch);
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override {  // .cc:99-125
    int32_t offset[2], size[2];
    const std::vector<uint8_t> gray = grid_.Draw(false, offset, size);
    sink_(gray, size[0], size[1], offset);
    return internal::FlushLastStage(next_, "ProbabilityGrid generation must be configured to occur after any stages that "
                                           "require multiple passes.");
  }
  const dliom_probability_grid* grid() const { return grid_.grid(); }

 private:
  ImageSink sink_;
  PointsProcessor* const next_;
  internal::ProbabilityGridOnDevice grid_;
};

// cartographer_ros/ros_map_writing_points_processor.{h,cc} with ros_map.cc: "write_ros_map"
class RosMapWritingPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "write_ros_map";
  RosMapWritingPointsProcessor(double resolution, const ProbabilityGridRangeDataInserterOptions2D& options,
                               FileWriterFactory file_writer_factory, const std::string& filestem, PointsProcessor* next,
                               Context* context = nullptr)
      : filestem_(filestem),
        next_(next),
        file_writer_factory_(std::move(file_writer_factory)),
        grid_(resolution, options, context != nullptr ? context : Context::ForThisThread()) {}

  void Process(std::unique_ptr<PointsBatch> batch) override {  // .cc:52-57
    grid_.Insert(*batch);
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override {  // .cc:59-94
    int32_t offset[2], size[2];
    const std::vector<uint8_t> gray = grid_.Draw(true, offset, size);  // image->Rotate90DegreesClockwise()
    double resolution, max_xy[2];
    int32_t num_cells[2];
    Check(dliom_probability_grid_limits(grid_.grid(), &resolution, max_xy, num_cells), "dliom_probability_grid_limits");
    std::unique_ptr<FileWriter> pgm_writer = file_writer_factory_(filestem_ + ".pgm");
    const std::string pgm_filename = pgm_writer->GetFilename();
    Write(pgm_writer.get(), [&](char* buffer, int64_t capacity, int64_t* length) {  // WritePgm (ros_map.cc:21-34)
      return dliom_ros_map_pgm_header(resolution, size[0], size[1], buffer, capacity, length);
    });
    if (!pgm_writer->Write(reinterpret_cast<const char*>(gray.data()), gray.size()) || !pgm_writer->Close()) Fail("pgm");
    double origin[2];
    Check(dliom_ros_map_yaml_origin(resolution, max_xy, offset, size[0], size[1], origin), "dliom_ros_map_yaml_origin");
    std::unique_ptr<FileWriter> yaml_writer = file_writer_factory_(filestem_ + ".yaml");
    Write(yaml_writer.get(), [&](char* buffer, int64_t capacity, int64_t* length) {  // WriteYaml (ros_map.cc:36-47)
      return dliom_ros_map_yaml(resolution, origin, pgm_filename.c_str(), buffer, capacity, length);
    });
    if (!yaml_writer->Close()) Fail("yaml");
    return internal::FlushLastStage(next_, "ROS map writing must be configured to occur after any stages that require "
                                           "multiple passes.");
  }
  const dliom_probability_grid* grid() const { return grid_.grid(); }

 private:
  static void Fail(const char* what) {
    std::fprintf(stderr, "Check failed: writing the %s file\n", what);  // CHECK(writer->Close())
    std::abort();
  }
  template <typename Text>
  static void Write(FileWriter* writer, Text text) {
    int64_t length = 0;
    text(nullptr, 0, &length);  // the size
    std::string buffer(static_cast<size_t>(length), '\0');
    Check(text(&buffer[0], length, &length), "ros map text");
    if (!writer->Write(buffer.data(), buffer.size())) Fail("map");
  }
  const std::string filestem_;
  PointsProcessor* const next_;
  FileWriterFactory file_writer_factory_;
  internal::ProbabilityGridOnDevice grid_;
};

namespace internal {
// What the PLY and the PCD writer share: the header rewritten in place, one Write of packed records a batch.
class RecordWriter {
 public:
  RecordWriter(std::unique_ptr<FileWriter> file, Context* context) : context_(context), file_(std::move(file)) {}
  template <typename Header>
  void WriteHeader(Header header) {
    int64_t length = 0;
    header(nullptr, 0, &length);  // the size
    std::string text(static_cast<size_t>(length), '\0');
    Check(header(&text[0], length, &length), "points file header");
    if (!file_->WriteHeader(text.data(), text.size())) Fail("WriteHeader");
  }
  // the batch's records, packed on the device and downloaded in one copy -> its number of points
  int64_t WriteRecords(PointsBatch* batch, int format, bool with_colors, bool with_intensities) {
    DeviceBatch* d = EnsureOnDevice(context_, batch);
    int64_t bytes = 0;
    Check(dliom_points_batch_pack(d->batch, format, with_colors ? 1 : 0, with_intensities ? 1 : 0, nullptr, 0, &bytes),
          "dliom_points_batch_pack: the first PointsBatch had an attribute that this one lacks");
    records_.resize(static_cast<size_t>(bytes));
    Check(dliom_points_batch_pack(d->batch, format, with_colors ? 1 : 0, with_intensities ? 1 : 0, records_.data(), bytes, &bytes),
          "dliom_points_batch_pack");
    DeviceBatch::DownloadedBytes() += bytes;
    if (!file_->Write(reinterpret_cast<const char*>(records_.data()), records_.size())) Fail("Write");
    return d->size();
  }
  void Close() {
    if (!file_->Close()) Fail("Close");
  }
  Context* context() const { return context_; }

 private:
  static void Fail(const char* what) {
    std::fprintf(stderr, "Check failed: file_writer->%s\n", what);
    std::abort();
  }
  Context* const context_;
  std::unique_ptr<FileWriter> file_;
  std::vector<uint8_t> records_;
};
inline int64_t BatchSize(Context* context, const PointsBatch& batch) {
  const DeviceBatch* d = BatchOnDevice(context, batch);
  return d != nullptr ? d->size() : static_cast<int64_t>(batch.points.size());
}
inline void BatchAttributes(Context* context, PointsBatch* batch, bool* has_colors, bool* has_intensities) {
  const DeviceBatch* d = EnsureOnDevice(context, batch);
  int colors = 0, intensities = 0;
  Check(dliom_points_batch_has_colors(d->batch, &colors), "dliom_points_batch_has_colors");
  Check(dliom_points_batch_has_intensities(d->batch, &intensities), "dliom_points_batch_has_intensities");
  *has_colors = colors != 0;
  *has_intensities = intensities != 0;
}
}  // namespace internal

// io/ply_writing_points_processor.{h,cc}: "write_ply"
class PlyWritingPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "write_ply";
  PlyWritingPointsProcessor(std::unique_ptr<FileWriter> file_writer, PointsProcessor* next, Context* context = nullptr)
      : next_(next), writer_(std::move(file_writer), context != nullptr ? context : Context::ForThisThread()) {}

  void Process(std::unique_ptr<PointsBatch> batch) override {  // .cc:106-150
    if (internal::BatchSize(writer_.context(), *batch) == 0) {
      next_->Process(std::move(batch));
      return;
    }
    if (num_points_ == 0) {
      internal::BatchAttributes(writer_.context(), batch.get(), &has_colors_, &has_intensities_);
      Header(0);
    }
    num_points_ += writer_.WriteRecords(batch.get(), DLIOM_PACK_PLY, has_colors_, has_intensities_);
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override {  // .cc:91-104
    Header(num_points_);
    writer_.Close();
    return internal::FlushLastStage(next_, "PLY generation must be configured to occur after any stages that require multiple "
                                           "passes.");
  }

 private:
  void Header(int64_t num_points) {
    writer_.WriteHeader([&](char* buffer, int64_t capacity, int64_t* length) {
      return dliom_ply_header(has_colors_ ? 1 : 0, has_intensities_ ? 1 : 0, num_points, buffer, capacity, length);
    });
  }
  PointsProcessor* const next_;
  internal::RecordWriter writer_;
  int64_t num_points_ = 0;
  bool has_colors_ = false, has_intensities_ = false;
};

// io/pcd_writing_points_processor.{h,cc}: "write_pcd".  The header's colour field is the first non-empty batch's; a later
// batch whose colours differ from it is refused (the reference would write records the header does not describe).
class PcdWritingPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "write_pcd";
  PcdWritingPointsProcessor(std::unique_ptr<FileWriter> file_writer, PointsProcessor* next, Context* context = nullptr)
      : next_(next), writer_(std::move(file_writer), context != nullptr ? context : Context::ForThisThread()) {}

  void Process(std::unique_ptr<PointsBatch> batch) override {  // .cc:93-131
    if (internal::BatchSize(writer_.context(), *batch) == 0) {
      next_->Process(std::move(batch));
      return;
    }
    if (num_points_ == 0) {
      bool unused = false;
      internal::BatchAttributes(writer_.context(), batch.get(), &has_colors_, &unused);
      Header(0);
    }
    num_points_ += writer_.WriteRecords(batch.get(), DLIOM_PACK_PCD, has_colors_, false);
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override {  // .cc:78-91
    Header(num_points_);
    writer_.Close();
    return internal::FlushLastStage(next_, "PCD generation must be configured to occur after any stages that require multiple "
                                           "passes.");
  }

 private:
  void Header(int64_t num_points) {
    writer_.WriteHeader([&](char* buffer, int64_t capacity, int64_t* length) {
      return dliom_pcd_header(has_colors_ ? 1 : 0, num_points, buffer, capacity, length);
    });
  }
  PointsProcessor* const next_;
  internal::RecordWriter writer_;
  int64_t num_points_ = 0;
  bool has_colors_ = false;
};

// io/xyz_writing_points_processor.{h,cc}: "write_xyz".  The reference formats one point at a time through a
// std::ostringstream; here the batch's text is made on the device (dliom.h "XYZ text of export batches": the same bytes)
// and written with one Write.  The buffer holds DLIOM_XYZ_MAX_RECORD bytes a point, which one call never refuses.
class XyzWriterPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "write_xyz";
  XyzWriterPointsProcessor(std::unique_ptr<FileWriter> file_writer, PointsProcessor* next, Context* context = nullptr)
      : next_(next), context_(context != nullptr ? context : Context::ForThisThread()), file_writer_(std::move(file_writer)) {}

  void Process(std::unique_ptr<PointsBatch> batch) override {  // .cc:50-55
    const int64_t n = internal::BatchSize(context_, *batch);
    if (n > 0) {
      internal::DeviceBatch* d = internal::EnsureOnDevice(context_, batch.get());
      text_.resize(static_cast<size_t>(n) * DLIOM_XYZ_MAX_RECORD);
      int64_t bytes = 0;
      Check(dliom_points_batch_pack_xyz(d->batch, text_.data(), static_cast<int64_t>(text_.size()), &bytes),
            "dliom_points_batch_pack_xyz");
      internal::DeviceBatch::DownloadedBytes() += bytes;
      if (!file_writer_->Write(reinterpret_cast<const char*>(text_.data()), static_cast<size_t>(bytes))) Fail("Write");
    }
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override {  // .cc:37-48
    if (!file_writer_->Close()) Fail("Close");  // "Closing XYZ file failed."
    return internal::FlushLastStage(next_, "XYZ generation must be configured to occur after any stages that require multiple "
                                           "passes.");
  }

 private:
  static void Fail(const char* what) {
    std::fprintf(stderr, "Check failed: file_writer->%s\n", what);
    std::abort();
  }
  PointsProcessor* const next_;
  Context* const context_;
  std::unique_ptr<FileWriter> file_writer_;
  std::vector<uint8_t> text_;
};

// io/counting_points_processor.{h,cc}: "dump_num_points".  A batch in HBM is asked for its size; nothing is downloaded.
class CountingPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "dump_num_points";
  explicit CountingPointsProcessor(PointsProcessor* next, Context* context = nullptr)
      : next_(next), context_(context != nullptr ? context : Context::ForThisThread()) {}

  void Process(std::unique_ptr<PointsBatch> batch) override {  // .cc:37-40
    num_points_ += internal::BatchSize(context_, *batch);
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override {  // .cc:42-55
    switch (next_->Flush()) {
      case FlushResult::kFinished:
        std::fprintf(stderr, "Processed %lld and finishing.\n", static_cast<long long>(num_points_));
        return FlushResult::kFinished;
      case FlushResult::kRestartStream:
        std::fprintf(stderr, "Processed %lld and restarting stream.\n", static_cast<long long>(num_points_));
        num_points_ = 0;
        return FlushResult::kRestartStream;
    }
    std::abort();  // LOG(FATAL)
  }
  int64_t num_points() const { return num_points_; }  // (not in the reference, which only logs it)

 private:
  PointsProcessor* const next_;
  Context* const context_;
  int64_t num_points_ = 0;
};

// io/frame_id_filtering_points_processor.{h,cc}: "frame_id_filter".  Whole batches are passed on or dropped by their
// frame_id; the points, wherever they are, are not touched.
class FrameIdFilteringPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "frame_id_filter";
  FrameIdFilteringPointsProcessor(const std::unordered_set<std::string>& keep_frame_ids,
                                  const std::unordered_set<std::string>& drop_frame_ids, PointsProcessor* next)
      : keep_frame_ids_(keep_frame_ids), drop_frame_ids_(drop_frame_ids), next_(next) {
    if (keep_frame_ids.empty() == drop_frame_ids.empty()) {  // CHECK_NE (.cc:52-54)
      std::fprintf(stderr, "Check failed: You have to specify exactly one of the `keep_frames` property or the `drop_frames` "
                           "property, but not both at the same time.\n");
      std::abort();
    }
  }

  void Process(std::unique_ptr<PointsBatch> batch) override {  // .cc:57-63
    if ((!keep_frame_ids_.empty() && keep_frame_ids_.count(batch->frame_id)) ||
        (!drop_frame_ids_.empty() && !drop_frame_ids_.count(batch->frame_id))) {
      next_->Process(std::move(batch));
    }
  }
  FlushResult Flush() override { return next_->Flush(); }  // .cc:65-67

 private:
  const std::unordered_set<std::string> keep_frame_ids_;
  const std::unordered_set<std::string> drop_frame_ids_;
  PointsProcessor* const next_;
};

// io/coloring_points_processor.{h,cc}: "color_points".  On a batch in HBM the colour is set there; on host vectors it
// writes batch->colors and leaves the points alone, so what a stage before left in device_points stays valid.
class ColoringPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "color_points";
  ColoringPointsProcessor(const FloatColor& color, const std::string& frame_id, PointsProcessor* next)
      : color_(color), frame_id_(frame_id), next_(next) {}
  // FromDictionary's ToFloatColor(Uint8Color) (io/color.h:40,46-49): c / 255.f
  static FloatColor FromUint8(uint8_t r, uint8_t g, uint8_t b) { return FloatColor{{r / 255.f, g / 255.f, b / 255.f}}; }

  void Process(std::unique_ptr<PointsBatch> batch) override {  // .cc:48-56
    if (batch->frame_id == frame_id_) {
      internal::DeviceBatch* d = batch->device_batch.get();
      if (d != nullptr && d->host_stale) {
        Check(dliom_points_batch_color(d->batch, color_.data()), "dliom_points_batch_color");
      } else {
        batch->device_batch.reset();
        batch->colors.assign(batch->points.size(), color_);
      }
    }
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override { return next_->Flush(); }

 private:
  const FloatColor color_;
  const std::string frame_id_;
  PointsProcessor* const next_;
};

// io/intensity_to_color_points_processor.{h,cc}: "intensity_to_color"
class IntensityToColorPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "intensity_to_color";
  IntensityToColorPointsProcessor(float min_intensity, float max_intensity, const std::string& frame_id, PointsProcessor* next)
      : min_intensity_(min_intensity), max_intensity_(max_intensity), frame_id_(frame_id), next_(next) {}

  void Process(std::unique_ptr<PointsBatch> batch) override {  // .cc:47-60
    internal::DeviceBatch* d = batch->device_batch.get();
    if (d != nullptr && d->host_stale) {  // (a batch without intensities is left alone by the call itself)
      if (frame_id_.empty() || batch->frame_id == frame_id_)
        Check(dliom_points_batch_intensity_to_color(d->batch, min_intensity_, max_intensity_), "dliom_points_batch_intensity_to_color");
      next_->Process(std::move(batch));
      return;
    }
    if (!batch->intensities.empty() && (frame_id_.empty() || batch->frame_id == frame_id_)) {
      batch->device_batch.reset();
      batch->colors.clear();
      for (const float intensity : batch->intensities) {
        const float scaled = (intensity - min_intensity_) / (max_intensity_ - min_intensity_);
        const float gray = scaled > 1.f ? 1.f : (scaled < 0.f ? 0.f : scaled);  // common::Clamp(value, 0.f, 1.f)
        batch->colors.push_back(FloatColor{{gray, gray, gray}});
      }
    }
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override { return next_->Flush(); }

 private:
  const float min_intensity_, max_intensity_;
  const std::string frame_id_;
  PointsProcessor* const next_;
};

// io/xray_points_processor.{h,cc}: "write_xray_image".  One device aggregator per floor (one without floors) and the
// reference's single bounding box over all of them.  Flush hands every image to `sink` as io::Image's pixels
// (0xFF000000 | r << 16 | g << 8 | b, row-major) under the reference's file name; PNG encoding, cairo's trajectory
// drawing (DrawTrajectories::kNo here; VoxelIndexToPixel is what a caller's DrawTrajectory needs) and DetectFloors stay
// with the caller.
class XRayPointsProcessor : public PointsProcessor {
 public:
  constexpr static const char* kConfigurationFileActionName = "write_xray_image";
  struct XRayImage {
    std::string filename;
    int width = 0, height = 0;
    std::vector<uint32_t> pixels;
  };
  using ImageSink = std::function<void(const XRayImage& image)>;
  XRayPointsProcessor(double voxel_size, const transform::Rigid3f& transform, const std::vector<mapping::Floor>& floors,
                      const std::string& output_filename, ImageSink sink, PointsProcessor* next, Context* context = nullptr)
      : next_(next),
        context_(context != nullptr ? context : Context::ForThisThread()),
        floors_(floors),
        output_filename_(output_filename),
        sink_(std::move(sink)) {
    const std::array<float, 7> t = transform.ToArray();
    aggregations_.resize(floors_.empty() ? 1 : floors_.size(), nullptr);  // .cc:112-115
    for (dliom_points_xray*& a : aggregations_)
      Check(dliom_points_xray_create(context_->get(), voxel_size, t.data(), &a), "dliom_points_xray_create");
  }
  ~XRayPointsProcessor() override {
    for (dliom_points_xray* a : aggregations_)
      if (a != nullptr) dliom_points_xray_destroy(a);
  }

  void Process(std::unique_ptr<PointsBatch> batch) override {  // .cc:215-228
    if (floors_.empty()) {
      Insert(*batch, aggregations_[0]);
    } else {
      for (size_t i = 0; i < floors_.size(); ++i) {
        if (!ContainedIn(batch->start_time, floors_[i].timespans)) continue;
        Insert(*batch, aggregations_[i]);
      }
    }
    next_->Process(std::move(batch));
  }

  FlushResult Flush() override {  // .cc:230-253
    if (floors_.empty()) {
      WriteVoxels(aggregations_[0], output_filename_ + ".png");
    } else {
      for (size_t i = 0; i < floors_.size(); ++i) WriteVoxels(aggregations_[i], output_filename_ + std::to_string(i) + ".png");
    }
    return internal::FlushLastStage(next_, "X-Ray generation must be configured to occur after any stages that require "
                                           "multiple passes.");
  }

  // bounding_box_ over every aggregation; false while it is empty
  bool BoundingBox(int32_t box_min[3], int32_t box_max[3]) const {
    bool any = false;
    for (const dliom_points_xray* a : aggregations_) {
      int32_t lo[3], hi[3];
      int empty = 1;
      Check(dliom_points_xray_bounding_box(a, lo, hi, &empty), "dliom_points_xray_bounding_box");
      if (empty) continue;
      for (int k = 0; k < 3; ++k) {
        box_min[k] = any ? std::min(box_min[k], lo[k]) : lo[k];
        box_max[k] = any ? std::max(box_max[k], hi[k]) : hi[k];
      }
      any = true;
    }
    return any;
  }
  // voxel_index_to_pixel (.cc:152-157) of a cell index in the current bounding box; false while the box is empty
  bool VoxelIndexToPixel(const int32_t index[3], int32_t pixel[2]) const {
    int32_t lo[3], hi[3];
    if (!BoundingBox(lo, hi)) return false;
    pixel[0] = hi[1] - index[1];
    pixel[1] = hi[2] - index[2];
    return true;
  }
  const std::vector<dliom_points_xray*>& aggregations() const { return aggregations_; }

 private:
  static bool ContainedIn(int64_t time, const std::vector<mapping::Timespan>& timespans) {  // .cc:86-94
    for (const mapping::Timespan& timespan : timespans)
      if (timespan.start <= time && time <= timespan.end) return true;
    return false;
  }
  void Insert(const PointsBatch& batch_in, dliom_points_xray* aggregation) {  // .cc:195-213
    if (const internal::DeviceBatch* d = internal::BatchOnDevice(context_, batch_in)) {
      if (d->host_stale) {  // the colours are read where they are
        Check(dliom_points_xray_insert_batch(aggregation, d->batch), "dliom_points_xray_insert_batch");
        return;
      }
    }
    PointsBatch synced;  // (a device batch of another context: by way of the host)
    const PointsBatch* host = &batch_in;
    if (batch_in.device_batch != nullptr && batch_in.device_batch->host_stale) {
      synced.device_batch = batch_in.device_batch;
      internal::SyncToHost(&synced);
      synced.device_batch.reset();
      host = &synced;
    }
    const PointsBatch& batch = *host;
    if (!batch.colors.empty() && batch.colors.size() < batch.points.size()) {
      std::fprintf(stderr, "Check failed: batch.colors.at(i)\n");  // std::out_of_range in the reference
      std::abort();
    }
    const std::shared_ptr<internal::DeviceCloud> points = internal::PointsOnDevice(context_, batch);
    // colours beyond the last point are never read (.cc:206-207)
    int64_t num_colors = static_cast<int64_t>(std::min(batch.colors.size(), batch.points.size()));
    // one colour for the whole batch (what ColoringPointsProcessor leaves) needs no per-point colours on the device
    if (num_colors > 1 && std::all_of(batch.colors.begin(), batch.colors.begin() + num_colors,
                                      [&](const FloatColor& c) { return SameBits(c, batch.colors[0]); }))
      num_colors = 1;
    Check(dliom_points_xray_insert(aggregation, points->cloud, num_colors > 0 ? batch.colors[0].data() : nullptr, num_colors),
          "dliom_points_xray_insert");
  }
  static bool SameBits(const FloatColor& a, const FloatColor& b) {
    uint32_t x[3], y[3];
    std::memcpy(x, a.data(), 12);
    std::memcpy(y, b.data(), 12);
    return x[0] == y[0] && x[1] == y[1] && x[2] == y[2];
  }
  void WriteVoxels(const dliom_points_xray* aggregation, const std::string& filename) {  // .cc:144-193
    int32_t lo[3], hi[3];
    if (!BoundingBox(lo, hi)) {
      std::fprintf(stderr, "Not writing output: bounding box is empty.\n");  // LOG(WARNING)
      return;
    }
    XRayImage image;
    image.filename = filename;
    int32_t w = 0, h = 0;
    Check(dliom_points_xray_draw(aggregation, lo, hi, nullptr, 0, &w, &h), "dliom_points_xray_draw");
    image.pixels.resize(static_cast<size_t>(w) * static_cast<size_t>(h));
    Check(dliom_points_xray_draw(aggregation, lo, hi, image.pixels.data(), static_cast<int64_t>(image.pixels.size()), &w, &h),
          "dliom_points_xray_draw");
    image.width = w;
    image.height = h;
    sink_(image);
  }

  PointsProcessor* const next_;
  Context* const context_;
  const std::vector<mapping::Floor> floors_;
  const std::string output_filename_;
  ImageSink sink_;
  std::vector<dliom_points_xray*> aggregations_;
};

// ---- io/submap_painter.{h,cc}: the map of all submaps -------------------------------------------------------------------
// A slice's texture lives in HBM (dliom_submap_slice) where the reference keeps a cairo surface; PaintSubmapSlices
// composites the slices on the device in std::map order (dliom.h "painting submap slices into one map") and returns
// pixels, not a cairo surface: cairo's trajectory drawing and PNG stay with the caller.
struct PaintSubmapSlicesResult {  // submap_painter.h:30-38
  std::vector<uint32_t> pixels;   // height x width, alpha << 24 | red << 16 | green << 8 | blue (CAIRO_FORMAT_ARGB32)
  int width = 0;
  int height = 0;
  std::array<float, 2> origin{{0.f, 0.f}};  // top left pixel of `pixels` in map frame
};

struct SubmapSlice {  // submap_painter.h:40-57
  // Texture data.
  int width = 0;
  int height = 0;
  int version = 0;
  double resolution = 0.;
  transform::Rigid3d slice_pose;
  std::shared_ptr<dliom_submap_slice> surface;  // the texture, on the device; null: PaintSubmapSlices stops there (.cc:38)
  // Metadata.
  transform::Rigid3d pose;  // set it after an optimisation as the reference does: the next paint uses it, no texel moves
  int metadata_version = -1;
};

struct SubmapTexturePixels {  // SubmapTexture::Pixels, submap_painter.h:60-63
  std::vector<char> intensity;
  std::vector<char> alpha;
};

// UnpackTextureData (submap_painter.cc:140-156) without its gunzip step: `cells` are the uncompressed bytes
inline SubmapTexturePixels UnpackTextureData(const std::string& cells, int width, int height) {
  SubmapTexturePixels pixels;
  const size_t num_pixels = static_cast<size_t>(width) * height;
  if (cells.size() != 2 * num_pixels) Check(DLIOM_ERR_INVALID_ARGUMENT, "UnpackTextureData: CHECK_EQ(cells.size(), 2 * num_pixels)");
  for (size_t i = 0; i < num_pixels; ++i) {
    pixels.intensity.push_back(cells[2 * i]);
    pixels.alpha.push_back(cells[2 * i + 1]);
  }
  return pixels;
}

namespace internal {
inline void AdoptSlice(dliom_submap_slice* handle, SubmapSlice* submap_slice) {
  submap_slice->surface = std::shared_ptr<dliom_submap_slice>(handle, [](dliom_submap_slice* s) { dliom_submap_slice_destroy(s); });
  dliom_submap_slice_description d;
  Check(dliom_submap_slice_info(handle, &d), "dliom_submap_slice_info");
  submap_slice->width = d.width;
  submap_slice->height = d.height;
  submap_slice->resolution = d.resolution;
  submap_slice->slice_pose = transform::Rigid3d::FromArray(d.slice_pose7);
  submap_slice->pose = transform::Rigid3d::FromArray(d.pose7);
}
}  // namespace internal

// FillSubmapSlice (submap_painter.cc:110-138) for a 3D submap on the device: textures(0), the high resolution grid's, made
// by the X-ray kernels and kept in HBM.  2D submaps are not covered.
inline void FillSubmapSlice(const transform::Rigid3d& global_submap_pose, const mapping::Submap3D& submap,
                            SubmapSlice* const submap_slice) {
  const std::array<double, 7> pose = global_submap_pose.ToArray();
  dliom_submap_slice* handle = nullptr;
  Check(dliom_submap_slice_create_from_grid(submap.high_resolution_hybrid_grid(), pose.data(), &handle),
        "dliom_submap_slice_create_from_grid");
  internal::AdoptSlice(handle, submap_slice);
  submap_slice->version = submap.num_range_data();
}
// ... and for a texture that arrived as bytes (a SubmapQuery response, cells uncompressed): uploaded once
inline void FillSubmapSlice(Context* context, const transform::Rigid3d& global_submap_pose, const mapping::SubmapTexture& texture,
                            SubmapSlice* const submap_slice) {
  const std::array<double, 7> pose = global_submap_pose.ToArray(), slice_pose = texture.slice_pose.ToArray();
  if (texture.cells.size() != 2 * static_cast<size_t>(texture.width) * texture.height)
    Check(DLIOM_ERR_INVALID_ARGUMENT, "FillSubmapSlice: CHECK_EQ(cells.size(), 2 * num_pixels)");
  dliom_submap_slice* handle = nullptr;
  Check(dliom_submap_slice_create(context->get(), reinterpret_cast<const uint8_t*>(texture.cells.data()), texture.width,
                                  texture.height, texture.resolution, slice_pose.data(), pose.data(), &handle),
        "dliom_submap_slice_create");
  internal::AdoptSlice(handle, submap_slice);
}

namespace internal {
// the handles in std::map order up to the first slice without a texture, their poses brought up to date
inline std::vector<const dliom_submap_slice*> SliceHandles(const std::map<mapping::SubmapId, SubmapSlice>& submaps) {
  std::vector<const dliom_submap_slice*> handles;
  for (const auto& pair : submaps) {
    if (pair.second.surface == nullptr) break;
    const std::array<double, 7> pose = pair.second.pose.ToArray();
    Check(dliom_submap_slice_set_pose(pair.second.surface.get(), pose.data()), "dliom_submap_slice_set_pose");
    handles.push_back(pair.second.surface.get());
  }
  return handles;
}
}  // namespace internal

// PaintSubmapSlices (submap_painter.cc:62-108)
inline PaintSubmapSlicesResult PaintSubmapSlices(const std::map<mapping::SubmapId, SubmapSlice>& submaps, const double resolution) {
  const std::vector<const dliom_submap_slice*> handles = internal::SliceHandles(submaps);
  PaintSubmapSlicesResult r;
  int32_t w = 0, h = 0;
  const int64_t n = static_cast<int64_t>(handles.size());
  Check(dliom_submap_slices_paint(nullptr, handles.data(), n, resolution, nullptr, 0, &w, &h, r.origin.data()),
        "dliom_submap_slices_paint");
  r.pixels.resize(static_cast<size_t>(w) * h);
  Check(dliom_submap_slices_paint(nullptr, handles.data(), n, resolution, r.pixels.data(), static_cast<int64_t>(r.pixels.size()), &w,
                                  &h, r.origin.data()), "dliom_submap_slices_paint");
  r.width = w;
  r.height = h;
  return r;
}

// nav_msgs::OccupancyGrid's info and data (cartographer_ros msg_conversion.cc:321-368) as a plain struct: header.stamp,
// frame_id and map_load_time stay with the caller; origin orientation is the identity
struct OccupancyGrid {
  double resolution = 0.;
  int width = 0;
  int height = 0;
  std::array<double, 3> origin_position{{0., 0., 0.}};
  std::vector<int8_t> data;
};
// PaintSubmapSlices + CreateOccupancyGridMsg in one call: painted and converted on the device, one byte a cell comes back
inline OccupancyGrid CreateOccupancyGrid(const std::map<mapping::SubmapId, SubmapSlice>& submaps, const double resolution) {
  const std::vector<const dliom_submap_slice*> handles = internal::SliceHandles(submaps);
  OccupancyGrid g;
  g.resolution = resolution;
  int32_t w = 0, h = 0;
  const int64_t n = static_cast<int64_t>(handles.size());
  Check(dliom_submap_slices_occupancy(nullptr, handles.data(), n, resolution, nullptr, 0, &w, &h, nullptr, g.origin_position.data()),
        "dliom_submap_slices_occupancy");
  g.data.resize(static_cast<size_t>(w) * h);
  Check(dliom_submap_slices_occupancy(nullptr, handles.data(), n, resolution, g.data.data(), static_cast<int64_t>(g.data.size()), &w,
                                      &h, nullptr, g.origin_position.data()), "dliom_submap_slices_occupancy");
  g.width = w;
  g.height = h;
  return g;
}

}  // namespace io

// ---- sensor::CompressedPointCloud and mapping::ToProto / FromProto(TrajectoryNode::Data) on device clouds
// (sensor/compressed_point_cloud.h:36-95, mapping/trajectory_node.h:39-69, .cc:27-69; dliom.h "compressed point clouds").
// Protos travel as their serialized bytes (std::string): inside cartographer, ParseFromString / SerializeAsString on the
// generated classes are the glue.
namespace sensor {
class CompressedPointCloud {
 public:
  CompressedPointCloud() {}
  // Compresses a cloud in HBM (what LocalTrajectoryBuilder3D::matched_clouds hands out)
  CompressedPointCloud(Context* context, const dliom_cloud* cloud) {
    int64_t words = 0;
    int64_t points = 0;
    Check(dliom_cloud_size(cloud, &points), "dliom_cloud_size");
    Check(dliom_cloud_compress(context->get(), cloud, nullptr, 0, &words), "CompressedPointCloud: a point beyond the 23-bit range");
    point_data_.resize(static_cast<size_t>(words));
    Check(dliom_cloud_compress(context->get(), cloud, point_data_.data(), words, &words), "dliom_cloud_compress");
    num_points_ = static_cast<int32_t>(points);
  }
  CompressedPointCloud(Context* context, const PointCloud& point_cloud)
      : CompressedPointCloud(context, io::internal::DeviceCloud(context, point_cloud).cloud) {}
  // CompressedPointCloud(const proto::CompressedPointCloud&), from the serialized message (host only)
  static CompressedPointCloud FromProto(const std::string& bytes) {
    CompressedPointCloud c;
    const uint8_t* b = reinterpret_cast<const uint8_t*>(bytes.data());
    int64_t words = 0;
    Check(dliom_compressed_point_cloud_from_proto(b, static_cast<int64_t>(bytes.size()), &c.num_points_, nullptr, 0, &words),
          "dliom_compressed_point_cloud_from_proto");
    c.point_data_.resize(static_cast<size_t>(words));
    Check(dliom_compressed_point_cloud_from_proto(b, static_cast<int64_t>(bytes.size()), &c.num_points_, c.point_data_.data(), words,
                                                  &words), "dliom_compressed_point_cloud_from_proto");
    return c;
  }
  bool empty() const { return num_points_ == 0; }
  size_t size() const { return static_cast<size_t>(num_points_); }
  const std::vector<int32_t>& point_data() const { return point_data_; }
  bool operator==(const CompressedPointCloud& other) const {
    return num_points_ == other.num_points_ && point_data_ == other.point_data_;
  }
  // Decompress() into HBM: the caller's cloud; a malformed stream fails the CHECK the reference lacks (its TODO)
  std::shared_ptr<io::internal::DeviceCloud> DecompressOnDevice(Context* context) const {
    dliom_cloud* cloud = nullptr;
    Check(dliom_cloud_decompress(context->get(), num_points_, point_data_.data(), static_cast<int64_t>(point_data_.size()), &cloud),
          "dliom_cloud_decompress");
    return std::make_shared<io::internal::DeviceCloud>(context, cloud);
  }
  PointCloud Decompress(Context* context) const {
    const std::shared_ptr<io::internal::DeviceCloud> cloud = DecompressOnDevice(context);
    PointCloud points(size());
    if (!points.empty()) Check(dliom_cloud_download(cloud->cloud, &points[0].x), "dliom_cloud_download");
    return points;
  }
  // ToProto().SerializeAsString() (host only: frames the words)
  std::string ToProto() const {
    int64_t size = 0;
    const int64_t words = static_cast<int64_t>(point_data_.size());
    Check(dliom_compressed_point_cloud_to_proto(num_points_, point_data_.data(), words, nullptr, 0, &size),
          "dliom_compressed_point_cloud_to_proto");
    std::string bytes(static_cast<size_t>(size), '\0');
    Check(dliom_compressed_point_cloud_to_proto(num_points_, point_data_.data(), words, reinterpret_cast<uint8_t*>(&bytes[0]), size, &size),
          "dliom_compressed_point_cloud_to_proto");
    return bytes;
  }

 private:
  int32_t num_points_ = 0;
  std::vector<int32_t> point_data_;
};
}  // namespace sensor

namespace mapping {
struct TrajectoryNode {
  // TrajectoryNode::Data with its clouds in HBM (null: the empty cloud); time in ticks of 100 ns (common::ToUniversal)
  struct Data {
    int64_t time = 0;
    transform::Quaterniond gravity_alignment{{1, 0, 0, 0}};
    std::shared_ptr<io::internal::DeviceCloud> filtered_gravity_aligned_point_cloud;
    std::shared_ptr<io::internal::DeviceCloud> high_resolution_point_cloud;
    std::shared_ptr<io::internal::DeviceCloud> low_resolution_point_cloud;
    std::vector<float> rotational_scan_matcher_histogram;
    transform::Rigid3d local_pose;
  };
};

// mapping::ToProto over a span of nodes, serialized: every cloud of every node is compressed in ONE device batch -- what
// a SerializeState loop calls instead of a ToProto a node.
inline std::vector<std::string> ToProto(Context* context, const TrajectoryNode::Data* const* nodes, size_t count) {
  std::vector<dliom_trajectory_node_data> in(count);
  for (size_t i = 0; i < count; ++i) {
    const TrajectoryNode::Data& d = *nodes[i];
    dliom_trajectory_node_data& n = in[i];
    n.timestamp = d.time;
    std::memcpy(n.gravity_alignment_wxyz, d.gravity_alignment.wxyz, sizeof n.gravity_alignment_wxyz);
    n.filtered_gravity_aligned = d.filtered_gravity_aligned_point_cloud ? d.filtered_gravity_aligned_point_cloud->cloud : nullptr;
    n.high_resolution = d.high_resolution_point_cloud ? d.high_resolution_point_cloud->cloud : nullptr;
    n.low_resolution = d.low_resolution_point_cloud ? d.low_resolution_point_cloud->cloud : nullptr;
    n.histogram = d.rotational_scan_matcher_histogram.data();
    n.histogram_size = static_cast<int>(d.rotational_scan_matcher_histogram.size());
    const std::array<double, 7> pose = d.local_pose.ToArray();
    std::memcpy(n.local_pose7, pose.data(), sizeof n.local_pose7);
  }
  std::vector<int64_t> offsets(count + 1, 0);
  int refused = -1;
  Check(dliom_trajectory_nodes_data_to_proto(context->get(), in.data(), static_cast<int>(count), nullptr, 0, offsets.data(), &refused),
        "mapping::ToProto(TrajectoryNode::Data): a point beyond the 23-bit range");
  std::vector<uint8_t> bytes(static_cast<size_t>(offsets[count]) + 1);
  Check(dliom_trajectory_nodes_data_to_proto(context->get(), in.data(), static_cast<int>(count), bytes.data(), offsets[count],
                                             offsets.data(), &refused), "dliom_trajectory_nodes_data_to_proto");
  std::vector<std::string> protos(count);
  for (size_t i = 0; i < count; ++i) protos[i].assign(reinterpret_cast<const char*>(bytes.data()) + offsets[i], static_cast<size_t>(offsets[i + 1] - offsets[i]));
  return protos;
}
inline std::string ToProto(Context* context, const TrajectoryNode::Data& constant_data) {
  const TrajectoryNode::Data* node = &constant_data;
  return ToProto(context, &node, 1)[0];
}
inline TrajectoryNode::Data FromProto(Context* context, const std::string& proto) {
  TrajectoryNode::Data d;
  dliom_cloud* clouds[3] = {nullptr, nullptr, nullptr};
  double gravity[4], pose[7];
  int histogram_size = 0;
  const uint8_t* b = reinterpret_cast<const uint8_t*>(proto.data());
  const int64_t size = static_cast<int64_t>(proto.size());
  d.rotational_scan_matcher_histogram.resize(256);
  int status = dliom_trajectory_node_data_from_proto(context->get(), b, size, &d.time, gravity, &clouds[0], &clouds[1], &clouds[2],
                                                     d.rotational_scan_matcher_histogram.data(), 256, &histogram_size, pose);
  if (status == DLIOM_ERR_CAPACITY) {
    d.rotational_scan_matcher_histogram.resize(static_cast<size_t>(histogram_size));
    status = dliom_trajectory_node_data_from_proto(context->get(), b, size, &d.time, gravity, &clouds[0], &clouds[1], &clouds[2],
                                                   d.rotational_scan_matcher_histogram.data(), histogram_size, &histogram_size, pose);
  }
  Check(status, "dliom_trajectory_node_data_from_proto");
  d.rotational_scan_matcher_histogram.resize(static_cast<size_t>(histogram_size));
  d.gravity_alignment = transform::Quaterniond{{gravity[0], gravity[1], gravity[2], gravity[3]}};
  d.filtered_gravity_aligned_point_cloud = std::make_shared<io::internal::DeviceCloud>(context, clouds[0]);
  d.high_resolution_point_cloud = std::make_shared<io::internal::DeviceCloud>(context, clouds[1]);
  d.low_resolution_point_cloud = std::make_shared<io::internal::DeviceCloud>(context, clouds[2]);
  d.local_pose = transform::Rigid3d::FromArray(pose);
  return d;
}
}  // namespace mapping
// pcl::IterativeClosestPoint<PointXYZ, PointXYZ> as gen_ground_truth_by_ndt_match.cc:190-205 and
// LocalTrajectoryBuilder3D::MatchByICP (local_trajectory_builder_3d.cc:937-967) use it, with PCL's method names, on the
// device (dliom.h "scan alignment by ICP": exact nearest neighbours, a fixed-order least-squares solve).  Parity unpinned
// against PCL (dliom.h).  Points with a non-finite coordinate take no part, so removeNaNFromPointCloud (:97) is not needed.
namespace registration {
struct Matrix4f {  // Eigen::Matrix4f's element access; row-major storage
  float m[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  static Matrix4f Identity() { return Matrix4f(); }
  float& operator()(int row, int col) { return m[4 * row + col]; }
  float operator()(int row, int col) const { return m[4 * row + col]; }
};
class IterativeClosestPoint {
 public:
  explicit IterativeClosestPoint(Context* context) : context_(context) {
    Check(dliom_icp_default_options(&options_), "dliom_icp_default_options");
    // PCL's own defaults where the tool sets nothing else: 10 iterations, no bound, both epsilons 0
    options_.max_correspondence_distance = std::sqrt(std::numeric_limits<double>::max());
    options_.maximum_iterations = 10;
    options_.transformation_epsilon = 0.0;
    options_.euclidean_fitness_epsilon = 0.0;
  }
  ~IterativeClosestPoint() { Reset(); }
  IterativeClosestPoint(const IterativeClosestPoint&) = delete;
  IterativeClosestPoint& operator=(const IterativeClosestPoint&) = delete;

  void setMaxCorrespondenceDistance(double distance) { options_.max_correspondence_distance = distance; }
  void setMaximumIterations(int iterations) { options_.maximum_iterations = iterations; }
  void setTransformationEpsilon(double epsilon) { options_.transformation_epsilon = epsilon; }
  void setEuclideanFitnessEpsilon(double epsilon) { options_.euclidean_fitness_epsilon = epsilon; }
  // the tool asks for none (:196); outlier rejection by RANSAC is not built
  void setRANSACIterations(int iterations) {
    if (iterations != 0) Check(DLIOM_ERR_INVALID_ARGUMENT, "IterativeClosestPoint::setRANSACIterations: only 0");
  }
  void setInputSource(const sensor::PointCloud* cloud) { source_ = cloud; }
  // builds the nearest-neighbour index of the target, as PCL builds its kd-tree here
  void setInputTarget(const sensor::PointCloud* cloud) {
    if (cloud == nullptr) Check(DLIOM_ERR_INVALID_ARGUMENT, "IterativeClosestPoint::setInputTarget");
    Reset();
    dliom_cloud* target = nullptr;
    Check(dliom_cloud_create(context_->get(), cloud->empty() ? nullptr : &(*cloud)[0].x, static_cast<int64_t>(cloud->size()), &target),
          "dliom_cloud_create");
    const int status = dliom_nn_index_create(context_->get(), target, nullptr, &index_);
    dliom_cloud_destroy(target);
    Check(status, "dliom_nn_index_create");
  }
  // output (may be null): the source under the final transformation
  void align(sensor::PointCloud* output, const Matrix4f& guess = Matrix4f::Identity()) {
    if (source_ == nullptr || index_ == nullptr) Check(DLIOM_ERR_INVALID_ARGUMENT, "IterativeClosestPoint::align: no input");
    dliom_cloud* source = nullptr;
    Check(dliom_cloud_create(context_->get(), source_->empty() ? nullptr : &(*source_)[0].x, static_cast<int64_t>(source_->size()),
                             &source),
          "dliom_cloud_create");
    double guess16[16];
    for (int k = 0; k < 16; ++k) guess16[k] = static_cast<double>(guess.m[k]);
    dliom_cloud* aligned = nullptr;
    const int status = dliom_icp_align(index_, source, guess16, &options_, &result_, output != nullptr ? &aligned : nullptr);
    dliom_cloud_destroy(source);
    Check(status, "dliom_icp_align");
    if (output != nullptr) {
      output->resize(source_->size());
      const int download = output->empty() ? DLIOM_OK : dliom_cloud_download(aligned, &(*output)[0].x);
      dliom_cloud_destroy(aligned);
      Check(download, "dliom_cloud_download");
    }
  }
  bool hasConverged() const { return result_.converged != 0; }
  double getFitnessScore() const { return result_.fitness_score; }
  Matrix4f getFinalTransformation() const {
    Matrix4f out;
    for (int k = 0; k < 16; ++k) out.m[k] = static_cast<float>(result_.transform[k]);
    return out;
  }
  const dliom_icp_result& result() const { return result_; }  // of the last align, with its reason and counts
  const dliom_icp_options& options() const { return options_; }

  // gen_ground_truth_by_ndt_match.cc:192-196
  static std::unique_ptr<IterativeClosestPoint> GroundTruthIcp(Context* context) { return Preset(context, 30.0); }
  // local_trajectory_builder_3d.cc:942-946
  static std::unique_ptr<IterativeClosestPoint> MatchByIcp(Context* context) { return Preset(context, 3.0); }

 private:
  static std::unique_ptr<IterativeClosestPoint> Preset(Context* context, double distance) {
    std::unique_ptr<IterativeClosestPoint> icp(new IterativeClosestPoint(context));
    icp->setMaxCorrespondenceDistance(distance);
    icp->setMaximumIterations(100);
    icp->setTransformationEpsilon(1e-6);
    icp->setEuclideanFitnessEpsilon(1e-6);
    icp->setRANSACIterations(0);
    return icp;
  }
  void Reset() {
    dliom_nn_index_destroy(index_);
    index_ = nullptr;
  }
  Context* context_;
  dliom_icp_options options_;
  dliom_icp_result result_ = {};
  const sensor::PointCloud* source_ = nullptr;
  dliom_nn_index* index_ = nullptr;
};

// The revisit node of gen_ground_truth_by_ndt_match.cc:158-167: among the nodes at least 60 s from node `from`, the one
// whose position is nearest to it; the first least distance wins.  -1: there is none (the tool would fall back on node 0
// unasked).  timestamps_ns: one a pose, nanoseconds.
inline int FindRevisitNode(const std::vector<transform::Rigid3d>& poses, const std::vector<int64_t>& timestamps_ns, size_t from) {
  if (from >= poses.size() || timestamps_ns.size() != poses.size()) Check(DLIOM_ERR_INVALID_ARGUMENT, "FindRevisitNode");
  int found = -1;
  double least = std::numeric_limits<double>::max();
  for (size_t k = 0; k < poses.size(); ++k) {
    if (k == from) continue;
    const int64_t apart = timestamps_ns[k] - timestamps_ns[from];
    if (static_cast<double>(apart < 0 ? -apart : apart) * 1e-9 < 60.) continue;
    const transform::Vector3d &a = poses[from].translation(), &b = poses[k].translation();
    const double dx = a.v[0] - b.v[0], dy = a.v[1] - b.v[1], dz = a.v[2] - b.v[2];
    const double distance = std::sqrt(dx * dx + dy * dy + dz * dz);
    if (distance < least) {
      least = distance;
      found = static_cast<int>(k);
    }
  }
  return found;
}

// One line of the tool's ground-truth file (:256-260) as an ostream with its default format writes it: the two stamps, the
// alignment error (a double), the three rows of (R | t) as floats, the norm of the translation's difference to the
// pose-graph's estimate (a float), each followed by a blank but the last, which a newline follows.
inline std::string FormatGroundTruthLine(int64_t stamp_from, int64_t stamp_to, double align_error, const Matrix4f& transformation,
                                         float difference_norm) {
  char text[64];
  std::snprintf(text, sizeof(text), "%lld %lld %g ", static_cast<long long>(stamp_from), static_cast<long long>(stamp_to), align_error);
  std::string line(text);
  for (int row = 0; row < 3; ++row)
    for (int col = 0; col < 4; ++col) {
      std::snprintf(text, sizeof(text), "%g ", static_cast<double>(transformation(row, col)));
      line += text;
    }
  std::snprintf(text, sizeof(text), "%g\n", static_cast<double>(difference_norm));
  return line + text;
}

// Many alignments in one call (dliom_icp_align_batch): the pairs of the tool's loop over a trajectory's constraints.
struct AlignmentPair {
  const sensor::PointCloud* source = nullptr;
  const sensor::PointCloud* target = nullptr;
  Matrix4f guess;
};
// Many nearest-neighbour indices in one call (dliom_nn_index_create_batch): what setInputTarget's dliom_nn_index_create
// builds cloud by cloud -- every query answered with the same bits -- in one device chain a chunk.  clouds: clouds of the
// context, none empty; a cloud may be named more than once.  options: NULL = the defaults, as setInputTarget passes.  -> an
// index a cloud, the caller's to destroy (dliom_nn_index_destroy), each on its own.  limits: NULL = the defaults.  stats
// (may be null): the call's.
inline std::vector<dliom_nn_index*> BuildNnIndices(Context* context, const std::vector<const dliom_cloud*>& clouds,
                                                   const dliom_nn_index_options* options = nullptr,
                                                   const dliom_nn_index_batch_limits* limits = nullptr,
                                                   dliom_nn_index_batch_stats* stats = nullptr) {
  std::vector<dliom_nn_index*> indices(clouds.size(), nullptr);
  dliom_nn_index* none = nullptr;
  Check(dliom_nn_index_create_batch(context->get(), clouds.data(), static_cast<int>(clouds.size()), options, limits,
                                    indices.empty() ? &none : indices.data(), stats),
        "dliom_nn_index_create_batch");
  return indices;
}
// How AlignPairs, AlignPairsNdt and the two generators build the indices of their distinct targets: one dliom_nn_index_create
// a target (one read-back each), or all of them in ONE dliom_nn_index_create_batch (one read-back a chunk).  The results are
// the same bits either way.
enum class IndexBuild { kOneByOne, kBatched };

// What IterativeClosestPoint with `icp_options` gives pair by pair (setInputSource, setInputTarget, align(guess), result()),
// bit for bit.  ONE index is built per distinct target pointer and one cloud uploaded per distinct source pointer, however
// many pairs name them.  limits: NULL = the defaults.  aligned (may be null): every pair's source under its final
// transformation.  stats (may be null): the call's.  build: kBatched uploads the distinct target clouds in the order of
// their first mention and builds all their indices in one call.
inline std::vector<dliom_icp_result> AlignPairs(Context* context, const dliom_icp_options& icp_options,
                                                const std::vector<AlignmentPair>& pairs, const dliom_icp_batch_limits* limits = nullptr,
                                                std::vector<sensor::PointCloud>* aligned = nullptr,
                                                dliom_icp_batch_stats* stats = nullptr, IndexBuild build = IndexBuild::kOneByOne) {
  struct Owned {  // destroyed on every way out, the indices before nothing else depends on them
    std::map<const sensor::PointCloud*, dliom_nn_index*> indices;
    std::map<const sensor::PointCloud*, dliom_cloud*> sources;
    std::vector<dliom_cloud*> target_clouds, outputs;
    ~Owned() {
      for (auto& e : indices) dliom_nn_index_destroy(e.second);
      for (auto& e : sources) dliom_cloud_destroy(e.second);
      for (dliom_cloud* c : target_clouds) dliom_cloud_destroy(c);
      for (dliom_cloud* c : outputs) dliom_cloud_destroy(c);
    }
  } owned;
  const auto upload = [context](const sensor::PointCloud* cloud) {
    dliom_cloud* out = nullptr;
    Check(dliom_cloud_create(context->get(), cloud->empty() ? nullptr : &(*cloud)[0].x, static_cast<int64_t>(cloud->size()), &out),
          "dliom_cloud_create");
    return out;
  };
  if (build == IndexBuild::kBatched) {
    std::vector<const sensor::PointCloud*> distinct;
    for (const AlignmentPair& p : pairs) {
      if (p.source == nullptr || p.target == nullptr) Check(DLIOM_ERR_INVALID_ARGUMENT, "AlignPairs: a pair without a cloud");
      if (std::find(distinct.begin(), distinct.end(), p.target) == distinct.end()) distinct.push_back(p.target);
    }
    for (const sensor::PointCloud* cloud : distinct) {
      owned.target_clouds.push_back(nullptr);
      owned.target_clouds.back() = upload(cloud);
    }
    const std::vector<const dliom_cloud*> clouds(owned.target_clouds.begin(), owned.target_clouds.end());
    const std::vector<dliom_nn_index*> built = BuildNnIndices(context, clouds);
    for (size_t k = 0; k < distinct.size(); ++k) owned.indices[distinct[k]] = built[k];
    for (dliom_cloud*& c : owned.target_clouds) {  // as one by one: a target's cloud is gone before the sources are uploaded
      dliom_cloud_destroy(c);
      c = nullptr;
    }
  }
  std::vector<dliom_icp_pair> table(pairs.size());
  for (size_t i = 0; i < pairs.size(); ++i) {
    const AlignmentPair& p = pairs[i];
    if (p.source == nullptr || p.target == nullptr) Check(DLIOM_ERR_INVALID_ARGUMENT, "AlignPairs: a pair without a cloud");
    if (owned.indices.find(p.target) == owned.indices.end()) {
      dliom_cloud* target = upload(p.target);
      dliom_nn_index* index = nullptr;
      const int status = dliom_nn_index_create(context->get(), target, nullptr, &index);
      dliom_cloud_destroy(target);
      Check(status, "dliom_nn_index_create");
      owned.indices[p.target] = index;
    }
    if (owned.sources.find(p.source) == owned.sources.end()) owned.sources[p.source] = upload(p.source);
    table[i].index = owned.indices[p.target];
    table[i].source = owned.sources[p.source];
    for (int k = 0; k < 16; ++k) table[i].guess[k] = static_cast<double>(p.guess.m[k]);
  }
  std::vector<dliom_icp_result> results(pairs.size());
  if (aligned != nullptr) owned.outputs.assign(pairs.size(), nullptr);
  Check(dliom_icp_align_batch(context->get(), table.data(), static_cast<int>(table.size()), &icp_options, limits, results.data(),
                              aligned != nullptr ? owned.outputs.data() : nullptr, stats),
        "dliom_icp_align_batch");
  if (aligned != nullptr) {
    aligned->assign(pairs.size(), sensor::PointCloud());
    for (size_t i = 0; i < pairs.size(); ++i) {
      (*aligned)[i].resize(pairs[i].source->size());
      if (!(*aligned)[i].empty()) Check(dliom_cloud_download(owned.outputs[i], &(*aligned)[i][0].x), "dliom_cloud_download");
    }
  }
  return results;
}

// gen_ground_truth_by_ndt_match.cc:182-185: gt = (poses[to].inverse() * poses[from]).cast<float>() as a 4x4, the rotation by
// toRotationMatrix's formula in float.
inline Matrix4f GroundTruthGuess(const transform::Rigid3d& to, const transform::Rigid3d& from) {
  namespace ff = mapping::optimization::fixed_frame;
  const transform::Rigid3f ig(ff::Multiply(ff::Inverse(to), from));
  const float w = ig.wxyz[0], x = ig.wxyz[1], y = ig.wxyz[2], z = ig.wxyz[3];
  const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
              tyy = ty * y, tyz = tz * y, tzz = tz * z;
  Matrix4f gt;
  const float R[9] = {1.f - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.f - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.f - (txx + tyy)};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) gt(r, c) = R[3 * r + c];
    gt(r, 3) = ig.t[r];
  }
  return gt;
}
// The line's last field (:202, :259): the norm of the translation of gt^-1 * trans.  The RIGID inverse in float, in this
// order: d = t_trans - t_gt per axis, v_c = (R_gt[0][c] * d_0 + R_gt[1][c] * d_1) + R_gt[2][c] * d_2, sqrt((v_0*v_0 + v_1*v_1) +
// v_2*v_2).  UNPINNED against Eigen's general 4x4 inverse, which the tool calls: the two agree to float rounding, not in bits.
inline float GroundTruthDifferenceNorm(const Matrix4f& gt, const Matrix4f& trans) {
  const float d[3] = {trans(0, 3) - gt(0, 3), trans(1, 3) - gt(1, 3), trans(2, 3) - gt(2, 3)};
  float v[3];
  for (int c = 0; c < 3; ++c) v[c] = (gt(0, c) * d[0] + gt(1, c) * d[1]) + gt(2, c) * d[2];
  return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

// The pair-collection half of the loop (:151-185), which the two methods share: for every `from` node that has a revisit node
// and whose two stamps lie within the bag, the stamps, the pose-graph's estimate gt and the pair (source: the `from` scan,
// target: the revisit node's, guess: gt), in order.
struct GroundTruthWanted {
  int64_t stamp_from, stamp_to;
  Matrix4f gt;
};
inline void CollectGroundTruthPairs(const std::vector<transform::Rigid3d>& poses, const std::vector<int64_t>& timestamps_ns,
                                    const std::vector<int64_t>& stamps_in_bag, const std::vector<sensor::PointCloud>& clouds,
                                    const std::vector<size_t>& from_nodes, std::vector<GroundTruthWanted>* wanted,
                                    std::vector<AlignmentPair>* pairs) {
  for (const size_t from : from_nodes) {
    const int to = FindRevisitNode(poses, timestamps_ns, from);
    if (to < 0) continue;
    const int64_t stamp_to = timestamps_ns[static_cast<size_t>(to)], stamp_from = timestamps_ns[from];
    const auto it_to = std::lower_bound(stamps_in_bag.begin(), stamps_in_bag.end(), stamp_to);
    const auto it_from = std::lower_bound(stamps_in_bag.begin(), stamps_in_bag.end(), stamp_from);
    if (it_to == stamps_in_bag.end() || it_from == stamps_in_bag.end()) continue;
    GroundTruthWanted w{stamp_from, stamp_to, GroundTruthGuess(poses[static_cast<size_t>(to)], poses[from])};
    AlignmentPair p;
    p.source = &clouds[static_cast<size_t>(it_from - stamps_in_bag.begin())];
    p.target = &clouds[static_cast<size_t>(it_to - stamps_in_bag.begin())];
    p.guess = w.gt;
    wanted->push_back(w);
    pairs->push_back(p);
  }
}

// The tool's loop (gen_ground_truth_by_ndt_match.cc:151-261) for --method icp over the constraints whose `from` nodes are
// given (the caller has dropped the intra-submap ones, :153): the text of the tool's file for them, in order.
// poses, timestamps_ns: one a node; stamps_in_bag (sorted) and clouds: one a scan of the bag.  A `from` node without a
// revisit node (FindRevisitNode: -1) is skipped; so is a pair with a stamp past the bag's last (:173-180) and a pair whose
// alignment does not converge (:205).  Alignments run batch_size pairs a call, with the GroundTruthIcp preset; the text is
// byte-equal to the loop through IterativeClosestPoint::GroundTruthIcp one pair at a time, whatever batch_size and build are.
inline std::string GenerateGroundTruthIcp(Context* context, const std::vector<transform::Rigid3d>& poses,
                                          const std::vector<int64_t>& timestamps_ns, const std::vector<int64_t>& stamps_in_bag,
                                          const std::vector<sensor::PointCloud>& clouds, const std::vector<size_t>& from_nodes,
                                          size_t batch_size, IndexBuild build = IndexBuild::kOneByOne) {
  if (batch_size < 1 || clouds.size() != stamps_in_bag.size() || timestamps_ns.size() != poses.size())
    Check(DLIOM_ERR_INVALID_ARGUMENT, "GenerateGroundTruthIcp");
  std::vector<GroundTruthWanted> wanted;
  std::vector<AlignmentPair> pairs;
  CollectGroundTruthPairs(poses, timestamps_ns, stamps_in_bag, clouds, from_nodes, &wanted, &pairs);
  const dliom_icp_options options = IterativeClosestPoint::GroundTruthIcp(context)->options();
  std::string text;
  for (size_t first = 0; first < pairs.size(); first += batch_size) {
    const size_t end = std::min(pairs.size(), first + batch_size);
    const std::vector<AlignmentPair> group(pairs.begin() + static_cast<std::ptrdiff_t>(first), pairs.begin() + static_cast<std::ptrdiff_t>(end));
    const std::vector<dliom_icp_result> results = AlignPairs(context, options, group, nullptr, nullptr, nullptr, build);
    for (size_t i = first; i < end; ++i) {
      const dliom_icp_result& r = results[i - first];
      if (r.converged == 0) continue;
      Matrix4f trans;
      for (int k = 0; k < 16; ++k) trans.m[k] = static_cast<float>(r.transform[k]);
      text += FormatGroundTruthLine(wanted[i].stamp_from, wanted[i].stamp_to, r.fitness_score, trans,
                                    GroundTruthDifferenceNorm(wanted[i].gt, trans));
    }
  }
  return text;
}

// pcl::ApproximateVoxelGrid<PointXYZ> as PCL 1.8.0 runs it (MatchByNDT filters both clouds with it at 0.2 m), on the HOST:
// the sequential loop of the definition in dliom.h ("the approximate voxel grid"), which
// dliom_cloud_approximate_voxel_filter replays on the device, bit for bit; this class is the cross-check of that call
// (tests/cpp/approx_voxel_adapter.cc).  xyz only; the points are taken to be finite.
class ApproximateVoxelGrid {
 public:
  void setLeafSize(float x, float y, float z) {
    if (!(x > 0.f) || y != x || z != x) Check(DLIOM_ERR_INVALID_ARGUMENT, "ApproximateVoxelGrid::setLeafSize: one positive edge");
    leaf_ = x;
  }
  void setInputCloud(const sensor::PointCloud* cloud) { input_ = cloud; }
  void filter(sensor::PointCloud* output) const {
    if (input_ == nullptr || output == nullptr || output == input_) Check(DLIOM_ERR_INVALID_ARGUMENT, "ApproximateVoxelGrid::filter");
    struct Slot {
      int ix, iy, iz, count;
      float sx, sy, sz;
    };
    std::vector<Slot> slots(512, Slot{0, 0, 0, 0, 0.f, 0.f, 0.f});
    const auto flush = [output](const Slot& s) {
      const float n = static_cast<float>(s.count);
      output->push_back(sensor::Vector3f(s.sx / n, s.sy / n, s.sz / n));
    };
    output->clear();
    const float inv = 1.0f / leaf_;
    for (const sensor::Vector3f& p : *input_) {
      const int ix = static_cast<int>(std::floor(p.x * inv)), iy = static_cast<int>(std::floor(p.y * inv)),
                iz = static_cast<int>(std::floor(p.z * inv));
      const unsigned hash = static_cast<unsigned>(ix) * 7171u + static_cast<unsigned>(iy) * 3079u + static_cast<unsigned>(iz) * 4231u;
      Slot& s = slots[hash & 511u];
      if (s.count != 0 && (s.ix != ix || s.iy != iy || s.iz != iz)) {
        flush(s);
        s.count = 0;
      }
      if (s.count == 0) s = Slot{ix, iy, iz, 0, 0.f, 0.f, 0.f};
      s.sx += p.x;
      s.sy += p.y;
      s.sz += p.z;
      ++s.count;
    }
    for (const Slot& s : slots)
      if (s.count != 0) flush(s);
  }

 private:
  float leaf_ = 0.2f;
  const sensor::PointCloud* input_ = nullptr;
};

// pcl::NormalDistributionsTransform<PointXYZ, PointXYZ> as gen_ground_truth_by_ndt_match.cc:142-145,211-222 and
// LocalTrajectoryBuilder3D::MatchByNDT (local_trajectory_builder_3d.cc:969-1008) use it, with PCL's method names, on the
// device (dliom.h "scan alignment by NDT").  Parity unpinned against PCL (dliom.h).
class NormalDistributionsTransform {
 public:
  explicit NormalDistributionsTransform(Context* context) : context_(context) {
    Check(dliom_ndt_default_options(&options_), "dliom_ndt_default_options");
  }
  ~NormalDistributionsTransform() { Reset(); }
  NormalDistributionsTransform(const NormalDistributionsTransform&) = delete;
  NormalDistributionsTransform& operator=(const NormalDistributionsTransform&) = delete;

  void setTransformationEpsilon(double epsilon) { options_.transformation_epsilon = epsilon; }
  void setStepSize(double step) { options_.step_size = step; }
  void setMaximumIterations(int iterations) { options_.maximum_iterations = iterations; }
  void setOulierRatio(double ratio) { options_.outlier_ratio = ratio; }  // PCL's own spelling
  void setStepMode(int mode) { options_.step_mode = mode; }              // DLIOM_NDT_STEP_*
  // call before setInputTarget, which builds the cells (PCL rebuilds them here)
  void setResolution(float resolution) {
    if (target_ != nullptr) Check(DLIOM_ERR_INVALID_ARGUMENT, "NormalDistributionsTransform::setResolution after setInputTarget");
    options_.resolution = static_cast<double>(resolution);
  }
  void setInputSource(const sensor::PointCloud* cloud) { source_ = cloud; }
  // builds the target's cells and, for getFitnessScore(), its nearest-neighbour index
  void setInputTarget(const sensor::PointCloud* cloud, bool want_fitness_score = true) {
    if (cloud == nullptr) Check(DLIOM_ERR_INVALID_ARGUMENT, "NormalDistributionsTransform::setInputTarget");
    Reset();
    dliom_cloud* target = nullptr;
    Check(dliom_cloud_create(context_->get(), cloud->empty() ? nullptr : &(*cloud)[0].x, static_cast<int64_t>(cloud->size()), &target),
          "dliom_cloud_create");
    int status = dliom_ndt_target_create(context_->get(), target, &options_, &target_);
    if (status == DLIOM_OK && want_fitness_score) status = dliom_nn_index_create(context_->get(), target, nullptr, &index_);
    dliom_cloud_destroy(target);
    if (status != DLIOM_OK) Reset();
    Check(status, "dliom_ndt_target_create");
  }
  // output (may be null): the source under the final transformation
  void align(sensor::PointCloud* output, const Matrix4f& guess = Matrix4f::Identity()) {
    if (source_ == nullptr || target_ == nullptr) Check(DLIOM_ERR_INVALID_ARGUMENT, "NormalDistributionsTransform::align: no input");
    dliom_cloud* source = nullptr;
    Check(dliom_cloud_create(context_->get(), source_->empty() ? nullptr : &(*source_)[0].x, static_cast<int64_t>(source_->size()),
                             &source),
          "dliom_cloud_create");
    double guess16[16];
    for (int k = 0; k < 16; ++k) guess16[k] = static_cast<double>(guess.m[k]);
    dliom_cloud* aligned = nullptr;
    const int status = dliom_ndt_align(target_, source, guess16, &options_, index_, &result_, output != nullptr ? &aligned : nullptr);
    dliom_cloud_destroy(source);
    Check(status, "dliom_ndt_align");
    if (output != nullptr) {
      output->resize(source_->size());
      const int download = output->empty() ? DLIOM_OK : dliom_cloud_download(aligned, &(*output)[0].x);
      dliom_cloud_destroy(aligned);
      Check(download, "dliom_cloud_download");
    }
  }
  bool hasConverged() const { return result_.converged != 0; }
  double getFitnessScore() const { return result_.fitness_score; }
  double getTransformationProbability() const { return result_.transformation_probability; }
  int getFinalNumIteration() const { return result_.iterations; }
  Matrix4f getFinalTransformation() const {
    Matrix4f out;
    for (int k = 0; k < 16; ++k) out.m[k] = static_cast<float>(result_.transform[k]);
    return out;
  }
  const dliom_ndt_result& result() const { return result_; }
  const dliom_ndt_options& options() const { return options_; }

  // gen_ground_truth_by_ndt_match.cc:142-145 and local_trajectory_builder_3d.cc:981-984: epsilon 0.01, step 0.1, resolution
  // 1.0, 35 iterations -- the library's defaults
  static std::unique_ptr<NormalDistributionsTransform> GroundTruthNdt(Context* context) {
    return std::unique_ptr<NormalDistributionsTransform>(new NormalDistributionsTransform(context));
  }

 private:
  void Reset() {
    dliom_ndt_target_destroy(target_);
    dliom_nn_index_destroy(index_);
    target_ = nullptr;
    index_ = nullptr;
  }
  Context* context_;
  dliom_ndt_options options_;
  dliom_ndt_result result_ = {};
  const sensor::PointCloud* source_ = nullptr;
  dliom_ndt_target* target_ = nullptr;
  dliom_nn_index* index_ = nullptr;
};

// Many NDT targets in one call (dliom_ndt_target_create_batch): what NormalDistributionsTransform::setInputTarget builds
// cloud by cloud with `ndt_options`, cell for cell and bit for bit, in one device chain a chunk.  clouds: clouds of the
// context, none empty; a cloud may be named more than once.  -> a target a cloud, the caller's to destroy
// (dliom_ndt_target_destroy), each on its own.  limits: NULL = the defaults.  stats (may be null): the call's.
inline std::vector<dliom_ndt_target*> BuildNdtTargets(Context* context, const dliom_ndt_options& ndt_options,
                                                      const std::vector<const dliom_cloud*>& clouds,
                                                      const dliom_ndt_target_batch_limits* limits = nullptr,
                                                      dliom_ndt_target_batch_stats* stats = nullptr) {
  std::vector<dliom_ndt_target*> targets(clouds.size(), nullptr);
  dliom_ndt_target* none = nullptr;
  Check(dliom_ndt_target_create_batch(context->get(), clouds.data(), static_cast<int>(clouds.size()), &ndt_options, limits,
                                      targets.empty() ? &none : targets.data(), stats),
        "dliom_ndt_target_create_batch");
  return targets;
}

// Many NDT alignments in one call (dliom_ndt_align_batch): the pairs of the tool's loop under --method ndt.  What
// NormalDistributionsTransform with `ndt_options` gives pair by pair (setInputSource, setInputTarget(target, with_fitness),
// align(guess), result()), bit for bit but for read_backs (dliom.h).  ONE dliom_ndt_target is built per distinct target
// pointer, all of them in ONE call (BuildNdtTargets) -- and with with_fitness ONE nearest-neighbour index for
// getFitnessScore() -- and one cloud uploaded per distinct source pointer, however many pairs name them; everything is
// destroyed on every way out.  limits: NULL = the defaults.
// aligned (may be null): every pair's source under its final transformation.  stats (may be null): the call's.  build:
// kBatched builds the fitness indices in ONE call too (BuildNnIndices).
inline std::vector<dliom_ndt_result> AlignPairsNdt(Context* context, const dliom_ndt_options& ndt_options,
                                                   const std::vector<AlignmentPair>& pairs, bool with_fitness = true,
                                                   const dliom_ndt_batch_limits* limits = nullptr,
                                                   std::vector<sensor::PointCloud>* aligned = nullptr,
                                                   dliom_ndt_batch_stats* stats = nullptr, IndexBuild build = IndexBuild::kOneByOne) {
  struct Owned {  // destroyed on every way out, the targets and indices before nothing else depends on them
    std::map<const sensor::PointCloud*, dliom_ndt_target*> targets;
    std::map<const sensor::PointCloud*, dliom_nn_index*> indices;
    std::map<const sensor::PointCloud*, dliom_cloud*> sources;
    std::vector<dliom_cloud*> target_clouds, outputs;
    ~Owned() {
      for (auto& e : targets) dliom_ndt_target_destroy(e.second);
      for (auto& e : indices) dliom_nn_index_destroy(e.second);
      for (auto& e : sources) dliom_cloud_destroy(e.second);
      for (dliom_cloud* c : target_clouds) dliom_cloud_destroy(c);
      for (dliom_cloud* c : outputs) dliom_cloud_destroy(c);
    }
  } owned;
  const auto upload = [context](const sensor::PointCloud* cloud) {
    dliom_cloud* out = nullptr;
    Check(dliom_cloud_create(context->get(), cloud->empty() ? nullptr : &(*cloud)[0].x, static_cast<int64_t>(cloud->size()), &out),
          "dliom_cloud_create");
    return out;
  };
  // the distinct target clouds, in the order of their first mention: uploaded, their cells built in one call, then their indices
  std::vector<const sensor::PointCloud*> distinct;
  for (const AlignmentPair& p : pairs) {
    if (p.source == nullptr || p.target == nullptr) Check(DLIOM_ERR_INVALID_ARGUMENT, "AlignPairsNdt: a pair without a cloud");
    if (std::find(distinct.begin(), distinct.end(), p.target) == distinct.end()) distinct.push_back(p.target);
  }
  for (const sensor::PointCloud* cloud : distinct) {
    owned.target_clouds.push_back(nullptr);
    owned.target_clouds.back() = upload(cloud);
  }
  {
    const std::vector<const dliom_cloud*> clouds(owned.target_clouds.begin(), owned.target_clouds.end());
    const std::vector<dliom_ndt_target*> built = BuildNdtTargets(context, ndt_options, clouds);
    for (size_t k = 0; k < distinct.size(); ++k) owned.targets[distinct[k]] = built[k];
  }
  if (with_fitness && build == IndexBuild::kBatched) {
    const std::vector<const dliom_cloud*> clouds(owned.target_clouds.begin(), owned.target_clouds.end());
    const std::vector<dliom_nn_index*> built = BuildNnIndices(context, clouds);
    for (size_t k = 0; k < distinct.size(); ++k) owned.indices[distinct[k]] = built[k];
  }
  for (size_t k = 0; with_fitness && build == IndexBuild::kOneByOne && k < distinct.size(); ++k) {
    dliom_nn_index* index = nullptr;
    Check(dliom_nn_index_create(context->get(), owned.target_clouds[k], nullptr, &index), "dliom_nn_index_create");
    owned.indices[distinct[k]] = index;
  }
  for (dliom_cloud*& c : owned.target_clouds) {  // as before: a target's cloud is gone before the sources are uploaded
    dliom_cloud_destroy(c);
    c = nullptr;
  }
  std::vector<dliom_ndt_pair> table(pairs.size());
  for (size_t i = 0; i < pairs.size(); ++i) {
    const AlignmentPair& p = pairs[i];
    if (owned.sources.find(p.source) == owned.sources.end()) owned.sources[p.source] = upload(p.source);
    table[i].target = owned.targets[p.target];
    table[i].source = owned.sources[p.source];
    table[i].fitness_index = with_fitness ? owned.indices[p.target] : nullptr;
    for (int k = 0; k < 16; ++k) table[i].guess[k] = static_cast<double>(p.guess.m[k]);
  }
  std::vector<dliom_ndt_result> results(pairs.size());
  if (aligned != nullptr) owned.outputs.assign(pairs.size(), nullptr);
  Check(dliom_ndt_align_batch(context->get(), table.data(), static_cast<int>(table.size()), &ndt_options, limits, results.data(),
                              aligned != nullptr ? owned.outputs.data() : nullptr, stats),
        "dliom_ndt_align_batch");
  if (aligned != nullptr) {
    aligned->assign(pairs.size(), sensor::PointCloud());
    for (size_t i = 0; i < pairs.size(); ++i) {
      (*aligned)[i].resize(pairs[i].source->size());
      if (!(*aligned)[i].empty()) Check(dliom_cloud_download(owned.outputs[i], &(*aligned)[i][0].x), "dliom_cloud_download");
    }
  }
  return results;
}

// The tool's loop (gen_ground_truth_by_ndt_match.cc:151-261) for --method ndt (:211-222), GenerateGroundTruthIcp's other
// half: the same pairs (CollectGroundTruthPairs), aligned batch_size pairs a call with the GroundTruthNdt preset on the raw
// clouds, getFitnessScore() as the alignment error, a pair that does not converge dropped (:218).  The text is byte-equal
// to the loop through NormalDistributionsTransform::GroundTruthNdt one pair at a time, whatever batch_size and build are.
inline std::string GenerateGroundTruthNdt(Context* context, const std::vector<transform::Rigid3d>& poses,
                                          const std::vector<int64_t>& timestamps_ns, const std::vector<int64_t>& stamps_in_bag,
                                          const std::vector<sensor::PointCloud>& clouds, const std::vector<size_t>& from_nodes,
                                          size_t batch_size, IndexBuild build = IndexBuild::kOneByOne) {
  if (batch_size < 1 || clouds.size() != stamps_in_bag.size() || timestamps_ns.size() != poses.size())
    Check(DLIOM_ERR_INVALID_ARGUMENT, "GenerateGroundTruthNdt");
  std::vector<GroundTruthWanted> wanted;
  std::vector<AlignmentPair> pairs;
  CollectGroundTruthPairs(poses, timestamps_ns, stamps_in_bag, clouds, from_nodes, &wanted, &pairs);
  const dliom_ndt_options options = NormalDistributionsTransform::GroundTruthNdt(context)->options();
  std::string text;
  for (size_t first = 0; first < pairs.size(); first += batch_size) {
    const size_t end = std::min(pairs.size(), first + batch_size);
    const std::vector<AlignmentPair> group(pairs.begin() + static_cast<std::ptrdiff_t>(first), pairs.begin() + static_cast<std::ptrdiff_t>(end));
    const std::vector<dliom_ndt_result> results = AlignPairsNdt(context, options, group, true, nullptr, nullptr, nullptr, build);
    for (size_t i = first; i < end; ++i) {
      const dliom_ndt_result& r = results[i - first];
      if (r.converged == 0) continue;
      Matrix4f trans;
      for (int k = 0; k < 16; ++k) trans.m[k] = static_cast<float>(r.transform[k]);
      text += FormatGroundTruthLine(wanted[i].stamp_from, wanted[i].stamp_to, r.fitness_score, trans,
                                    GroundTruthDifferenceNorm(wanted[i].gt, trans));
    }
  }
  return text;
}

// LocalTrajectoryBuilder3D::MatchByNDT (local_trajectory_builder_3d.cc:969-1008): both clouds through ApproximateVoxelGrid
// at 0.2 m, NDT of the filtered current scan against the filtered previous one from init_guess; -> the final
// transformation's rotation (row-major) and translation, as floats like the reference's Matrix4f.  The target is rebuilt
// for every pair.
inline void MatchByNDT(Context* context, const sensor::PointCloud& pre_scan, const sensor::PointCloud& cur_scan, const Matrix4f& init_guess,
                       float rotation9[9], float translation3[3]) {
  sensor::PointCloud pre_filtered, cur_filtered;
  ApproximateVoxelGrid filter;
  filter.setLeafSize(0.2f, 0.2f, 0.2f);
  filter.setInputCloud(&pre_scan);
  filter.filter(&pre_filtered);
  filter.setInputCloud(&cur_scan);
  filter.filter(&cur_filtered);
  NormalDistributionsTransform ndt(context);
  ndt.setInputSource(&cur_filtered);
  ndt.setInputTarget(&pre_filtered, false);
  ndt.align(nullptr, init_guess);
  const Matrix4f t = ndt.getFinalTransformation();
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) rotation9[3 * r + c] = t(r, c);
    translation3[r] = t(r, 3);
  }
}

// MatchByNDT over a stream of scans, as InitilizeByNDT calls it (local_trajectory_builder_3d.cc:231-330): every scan is
// filtered once, on the device, and aligned to its predecessor, whose cells stay there (dliom_ndt_scan_matcher).  For every
// pair the rotation and translation are, bit for bit, MatchByNDT's above for the same two raw scans and guess.
class NdtScanMatcher {
 public:
  explicit NdtScanMatcher(Context* context, float leaf = 0.2f) {
    dliom_ndt_options options;
    Check(dliom_ndt_default_options(&options), "dliom_ndt_default_options");
    Check(dliom_ndt_scan_matcher_create(context->get(), &options, leaf, &matcher_), "dliom_ndt_scan_matcher_create");
  }
  ~NdtScanMatcher() { dliom_ndt_scan_matcher_destroy(matcher_); }
  NdtScanMatcher(const NdtScanMatcher&) = delete;
  NdtScanMatcher& operator=(const NdtScanMatcher&) = delete;
  // -> false for the first scan (nothing is written), true for every later one.  `scan`: a cloud of the matcher's context
  // (dliom_cloud_create of a host cloud; dliom_timed_cloud_points of a decoded, stamped or merged one)
  bool Match(const dliom_cloud* scan, const Matrix4f& init_guess, float rotation9[9], float translation3[3]) {
    double guess16[16];
    for (int k = 0; k < 16; ++k) guess16[k] = static_cast<double>(init_guess.m[k]);
    dliom_ndt_result result = {};
    int had_target = 0;
    Check(dliom_ndt_scan_matcher_has_target(matcher_, &had_target), "dliom_ndt_scan_matcher_has_target");
    Check(dliom_ndt_scan_matcher_match(matcher_, scan, guess16, &result), "dliom_ndt_scan_matcher_match");
    if (had_target == 0) return false;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) rotation9[3 * r + c] = static_cast<float>(result.transform[4 * r + c]);
      translation3[r] = static_cast<float>(result.transform[4 * r + 3]);
    }
    return true;
  }

 private:
  dliom_ndt_scan_matcher* matcher_ = nullptr;
};
}  // namespace registration
}  // namespace dliom

#endif  // DLIOM_CPP_DLIOM_CARTOGRAPHER_H_
