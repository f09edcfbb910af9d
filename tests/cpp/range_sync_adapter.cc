// Two lidars through SensorBridge::HandlePointCloud2Message -> LocalTrajectoryBuilder3D::AddRangeData on the device path
// (the synchronizer's device overload: stamp, merge and std::sort's order in HBM; the accumulator's device input), against
// the same messages decoded on the host by the one-thread model (point_cloud2_model.cc, linked in) into the host
// AddRangeData and its host RangeDataSynchronizer.  Input: the stream file of tests/cpp/ltb3d_adapter.cc, written by
// tests/test_gpu_range_sync.py.  Every scan becomes two Velodyne-shaped messages: "lidar_b" (the secondary; the scan seen
// from another mount, its sweep ending half a sweep before the prior one's) arrives first and waits, "lidar_a" then merges
// with it.  Usage: range_sync_adapter <stream> <num_accumulated_range_data> <manual de-skew 0|1> [sensor type].  Prints one
// DEVICE and one HOST line a result and the device path's counters; the test asserts the lines are equal and what the
// counters must be.  Sensor type "other" (no point times: the adapter leaves such merges to the host) wants de-skew on.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dliom_cartographer.h"

using namespace dliom;

extern "C" int point_cloud2_model(const dliom_point_cloud2* message, int mode, const double* sensor_to_tracking, float* xyzt,
                                  float* intensities, int64_t* kept, int* has_intensities, int64_t* time, float origin[3]);

static bool read_all(FILE* f, void* p, size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }

// the scan as a message of 22-byte records stamped at `first` ticks since stamp_sec0, the float `time` since then at offset 18
static sensor_msgs::PointCloud2 message_of(const std::vector<float>& scan, uint32_t stamp_sec0, int64_t first) {
  const size_t n = scan.size() / 4;
  sensor_msgs::PointCloud2 msg;
  const int64_t stamp = static_cast<int64_t>(stamp_sec0) * 10000000 + first;  // (`first` may lie before stamp_sec0)
  msg.header.stamp.sec = static_cast<uint32_t>(stamp / 10000000);
  msg.header.stamp.nsec = static_cast<uint32_t>(stamp % 10000000) * 100u;
  msg.height = 1;
  msg.width = static_cast<uint32_t>(n);
  msg.point_step = 22;
  msg.row_step = msg.width * msg.point_step;
  msg.fields = {{"x", 0, 7, 1}, {"y", 4, 7, 1}, {"z", 8, 7, 1}, {"intensity", 12, 7, 1}, {"ring", 16, 4, 1}, {"time", 18, 7, 1}};
  msg.data.assign(n * 22, 0);
  for (size_t i = 0; i < n; ++i) {
    const float since_first = scan[4 * i + 3] - scan[3];
    std::memcpy(msg.data.data() + 22 * i, &scan[4 * i], 12);
    std::memcpy(msg.data.data() + 22 * i + 18, &since_first, 4);
  }
  return msg;
}

static sensor::TimedPointCloudData decoded_on_host(const sensor_msgs::PointCloud2& msg, const transform::Rigid3d& mount, int mode) {
  std::vector<dliom_point_field> fields(msg.fields.size());
  for (size_t k = 0; k < fields.size(); ++k)
    fields[k] = dliom_point_field{msg.fields[k].name.c_str(), msg.fields[k].offset, msg.fields[k].datatype, msg.fields[k].count};
  dliom_point_cloud2 m{};
  m.height = msg.height;
  m.width = msg.width;
  m.point_step = msg.point_step;
  m.row_step = msg.row_step;
  m.num_fields = static_cast<int32_t>(fields.size());
  m.fields = fields.data();
  m.data = msg.data.data();
  m.data_size = msg.data.size();
  m.stamp_sec = msg.header.stamp.sec;
  m.stamp_nsec = msg.header.stamp.nsec;
  sensor::TimedPointCloudData cloud;
  cloud.ranges.resize(msg.width);
  int64_t kept = 0;
  int has = 0;
  float origin[3];
  const std::array<double, 7> mount7 = mount.ToArray();
  if (point_cloud2_model(&m, mode, mount7.data(), &cloud.ranges[0].x, nullptr, &kept, &has, &cloud.time,
                         origin) != DLIOM_OK)
    std::exit(3);
  cloud.ranges.resize(static_cast<size_t>(kept));
  cloud.origin = sensor::Vector3f(origin[0], origin[1], origin[2]);
  return cloud;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) return 2;
  int32_t header[4];  // num_scans, points_per_scan, imu_per_scan, (unused)
  double init[16];    // pose7, velocity3, bias6
  if (!read_all(f, header, sizeof header) || !read_all(f, init, sizeof init)) return 2;
  Context context(0);
  mapping::LocalTrajectoryBuilderOptions3D options;
  std::memset(&options.front_end, 0, sizeof options.front_end);
  if (!read_all(f, &options.front_end, sizeof options.front_end)) return 2;
  Check(dliom_imu_window_default_options(&options.imu), "dliom_imu_window_default_options");
  double imu_noise[4];
  if (!read_all(f, imu_noise, sizeof imu_noise)) return 2;
  options.imu.acc_noise = imu_noise[0];
  options.imu.gyr_noise = imu_noise[1];
  options.imu.acc_bias_noise = imu_noise[2];
  options.imu.gyr_bias_noise = imu_noise[3];
  options.num_accumulated_range_data = std::atoi(argv[2]);
  options.enable_manual_descrew = std::atoi(argv[3]) != 0;
  options.min_range = 1.f;
  options.max_range = 100.f;
  options.voxel_filter_size = 0.15f;
  options.scan_period = 0.1;
  const std::string sensor_type = argc > 4 ? argv[4] : "velodyne";  // "other": no point times, t = 0 (column times)
  const int mode = SensorBridge::ModeOf(sensor_type);
  const std::vector<std::string> sensors = {"lidar_a", "lidar_b"};
  mapping::LocalTrajectoryBuilder3D on_device(&context, options, sensors), on_host(&context, options, sensors);
  for (mapping::LocalTrajectoryBuilder3D* b : {&on_device, &on_host})
    b->SetInitialState(transform::Rigid3d::FromArray(init), transform::Vector3d{{init[7], init[8], init[9]}}, init + 10);
  SensorBridge bridge(&context, &on_device);
  const transform::Rigid3d mount_a(transform::Vector3d{{0.02, -0.01, 0.03}}, transform::Quaterniond{{0.99995, 0.006, -0.005, 0.004}});
  const transform::Rigid3d mount_b(transform::Vector3d{{-0.03, 0.02, 0.05}}, transform::Quaterniond{{0.99995, -0.004, 0.006, 0.005}});
  const uint32_t stamp_sec0 = 1790000000u;
  const int64_t ticks0 = (static_cast<int64_t>(stamp_sec0) + 719162LL * 86400LL) * 10000000LL;
  int64_t t = 0;
  int results[2] = {0, 0}, waiting[2] = {0, 0};
  for (int s = 0; s < header[0]; ++s) {
    std::vector<double> imu(static_cast<size_t>(header[2]) * 7);  // dt, acc3, gyr3
    if (!read_all(f, imu.data(), imu.size() * 8)) return 2;
    for (int k = 0; k < header[2]; ++k) {
      t += static_cast<int64_t>(imu[7 * k] * 1e7 + 0.5);
      sensor::ImuData d;
      d.time = ticks0 + t;
      std::memcpy(d.linear_acceleration, &imu[7 * k + 1], 24);
      std::memcpy(d.angular_velocity, &imu[7 * k + 4], 24);
      on_device.AddImuData(d);
      on_host.AddImuData(d);
    }
    std::vector<float> scan(4 * static_cast<size_t>(header[1]));
    if (!read_all(f, scan.data(), scan.size() * 4)) return 2;
    const int64_t first = t + static_cast<int64_t>(static_cast<double>(scan[3]) * 1e7);
    const sensor_msgs::PointCloud2 msg_b = message_of(scan, stamp_sec0, first - 500000), msg_a = message_of(scan, stamp_sec0, first);
    const auto report = [&](const char* who, int which, const std::unique_ptr<mapping::LocalTrajectoryBuilder3D::MatchingResult>& r) {
      if (r == nullptr) return;
      const std::array<double, 7> p = r->local_pose.ToArray();
      std::printf("%s %d %lld %.17g %.17g %.17g %.17g %.17g %.17g %.17g %zu\n", who, s, static_cast<long long>(r->time), p[0], p[1], p[2],
                  p[3], p[4], p[5], p[6], r->range_data_in_local.returns.size());
      ++results[which];
    };
    // the secondary lidar's message waits in the synchronizer ...
    waiting[0] += bridge.HandlePointCloud2Message("lidar_b", msg_b, sensor_type, mount_b) == nullptr;
    waiting[1] += on_host.AddRangeData("lidar_b", decoded_on_host(msg_b, mount_b, mode)) == nullptr;
    // ... and the prior lidar's is merged with it
    report("DEVICE", 0, bridge.HandlePointCloud2Message("lidar_a", msg_a, sensor_type, mount_a));
    report("HOST", 1, on_host.AddRangeData("lidar_a", decoded_on_host(msg_a, mount_a, mode)));
  }
  std::fclose(f);
  if (results[0] != results[1] || waiting[0] != header[0] || waiting[1] != header[0]) return 5;
  std::printf("COUNTERS device_merges %lld merge_host_fallbacks %lld merges_left_to_host %lld downloads %lld\n",
              static_cast<long long>(on_device.device_merges()), static_cast<long long>(on_device.merge_host_fallbacks()),
              static_cast<long long>(on_device.merges_left_to_host()),
              static_cast<long long>(sensor::TimedCloudOnDevice::Downloads().load()));
  std::printf("RANGE SYNC ADAPTER DONE\n");
  return 0;
}
