// cartographer_ros::NodeCloudCache (d-liom_amd/cpp/dliom_cartographer.h) driven like the D-LIOM fork drives its kept scans.
//   nodes <in> <out>    the scans of <in> through OnLocalSlamResult's host overload, then SerializeRangeData, FullMapCloud and
//                       GlobalClouds; each is compared here with the adapter's host loops (exit 3 on a difference) and
//                       written to <out>, where tests/test_gpu_node_clouds.py compares it with its model
//   frontend <stream>   tests/cpp/ltb3d_adapter.cc's stream through LocalTrajectoryBuilder3D with a cache set: every
//                       MatchingResult's range_data_in_local equals what the cache kept of it, bit for bit (exit 4 otherwise)
//   g++ -std=c++17 node_clouds_adapter.cc -L../../d-liom_amd -ldliom
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../d-liom_amd/cpp/dliom_cartographer.h"

using namespace dliom;

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static void write_blob(FILE* f, const std::vector<uint8_t>& data, const std::vector<int64_t>& offsets) {
  const int64_t sizes[2] = {static_cast<int64_t>(offsets.size()), static_cast<int64_t>(data.size())};
  std::fwrite(sizes, 8, 2, f);
  std::fwrite(offsets.data(), 8, offsets.size(), f);
  if (!data.empty()) std::fwrite(data.data(), 1, data.size(), f);
}

struct Scan {
  int32_t trajectory_id;
  int64_t time;
  double local_pose[7];
  sensor::RangeData range_data;
};

static int run_nodes(const char* in, const char* out) {
  FILE* f = std::fopen(in, "rb");
  if (f == nullptr) return 2;
  int32_t counts[2];  // scans, node table entries
  double local_to_map[7];
  if (!read_all(f, counts, sizeof counts) || !read_all(f, local_to_map, sizeof local_to_map)) return 2;
  std::map<int64_t, transform::Rigid3d> node_table;
  for (int i = 0; i < counts[1]; ++i) {
    int64_t time;
    double pose[7];
    if (!read_all(f, &time, 8) || !read_all(f, pose, sizeof pose)) return 2;
    node_table[time] = transform::Rigid3d::FromArray(pose);
  }
  std::vector<Scan> scans(static_cast<size_t>(counts[0]));
  for (Scan& s : scans) {
    int32_t head[3];  // trajectory, returns, misses
    float origin[3];
    if (!read_all(f, head, sizeof head) || !read_all(f, &s.time, 8) || !read_all(f, s.local_pose, sizeof s.local_pose) ||
        !read_all(f, origin, sizeof origin))
      return 2;
    s.trajectory_id = head[0];
    s.range_data.origin = sensor::Vector3f(origin[0], origin[1], origin[2]);
    s.range_data.returns.resize(static_cast<size_t>(head[1]));
    s.range_data.misses.resize(static_cast<size_t>(head[2]));
    if (!read_all(f, s.range_data.returns.data(), 12 * s.range_data.returns.size()) ||
        !read_all(f, s.range_data.misses.data(), 12 * s.range_data.misses.size()))
      return 2;
  }
  std::fclose(f);

  Context context(0);
  cartographer_ros::NodeCloudCache cache(&context);
  std::map<int, std::vector<size_t>> by_trajectory;  // range_data_local_all_'s order
  for (size_t i = 0; i < scans.size(); ++i) {
    const Scan& s = scans[i];
    cache.OnLocalSlamResult(s.trajectory_id, s.time, transform::Rigid3d::FromArray(s.local_pose), s.range_data);
    by_trajectory[s.trajectory_id].push_back(i);
  }
  FILE* o = std::fopen(out, "wb");
  if (o == nullptr) return 2;

  // SerializeRangeData against the host loop
  std::vector<uint8_t> device, host;
  std::vector<int64_t> device_offsets{0}, host_offsets{0};
  cache.SerializeRangeData([&](const uint8_t* data, size_t size) {
    device.insert(device.end(), data, data + size);
    device_offsets.push_back(static_cast<int64_t>(device.size()));
  });
  for (const auto& trajectory : by_trajectory)
    for (size_t i : trajectory.second) {
      const Scan& s = scans[i];
      cartographer_ros::NodeCloudCache::HostNodeRangeData(s.trajectory_id, s.time, transform::Rigid3d::FromArray(s.local_pose), s.range_data, &host);
      host_offsets.push_back(static_cast<int64_t>(host.size()));
    }
  if (device != host || device_offsets != host_offsets) return 3;
  write_blob(o, device, device_offsets);

  // FullMapCloud
  const transform::Rigid3d to_map = transform::Rigid3d::FromArray(local_to_map);
  const cartographer_ros::NodeCloudCache::CloudData full = cache.FullMapCloud(to_map);
  host.clear();
  host_offsets.assign(1, 0);
  const std::array<float, 7> to_map_f = transform::Rigid3f(to_map).ToArray();
  for (const auto& trajectory : by_trajectory)
    for (size_t i : trajectory.second) {
      cartographer_ros::NodeCloudCache::HostPointCloud2Data(scans[i].range_data.returns, to_map_f.data(), 1, &host);
      host_offsets.push_back(static_cast<int64_t>(host.size()));
    }
  if (full.data != host || full.offsets != host_offsets) return 3;
  write_blob(o, full.data, full.offsets);

  // GlobalClouds: cache order (the file's order), scans the table lacks skipped
  const cartographer_ros::NodeCloudCache::CloudData global = cache.GlobalClouds(node_table);
  host.clear();
  host_offsets.assign(1, 0);
  std::vector<int64_t> kept;
  for (size_t i = 0; i < scans.size(); ++i) {
    const auto found = node_table.find(scans[i].time);
    if (found == node_table.end()) continue;
    const std::array<float, 7> local = transform::Rigid3f(transform::Rigid3d::FromArray(scans[i].local_pose)).ToArray();
    const std::array<float, 7> global_pose = transform::Rigid3f(found->second).ToArray();
    float poses[14];
    Check(dliom_rigid3f_inverse(local.data(), poses), "dliom_rigid3f_inverse");
    std::copy(global_pose.begin(), global_pose.end(), poses + 7);
    cartographer_ros::NodeCloudCache::HostPointCloud2Data(scans[i].range_data.returns, poses, 2, &host);
    host_offsets.push_back(static_cast<int64_t>(host.size()));
    kept.push_back(static_cast<int64_t>(i));
  }
  if (global.data != host || global.offsets != host_offsets || global.nodes != kept) return 3;
  write_blob(o, global.data, global.offsets);
  std::fclose(o);
  std::printf("NODE CLOUDS ADAPTER DONE scans %zu kept %zu\n", scans.size(), kept.size());
  return 0;
}

static int run_front_end(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (f == nullptr) return 2;
  int32_t header[4];  // num_scans, points_per_scan, imu_per_scan, num_accumulated_range_data
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
  options.num_accumulated_range_data = header[3];
  options.min_range = 1.f;
  options.max_range = 100.f;
  options.voxel_filter_size = 0.15f;
  options.scan_period = 0.1;
  cartographer_ros::NodeCloudCache cache(&context);
  mapping::LocalTrajectoryBuilder3D builder(&context, options, {"lidar"});
  builder.SetNodeCloudCache(&cache, 7);
  builder.SetInitialState(transform::Rigid3d::FromArray(init), transform::Vector3d{{init[7], init[8], init[9]}}, init + 10);
  int64_t t = 0;
  int results = 0;
  for (int s = 0; s < header[0]; ++s) {
    std::vector<double> imu(static_cast<size_t>(header[2]) * 7);  // dt, acc3, gyr3
    if (!read_all(f, imu.data(), imu.size() * 8)) return 2;
    for (int k = 0; k < header[2]; ++k) {
      t += static_cast<int64_t>(imu[7 * k] * 1e7 + 0.5);
      sensor::ImuData d;
      d.time = t;
      std::memcpy(d.linear_acceleration, &imu[7 * k + 1], 24);
      std::memcpy(d.angular_velocity, &imu[7 * k + 4], 24);
      builder.AddImuData(d);
    }
    sensor::TimedPointCloudData cloud;
    cloud.time = t;
    cloud.origin = sensor::Vector3f{0.f, 0.f, 0.f};
    cloud.ranges.resize(static_cast<size_t>(header[1]));
    if (!read_all(f, cloud.ranges.data(), cloud.ranges.size() * 16)) return 2;
    std::unique_ptr<mapping::LocalTrajectoryBuilder3D::MatchingResult> r = builder.AddRangeData("lidar", cloud);
    if (r == nullptr) continue;
    if (r->node_cloud_index != results) return 4;
    dliom_node_cloud_info info;
    int64_t num_returns = -1, num_misses = -1;
    Check(dliom_node_clouds_info(cache.get(), r->node_cloud_index, &info, &num_returns, &num_misses), "dliom_node_clouds_info");
    const sensor::RangeData& want = r->range_data_in_local;
    if (num_returns != static_cast<int64_t>(want.returns.size()) || num_misses != 0 || want.returns.empty()) return 4;
    sensor::PointCloud kept(want.returns.size());
    Check(dliom_node_clouds_download(cache.get(), r->node_cloud_index, &kept[0].x, nullptr), "dliom_node_clouds_download");
    if (std::memcmp(kept.data(), want.returns.data(), 12 * kept.size()) != 0) return 4;
    const std::array<double, 7> pose = r->local_pose.ToArray();
    if (info.timestamp != r->time || info.trajectory_id != 7 || std::memcmp(info.local_pose7, pose.data(), sizeof info.local_pose7) != 0 ||
        std::memcmp(info.origin_in_local, &want.origin.x, 12) != 0)
      return 4;
    ++results;
  }
  std::fclose(f);
  std::printf("NODE CLOUDS FRONT END DONE results %d\n", results);
  return results > 0 ? 0 : 4;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "nodes") return run_nodes(argv[2], argv[3]);
  if (argc == 3 && std::string(argv[1]) == "frontend") return run_front_end(argv[2]);
  return 2;
}
