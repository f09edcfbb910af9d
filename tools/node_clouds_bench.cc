// tools/node_clouds_bench.py's program: K kept scans of one filtered cloud in a cartographer_ros::NodeCloudCache, the device
// calls against the adapter's host loops (the reference's loops, one thread) in one process, alternating repetitions.
//   node_clouds_bench <cloud.bin (int32 n, n packed xyz)> <K> <repeats>
// The results are compared before anything is timed (exit 3 on a difference).  One line of medians on stdout.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../d-liom_amd/cpp/dliom_cartographer.h"

using namespace dliom;
using Cache = cartographer_ros::NodeCloudCache;

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  int32_t n = 0;
  if (f == nullptr || std::fread(&n, 4, 1, f) != 1) return 2;
  sensor::RangeData scan;
  scan.origin = sensor::Vector3f(0.5f, -0.25f, 1.5f);
  scan.returns.resize(static_cast<size_t>(n));
  if (std::fread(scan.returns.data(), 12, scan.returns.size(), f) != scan.returns.size()) return 2;
  std::fclose(f);
  const int k = std::atoi(argv[2]), repeats = std::atoi(argv[3]);
  const double local_pose[7] = {12.5, -3.25, 0.75, 0.9238795325112867, 0.0, 0.0, 0.3826834323650898};
  const double to_map_d[7] = {-1.5, 2.25, 0.125, 0.9807852804032304, 0.0, 0.19509032201612825, 0.0};
  const transform::Rigid3d pose = transform::Rigid3d::FromArray(local_pose), to_map = transform::Rigid3d::FromArray(to_map_d);
  const std::array<float, 7> to_map_f = transform::Rigid3f(to_map).ToArray();

  Context context(0);
  Cache cache(&context);
  for (int i = 0; i < k; ++i) cache.OnLocalSlamResult(0, 636000000000000000ll + 1000 * i, pose, scan);

  std::vector<uint8_t> host, device;
  std::vector<int64_t> offsets(static_cast<size_t>(k) + 1);
  auto host_clouds = [&] {
    host.clear();
    for (int i = 0; i < k; ++i) Cache::HostPointCloud2Data(scan.returns, to_map_f.data(), 1, &host);
  };
  auto host_protos = [&] {
    host.clear();
    for (int i = 0; i < k; ++i) Cache::HostNodeRangeData(0, 636000000000000000ll + 1000 * i, pose, scan, &host);
  };
  auto device_clouds = [&] { device = cache.FullMapCloud(to_map).data; };
  auto device_protos = [&] {
    device.clear();
    cache.SerializeRangeData([&](const uint8_t* data, size_t size) { device.insert(device.end(), data, data + size); });
  };
  // the sizing half of to_proto alone: the size launch, the scan and the polled read-back of every chunk
  auto device_sizes = [&] { Check(dliom_node_clouds_to_proto(cache.get(), 0, k, nullptr, nullptr, 0, offsets.data(), nullptr), "sizes"); };

  // the C calls straight into one page-locked buffer the caller keeps (dliom_host_register): no vector is made or zeroed,
  // and the download is one DMA instead of a staged copy into pageable memory
  const size_t pinned_capacity = static_cast<size_t>(k) * (DLIOM_NODE_RANGE_MAX_HEADER + DLIOM_NODE_RANGE_MAX_RECORD * static_cast<size_t>(n));
  std::vector<uint8_t> pinned(pinned_capacity);
  Check(dliom_host_register(context.get(), pinned.data(), pinned.size()), "dliom_host_register");
  dliom_node_clouds_transform to_map_transform;
  to_map_transform.num_poses = 1;
  to_map_transform.per_node = 0;
  to_map_transform.poses7 = to_map_f.data();
  auto pinned_clouds = [&] {
    Check(dliom_node_clouds_pack_point_cloud2(cache.get(), 0, k, &to_map_transform, nullptr, pinned.data(), static_cast<int64_t>(pinned.size()),
                                              offsets.data(), nullptr), "pack_point_cloud2");
  };
  auto pinned_protos = [&] {
    Check(dliom_node_clouds_to_proto(cache.get(), 0, k, nullptr, pinned.data(), static_cast<int64_t>(pinned.size()), offsets.data(), nullptr), "to_proto");
  };

  host_clouds();
  device_clouds();
  if (host != device) return 3;
  pinned_clouds();
  if (static_cast<size_t>(offsets[k]) != host.size() || !std::equal(host.begin(), host.end(), pinned.begin())) return 3;
  const size_t cloud_bytes = device.size();
  host_protos();
  device_protos();
  if (host != device) return 3;
  const size_t proto_bytes = device.size();
  pinned_protos();
  if (static_cast<size_t>(offsets[k]) != host.size() || !std::equal(host.begin(), host.end(), pinned.begin())) return 3;

  std::vector<double> t[7];
  for (int r = 0; r < repeats + 1; ++r) {  // (the first round warms up)
    double t0 = now_ms();
    device_clouds();
    double t1 = now_ms();
    host_clouds();
    double t2 = now_ms();
    device_protos();
    double t3 = now_ms();
    host_protos();
    double t4 = now_ms();
    device_sizes();
    double t5 = now_ms();
    pinned_clouds();
    double t6 = now_ms();
    pinned_protos();
    double t7 = now_ms();
    if (r == 0) continue;
    t[5].push_back(t6 - t5);
    t[6].push_back(t7 - t6);
    t[0].push_back(t1 - t0);
    t[1].push_back(t2 - t1);
    t[2].push_back(t3 - t2);
    t[3].push_back(t4 - t3);
    t[4].push_back(t5 - t4);
  }
  const double points = static_cast<double>(n) * k;
  std::printf("K %d points %d cloud_bytes %zu proto_bytes %zu | pack_point_cloud2 device_ms %.3f host_ms %.3f device_Mpts_s %.1f host_Mpts_s %.1f "
              "page_locked_ms %.3f | to_proto device_ms %.3f host_ms %.3f device_Mpts_s %.1f host_Mpts_s %.1f sizing_ms %.3f "
              "emit_and_download_ms %.3f page_locked_ms %.3f\n",
              k, n, cloud_bytes, proto_bytes, median(t[0]), median(t[1]), points / median(t[0]) / 1e3, points / median(t[1]) / 1e3, median(t[5]), median(t[2]),
              median(t[3]), points / median(t[2]) / 1e3, points / median(t[3]) / 1e3, median(t[4]), median(t[2]) - median(t[4]), median(t[6]));
  Check(dliom_host_unregister(context.get(), pinned.data()), "dliom_host_unregister");
  return 0;
}
