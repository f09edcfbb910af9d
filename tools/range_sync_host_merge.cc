// The host path of two lidars' scans as the adapter runs it for host clouds (d-liom_amd/cpp/dliom_cartographer.h): the
// RangeDataSynchronizer's copy, merge and std::sort of 20-byte records, then the repack into the two vectors
// dliom_range_accumulator_add takes.  tools/range_sync_bench.py builds this into a shared library and times it as the
// parent path's middle part.
#include <cstring>

#include "dliom_cartographer.h"

using namespace dliom;

// xyzt arrays in, merged xyzt (capacity n_primary + n_secondary points) and origin index out; returns the merged size, or
// -1 when the synchronizer did not merge
extern "C" long long range_sync_host_merge(const float* primary, long long n_primary, long long primary_time, const float* secondary,
                                           long long n_secondary, long long secondary_time, int descrew, float* merged_xyzt,
                                           float* merged_index) {
  mapping::RangeDataSynchronizer synchronizer({"lidar_a", "lidar_b"});
  sensor::TimedPointCloudData a, b;
  a.time = primary_time;
  b.time = secondary_time;
  a.origin = b.origin = sensor::Vector3f(0.f, 0.f, 0.f);
  a.ranges.resize(static_cast<size_t>(n_primary));
  b.ranges.resize(static_cast<size_t>(n_secondary));
  static_assert(sizeof(sensor::TimedPoint) == 16, "packed x, y, z, t");
  if (n_primary > 0) std::memcpy(&a.ranges[0].x, primary, 16 * static_cast<size_t>(n_primary));
  if (n_secondary > 0) std::memcpy(&b.ranges[0].x, secondary, 16 * static_cast<size_t>(n_secondary));
  synchronizer.AddRangeData("lidar_b", b, descrew != 0);
  const sensor::TimedPointCloudOriginData sync = synchronizer.AddRangeData("lidar_a", a, descrew != 0);
  if (sync.origins.size() != 2) return -1;
  for (size_t i = 0; i < sync.ranges.size(); ++i) {  // LocalTrajectoryBuilder3D::AddRangeData's repack
    merged_xyzt[4 * i] = sync.ranges[i].point_time.x;
    merged_xyzt[4 * i + 1] = sync.ranges[i].point_time.y;
    merged_xyzt[4 * i + 2] = sync.ranges[i].point_time.z;
    merged_xyzt[4 * i + 3] = sync.ranges[i].point_time.t;
    merged_index[i] = static_cast<float>(sync.ranges[i].origin_index);
  }
  return static_cast<long long>(sync.ranges.size());
}
