// transform::TransformInterpolationBuffer and io::AssemblePointsBatch of dliom_cartographer.h at the head of the export
// chain: one message assembled on the device, then MinMaxRangeFiteringPointsProcessor -> OutlierRemovingPointsProcessor
// (its first phase: the hits marked).  The chain runs twice: on the assembled batch, whose points are on the device
// already, and on a copy without device_points, which is uploaded the way every batch was before.
//
//   assemble_adapter in.bin out.bin voxel_size min_range max_range
//     in.bin:  int64 nodes | int64 time[nodes] | double pose7[nodes] | int64 cloud_time | double sensor_to_tracking[7] |
//              int64 n | float xyzt[4 n]          (intensity of point i = i)
//     out.bin: int64 kept | float xyz[3 kept] | float intensity[kept] | float origin[3] | int64 start_time |
//              per chain: int64 uploads | int64 voxels | int32 xyz[3 voxels] | int32 hits[voxels]
//              int32 Has(earliest - 1), Has(earliest), Has(latest), Has(latest + 1) | double Lookup(earliest)[7]
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "dliom_cartographer.h"

namespace io = dliom::io;

class Sink : public io::PointsProcessor {
 public:
  void Process(std::unique_ptr<io::PointsBatch>) override { std::abort(); }  // the first phase passes nothing on
  FlushResult Flush() override { return FlushResult::kFinished; }
};

static void Chain(std::unique_ptr<io::PointsBatch> batch, double voxel_size, double min_range, double max_range,
                  dliom::Context* context, std::FILE* out) {
  Sink sink;
  io::OutlierRemovingPointsProcessor remover(voxel_size, &sink, context);
  io::MinMaxRangeFiteringPointsProcessor range_filter(min_range, max_range, &remover, context);
  const int64_t before = io::internal::DeviceCloud::Uploads();
  range_filter.Process(std::move(batch));
  const int64_t uploads = io::internal::DeviceCloud::Uploads() - before;
  int64_t voxels = 0;
  dliom::Check(dliom_outlier_remover_voxels(remover.remover(), nullptr, nullptr, nullptr, 0, &voxels), "voxels");
  std::vector<int32_t> xyz(3 * static_cast<size_t>(voxels) + 1), hits(static_cast<size_t>(voxels) + 1), rays(hits.size());
  if (voxels > 0)
    dliom::Check(dliom_outlier_remover_voxels(remover.remover(), xyz.data(), hits.data(), rays.data(), voxels, &voxels), "voxels");
  std::fwrite(&uploads, 8, 1, out);
  std::fwrite(&voxels, 8, 1, out);
  std::fwrite(xyz.data(), 12, static_cast<size_t>(voxels), out);
  std::fwrite(hits.data(), 4, static_cast<size_t>(voxels), out);
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (in == nullptr || out == nullptr) return 2;
  int64_t nodes = 0, cloud_time = 0, n = 0;
  if (std::fread(&nodes, 8, 1, in) != 1 || nodes < 1) return 2;
  std::vector<int64_t> times(static_cast<size_t>(nodes));
  std::vector<double> poses(7 * times.size());
  double mount[7];
  if (std::fread(times.data(), 8, times.size(), in) != times.size() || std::fread(poses.data(), 8, poses.size(), in) != poses.size() ||
      std::fread(&cloud_time, 8, 1, in) != 1 || std::fread(mount, 8, 7, in) != 7 || std::fread(&n, 8, 1, in) != 1 || n < 1)
    return 2;
  dliom::sensor::TimedPointCloud points(static_cast<size_t>(n));
  if (std::fread(&points[0].x, 16, points.size(), in) != points.size()) return 2;
  std::vector<float> intensities;
  for (int64_t i = 0; i < n; ++i) intensities.push_back(static_cast<float>(i));

  dliom::Context context(0);
  dliom::transform::TransformInterpolationBuffer buffer(&context);
  if (!buffer.empty() || buffer.Has(times[0])) return 3;
  for (int64_t i = 0; i < nodes; ++i) {
    buffer.Push(times[static_cast<size_t>(i)], dliom::transform::Rigid3d::FromArray(&poses[7 * static_cast<size_t>(i)]));
    if (i == 0 && !buffer.Has(times[0])) return 3;  // the trajectory behind the buffer is made again after the next Push
  }
  if (buffer.empty() || buffer.earliest_time() != times.front() || buffer.latest_time() != times.back()) return 3;

  const int64_t before = io::internal::DeviceCloud::Uploads();
  std::unique_ptr<io::PointsBatch> batch =
      io::AssemblePointsBatch(buffer, cloud_time, points, intensities, dliom::transform::Rigid3d::FromArray(mount), "lidar", &context);
  if (io::internal::DeviceCloud::Uploads() != before) return 4;
  if (batch == nullptr || batch->frame_id != "lidar" || batch->device_points == nullptr ||
      batch->intensities.size() != batch->points.size())
    return 4;
  const int64_t kept = static_cast<int64_t>(batch->points.size());
  std::fwrite(&kept, 8, 1, out);
  std::fwrite(batch->points.data(), 12, batch->points.size(), out);
  std::fwrite(batch->intensities.data(), 4, batch->intensities.size(), out);
  std::fwrite(&batch->origin.x, 4, 3, out);
  std::fwrite(&batch->start_time, 8, 1, out);

  std::unique_ptr<io::PointsBatch> old_way(new io::PointsBatch(*batch));
  old_way->device_points.reset();
  Chain(std::move(batch), std::atof(argv[3]), std::atof(argv[4]), std::atof(argv[5]), &context, out);
  Chain(std::move(old_way), std::atof(argv[3]), std::atof(argv[4]), std::atof(argv[5]), &context, out);

  // a message whose times all lie behind the trajectory: null, as in the reference
  if (io::AssemblePointsBatch(buffer, times.back() + 20000000, points, intensities, dliom::transform::Rigid3d(), "lidar") != nullptr)
    return 5;
  const int32_t has[4] = {buffer.Has(times.front() - 1), buffer.Has(times.front()), buffer.Has(times.back()), buffer.Has(times.back() + 1)};
  std::fwrite(has, 4, 4, out);
  const std::array<double, 7> first = buffer.Lookup(times.front()).ToArray();
  std::fwrite(first.data(), 8, 7, out);
  std::fclose(out);
  return 0;
}
