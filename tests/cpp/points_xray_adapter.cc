// The X-ray and colouring adapters of dliom_cartographer.h driven like an asset-writer pipeline (the stock
// assets_writer_backpack_3d configuration's shape): a stream of batches with intensities through
//   MinMaxRangeFiteringPointsProcessor -> XRayPointsProcessor yz, xy, xz -> IntensityToColorPointsProcessor ->
//   XRayPointsProcessor yz, xy, xz -> ColoringPointsProcessor (255, 100, 0) -> XRayPointsProcessor xy -> end,
// then one Flush().  tests/test_gpu_points_xray.py compares the seven images with the model's and checks that every batch
// went to the device once.
//
//   points_xray_adapter batches.bin out.bin voxel_size min_range max_range
//     batches.bin: int32 count; per batch float origin[3], int32 n, n * 3 floats, n intensities
//     out.bin: per image in Flush order: int32 length of the file name, the name, int32 width, height, the pixels;
//              then int64 clouds uploaded from host points, int64 batches that reached the end
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "dliom_cartographer.h"

namespace io = dliom::io;

class End : public io::PointsProcessor {
 public:
  void Process(std::unique_ptr<io::PointsBatch> batch) override {
    if (batch->colors.size() != batch->points.size()) std::abort();
    ++batches;
  }
  FlushResult Flush() override { return FlushResult::kFinished; }
  int64_t batches = 0;
};

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (in == nullptr || out == nullptr) return 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, in) != 1) return 2;
  std::vector<io::PointsBatch> batches(static_cast<size_t>(count));
  for (io::PointsBatch& b : batches) {
    int32_t n = 0;
    if (std::fread(&b.origin.x, 4, 3, in) != 3 || std::fread(&n, 4, 1, in) != 1) return 2;
    b.points.resize(static_cast<size_t>(n));
    b.intensities.resize(static_cast<size_t>(n));
    if (n > 0 && (std::fread(&b.points[0].x, 12, b.points.size(), in) != b.points.size() ||
                  std::fread(b.intensities.data(), 4, b.intensities.size(), in) != b.intensities.size()))
      return 2;
    b.frame_id = "horizontal_laser";
  }
  const double voxel_size = std::atof(argv[3]);
  // YZ_TRANSFORM, XY_TRANSFORM, XZ_TRANSFORM of the stock configurations (roll, pitch, yaw = (0, 0, pi), (0, -pi/2, 0),
  // (0, 0, -pi/2)) as the quaternions RollPitchYaw gives, cast to float
  const dliom::transform::Rigid3f yz(dliom::transform::Rigid3d({{0, 0, 0}}, {{6.123233995736766e-17, 0, 0, 1.0}}));
  const dliom::transform::Rigid3f xy(dliom::transform::Rigid3d({{0, 0, 0}}, {{0.7071067811865476, 0, -0.7071067811865475, 0}}));
  const dliom::transform::Rigid3f xz(dliom::transform::Rigid3d({{0, 0, 0}}, {{0.7071067811865476, 0, 0, -0.7071067811865475}}));
  const io::XRayPointsProcessor::ImageSink sink = [out](const io::XRayPointsProcessor::XRayImage& image) {
    const int32_t length = static_cast<int32_t>(image.filename.size()), size[2] = {image.width, image.height};
    std::fwrite(&length, 4, 1, out);
    std::fwrite(image.filename.data(), 1, image.filename.size(), out);
    std::fwrite(size, 4, 2, out);
    std::fwrite(image.pixels.data(), 4, image.pixels.size(), out);
  };
  dliom::Context context(0);
  const int64_t uploads_before = io::internal::DeviceCloud::Uploads();
  End end;
  io::XRayPointsProcessor xy_constant(voxel_size, xy, {}, "xray_xy_constant", sink, &end, &context);
  io::ColoringPointsProcessor coloring(io::ColoringPointsProcessor::FromUint8(255, 100, 0), "horizontal_laser", &xy_constant);
  io::XRayPointsProcessor xz_intensity(voxel_size, xz, {}, "xray_xz_intensity", sink, &coloring, &context);
  io::XRayPointsProcessor xy_intensity(voxel_size, xy, {}, "xray_xy_intensity", sink, &xz_intensity, &context);
  io::XRayPointsProcessor yz_intensity(voxel_size, yz, {}, "xray_yz_intensity", sink, &xy_intensity, &context);
  io::IntensityToColorPointsProcessor intensity(0.f, 255.f, "", &yz_intensity);
  io::XRayPointsProcessor xz_gray(voxel_size, xz, {}, "xray_xz_gray", sink, &intensity, &context);
  io::XRayPointsProcessor xy_gray(voxel_size, xy, {}, "xray_xy_gray", sink, &xz_gray, &context);
  io::XRayPointsProcessor yz_gray(voxel_size, yz, {}, "xray_yz_gray", sink, &xy_gray, &context);
  io::MinMaxRangeFiteringPointsProcessor range_filter(std::atof(argv[4]), std::atof(argv[5]), &yz_gray, &context);
  for (const io::PointsBatch& b : batches) range_filter.Process(std::make_unique<io::PointsBatch>(b));
  if (range_filter.Flush() != io::PointsProcessor::FlushResult::kFinished) return 3;
  int32_t pixel[2];
  const int32_t origin[3] = {0, 0, 0};
  if (!yz_gray.VoxelIndexToPixel(origin, pixel) || pixel[0] < 0 || pixel[1] < 0) return 4;
  const int64_t counters[2] = {io::internal::DeviceCloud::Uploads() - uploads_before, end.batches};
  std::fwrite(counters, 8, 2, out);
  std::fclose(out);
  std::fclose(in);
  return 0;
}
