// The export pipeline of dliom_cartographer.h, twice over the same messages:
//   assemble -> min_max_range_filter -> fixed_ratio_sampler -> voxel_filter_and_remove_moving_objects (three phases)
//            -> intensity_to_color -> write_xray_image -> write_ply
//   device:  AssemblePointsBatch(kOnDevice, ...) and the adapter's processors: the batch stays in HBM between the stages
//   host:    AssemblePointsBatch's host vectors through the processors as they were before batches lived on the device,
//            with the reference's sampler and PLY loops (written out below) for the two stages that had no device form
//
//   points_batch_adapter in.bin out.bin voxel_size min_range max_range ratio xray_voxel_size [repeats]
//     in.bin:  int64 nodes | int64 time[nodes] | double pose7[nodes] | double sensor_to_tracking[7] | int64 scans |
//              per scan: int64 cloud_time | int64 n | float xyzt[4 n] | float intensity[n]
//     out.bin: per run (device, host): int64 file bytes | the PLY file | int64 width | int64 height | uint32 pixels
//              then int64 uploads, int64 downloaded bytes, int64 PLY record bytes of the device run
//     repeats > 0: both runs `repeats` more times, warm; prints "device_ms host_ms" (medians of the whole pipeline)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_set>
#include <vector>

#include "dliom_cartographer.h"

namespace io = dliom::io;

struct Message {
  int64_t cloud_time;
  dliom::sensor::TimedPointCloud points;
  std::vector<float> intensities;
};

class MemoryFile : public io::FileWriter {
 public:
  explicit MemoryFile(std::string* out) : out_(out) { out_->clear(); }
  bool Write(const char* data, size_t len) override {
    out_->append(data, len);
    return true;
  }
  bool WriteHeader(const char* data, size_t len) override {
    if (out_->size() < len) out_->resize(len);
    out_->replace(0, len, data, len);
    return true;
  }
  bool Close() override { return true; }
  std::string GetFilename() override { return "points.ply"; }

 private:
  std::string* const out_;
};

class Sink : public io::PointsProcessor {  // reads nothing: the batch is dropped where it is
 public:
  void Process(std::unique_ptr<io::PointsBatch>) override {}
  FlushResult Flush() override { return FlushResult::kFinished; }
};

// common::FixedRatioSampler and io::FixedRatioSamplingPointsProcessor on host vectors, from the reference's text
class HostSampler : public io::PointsProcessor {
 public:
  HostSampler(double ratio, io::PointsProcessor* next) : ratio_(ratio), next_(next) {}
  void Process(std::unique_ptr<io::PointsBatch> batch) override {
    std::unordered_set<int> to_remove;
    for (size_t i = 0; i < batch->points.size(); ++i) {
      ++num_pulses_;
      if (static_cast<double>(num_samples_) / num_pulses_ < ratio_) ++num_samples_;
      else to_remove.insert(static_cast<int>(i));
    }
    io::PointsBatch kept;  // RemovePoints
    for (size_t i = 0; i < batch->points.size(); ++i) {
      if (to_remove.count(static_cast<int>(i)) == 1) continue;
      kept.points.push_back(batch->points[i]);
      if (!batch->colors.empty()) kept.colors.push_back(batch->colors[i]);
      if (!batch->intensities.empty()) kept.intensities.push_back(batch->intensities[i]);
    }
    batch->points = std::move(kept.points);
    batch->intensities = std::move(kept.intensities);
    batch->colors = std::move(kept.colors);
    batch->device_points.reset();
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override {
    if (next_->Flush() == FlushResult::kFinished) return FlushResult::kFinished;
    num_pulses_ = num_samples_ = 0;
    return FlushResult::kRestartStream;
  }

 private:
  const double ratio_;
  io::PointsProcessor* const next_;
  int64_t num_pulses_ = 0, num_samples_ = 0;
};

// io::PlyWritingPointsProcessor on host vectors, from the reference's text (header by snprintf: 15 digits, zero-padded)
class HostPly : public io::PointsProcessor {
 public:
  HostPly(std::string* file, io::PointsProcessor* next) : file_(file), next_(next) { file_->clear(); }
  void Process(std::unique_ptr<io::PointsBatch> batch) override {
    if (batch->points.empty()) {
      next_->Process(std::move(batch));
      return;
    }
    if (num_points_ == 0) {
      has_colors_ = !batch->colors.empty();
      has_intensities_ = !batch->intensities.empty();
      *file_ = Header(0);
    }
    for (size_t i = 0; i < batch->points.size(); ++i) {
      file_->append(reinterpret_cast<const char*>(&batch->points[i].x), 12);
      if (has_colors_) {
        char c[3];
        for (int k = 0; k < 3; ++k) {
          const float v = batch->colors[i][k];
          const float clamped = v > 1.f ? 1.f : (v < 0.f ? 0.f : v);
          c[k] = static_cast<char>(static_cast<uint8_t>(std::lround(clamped * 255)));
        }
        file_->append(c, 3);
      }
      if (has_intensities_) file_->append(reinterpret_cast<const char*>(&batch->intensities[i]), 4);
      ++num_points_;
    }
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override {
    const std::string header = Header(num_points_);
    file_->replace(0, header.size(), header);
    return next_->Flush();
  }

 private:
  std::string Header(int64_t n) const {
    char count[32];
    std::snprintf(count, sizeof count, "%015lld", static_cast<long long>(n));
    return std::string("ply\nformat binary_little_endian 1.0\ncomment generated by Cartographer\nelement vertex ") + count +
           "\nproperty float x\nproperty float y\nproperty float z\n" +
           (has_colors_ ? "property uchar red\nproperty uchar green\nproperty uchar blue\n" : "") +
           (has_intensities_ ? "property float intensity\n" : "") + "end_header\n";
  }
  std::string* const file_;
  io::PointsProcessor* const next_;
  int64_t num_points_ = 0;
  bool has_colors_ = false, has_intensities_ = false;
};

struct Options {
  double voxel_size, min_range, max_range, ratio, xray_voxel_size;
};

struct Output {
  std::string ply;
  io::XRayPointsProcessor::XRayImage image;
};

static void Stream(io::PointsProcessor* head, const dliom::transform::TransformInterpolationBuffer& buffer,
                   const std::vector<Message>& messages, const dliom::transform::Rigid3d& mount, bool on_device,
                   dliom::Context* context) {
  io::PointsProcessor::FlushResult result;
  do {  // assets_writer.cc: the whole stream again while Flush asks for it
    for (const Message& m : messages) {
      std::unique_ptr<io::PointsBatch> batch =
          on_device ? io::AssemblePointsBatch(io::kOnDevice, buffer, m.cloud_time, m.points, m.intensities, mount, "lidar", context)
                    : io::AssemblePointsBatch(buffer, m.cloud_time, m.points, m.intensities, mount, "lidar", context);
      if (batch != nullptr) head->Process(std::move(batch));
    }
    result = head->Flush();
  } while (result == io::PointsProcessor::FlushResult::kRestartStream);
}

static Output Run(bool on_device, const Options& o, const dliom::transform::TransformInterpolationBuffer& buffer,
                  const std::vector<Message>& messages, const dliom::transform::Rigid3d& mount, dliom::Context* context) {
  Output out;
  Sink sink;
  const auto keep_image = [&](const io::XRayPointsProcessor::XRayImage& image) { out.image = image; };
  const dliom::transform::Rigid3f view;  // the identity
  if (on_device) {
    io::PlyWritingPointsProcessor ply(std::unique_ptr<io::FileWriter>(new MemoryFile(&out.ply)), &sink, context);
    io::XRayPointsProcessor xray(o.xray_voxel_size, view, {}, "xray", keep_image, &ply, context);
    io::IntensityToColorPointsProcessor to_color(0.f, 255.f, "", &xray);
    io::OutlierRemovingPointsProcessor remover(o.voxel_size, &to_color, context);
    io::FixedRatioSamplingPointsProcessor sampler(o.ratio, &remover, context);
    io::MinMaxRangeFiteringPointsProcessor range_filter(o.min_range, o.max_range, &sampler, context);
    Stream(&range_filter, buffer, messages, mount, true, context);
  } else {
    HostPly ply(&out.ply, &sink);
    io::XRayPointsProcessor xray(o.xray_voxel_size, view, {}, "xray", keep_image, &ply, context);
    io::IntensityToColorPointsProcessor to_color(0.f, 255.f, "", &xray);
    io::OutlierRemovingPointsProcessor remover(o.voxel_size, &to_color, context);
    HostSampler sampler(o.ratio, &remover);
    io::MinMaxRangeFiteringPointsProcessor range_filter(o.min_range, o.max_range, &sampler, context);
    Stream(&range_filter, buffer, messages, mount, false, context);
  }
  return out;
}

static void Put(std::FILE* f, const Output& o) {
  const int64_t bytes = static_cast<int64_t>(o.ply.size()), w = o.image.width, h = o.image.height;
  std::fwrite(&bytes, 8, 1, f);
  std::fwrite(o.ply.data(), 1, o.ply.size(), f);
  std::fwrite(&w, 8, 1, f);
  std::fwrite(&h, 8, 1, f);
  std::fwrite(o.image.pixels.data(), 4, o.image.pixels.size(), f);
}

static double Median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (in == nullptr || out == nullptr) return 2;
  const Options o{std::atof(argv[3]), std::atof(argv[4]), std::atof(argv[5]), std::atof(argv[6]), std::atof(argv[7])};
  const int repeats = argc > 8 ? std::atoi(argv[8]) : 0;
  int64_t nodes = 0, scans = 0;
  if (std::fread(&nodes, 8, 1, in) != 1 || nodes < 1) return 2;
  std::vector<int64_t> times(static_cast<size_t>(nodes));
  std::vector<double> poses(7 * times.size());
  double mount7[7];
  if (std::fread(times.data(), 8, times.size(), in) != times.size() || std::fread(poses.data(), 8, poses.size(), in) != poses.size() ||
      std::fread(mount7, 8, 7, in) != 7 || std::fread(&scans, 8, 1, in) != 1 || scans < 1)
    return 2;
  std::vector<Message> messages(static_cast<size_t>(scans));
  for (Message& m : messages) {
    int64_t n = 0;
    if (std::fread(&m.cloud_time, 8, 1, in) != 1 || std::fread(&n, 8, 1, in) != 1 || n < 1) return 2;
    m.points.resize(static_cast<size_t>(n));
    m.intensities.resize(static_cast<size_t>(n));
    if (std::fread(&m.points[0].x, 16, m.points.size(), in) != m.points.size() ||
        std::fread(m.intensities.data(), 4, m.intensities.size(), in) != m.intensities.size())
      return 2;
  }
  dliom::Context context(0);
  dliom::transform::TransformInterpolationBuffer buffer(&context);
  for (int64_t i = 0; i < nodes; ++i)
    buffer.Push(times[static_cast<size_t>(i)], dliom::transform::Rigid3d::FromArray(&poses[7 * static_cast<size_t>(i)]));
  const dliom::transform::Rigid3d mount = dliom::transform::Rigid3d::FromArray(mount7);

  const int64_t uploads0 = io::internal::DeviceCloud::Uploads(), bytes0 = io::internal::DeviceBatch::DownloadedBytes();
  const Output device = Run(true, o, buffer, messages, mount, &context);
  const int64_t uploads = io::internal::DeviceCloud::Uploads() - uploads0;
  const int64_t downloaded = io::internal::DeviceBatch::DownloadedBytes() - bytes0;
  const Output host = Run(false, o, buffer, messages, mount, &context);
  Put(out, device);
  Put(out, host);
  int64_t header = 0;
  dliom::Check(dliom_ply_header(1, 1, 0, nullptr, 0, &header) == DLIOM_ERR_CAPACITY ? DLIOM_OK : DLIOM_ERR_INTERNAL, "dliom_ply_header");
  const int64_t records = static_cast<int64_t>(device.ply.size()) - header;
  std::fwrite(&uploads, 8, 1, out);
  std::fwrite(&downloaded, 8, 1, out);
  std::fwrite(&records, 8, 1, out);
  std::fclose(out);
  if (repeats > 0) {
    std::vector<double> ms[2];
    for (int which = 0; which < 2; ++which)
      for (int r = 0; r < repeats; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        Run(which == 0, o, buffer, messages, mount, &context);
        ms[which].push_back(1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
      }
    std::printf("%.6f %.6f\n", Median(ms[0]), Median(ms[1]));
  }
  return 0;
}
