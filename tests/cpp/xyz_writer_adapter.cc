// The tail of the export pipeline of dliom_cartographer.h, twice over the same messages:
//   assemble -> min_max_range_filter -> frame_id_filter -> dump_num_points -> write_xyz
//   device:  AssemblePointsBatch(kOnDevice, ...) and the adapter's processors: the batch stays in HBM up to the writer,
//            which brings back the text and nothing else
//   host:    AssemblePointsBatch's host vectors, the adapter's range filter, and the reference's frame filter, counter and
//            XYZ loop on host vectors (written out below, from the reference's text)
//
//   xyz_writer_adapter in.bin out.bin min_range max_range
//     in.bin:  int64 nodes | int64 time[nodes] | double pose7[nodes] | double sensor_to_tracking[7] | int64 scans |
//              per scan: int64 cloud_time | int64 n | int64 name bytes | frame_id | float xyzt[4 n] | float intensity[n]
//     out.bin: per run (device, host): int64 file bytes | int64 counted points | the XYZ file
//              then int64 uploads, int64 downloaded bytes of the device run
// Frames named "dropped" are dropped (drop_frames = {"dropped"}); every other frame is kept.
#include <cstdio>
#include <cstdlib>
#include <iomanip>
#include <memory>
#include <sstream>
#include <string>
#include <unordered_set>
#include <vector>

#include "dliom_cartographer.h"

namespace io = dliom::io;

struct Message {
  int64_t cloud_time;
  std::string frame_id;
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
  bool Close() override { return true; }
  std::string GetFilename() override { return "points.xyz"; }

 private:
  std::string* const out_;
};

class Sink : public io::PointsProcessor {  // reads nothing: the batch is dropped where it is
 public:
  void Process(std::unique_ptr<io::PointsBatch>) override {}
  FlushResult Flush() override { return FlushResult::kFinished; }
};

// io::XyzWriterPointsProcessor on host vectors, from the reference's text
class HostXyz : public io::PointsProcessor {
 public:
  HostXyz(std::string* file, io::PointsProcessor* next) : file_(file), next_(next) { file_->clear(); }
  void Process(std::unique_ptr<io::PointsBatch> batch) override {
    for (const dliom::sensor::Vector3f& point : batch->points) {
      std::ostringstream stream;
      stream << std::setprecision(6);
      stream << point.x << " " << point.y << " " << point.z << "\n";
      file_->append(stream.str());
    }
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override { return next_->Flush(); }

 private:
  std::string* const file_;
  io::PointsProcessor* const next_;
};

// io::CountingPointsProcessor on host vectors
class HostCounter : public io::PointsProcessor {
 public:
  explicit HostCounter(io::PointsProcessor* next) : next_(next) {}
  void Process(std::unique_ptr<io::PointsBatch> batch) override {
    num_points_ += static_cast<int64_t>(batch->points.size());
    next_->Process(std::move(batch));
  }
  FlushResult Flush() override { return next_->Flush(); }
  int64_t num_points() const { return num_points_; }

 private:
  io::PointsProcessor* const next_;
  int64_t num_points_ = 0;
};

// io::FrameIdFilteringPointsProcessor with drop_frames
class HostFrameDrop : public io::PointsProcessor {
 public:
  HostFrameDrop(const std::unordered_set<std::string>& drop, io::PointsProcessor* next) : drop_(drop), next_(next) {}
  void Process(std::unique_ptr<io::PointsBatch> batch) override {
    if (!drop_.count(batch->frame_id)) next_->Process(std::move(batch));
  }
  FlushResult Flush() override { return next_->Flush(); }

 private:
  const std::unordered_set<std::string> drop_;
  io::PointsProcessor* const next_;
};

struct Output {
  std::string file;
  int64_t counted = 0;
};

static void Stream(io::PointsProcessor* head, const dliom::transform::TransformInterpolationBuffer& buffer,
                   const std::vector<Message>& messages, const dliom::transform::Rigid3d& mount, bool on_device,
                   dliom::Context* context) {
  for (const Message& m : messages) {
    std::unique_ptr<io::PointsBatch> batch =
        on_device ? io::AssemblePointsBatch(io::kOnDevice, buffer, m.cloud_time, m.points, m.intensities, mount, m.frame_id, context)
                  : io::AssemblePointsBatch(buffer, m.cloud_time, m.points, m.intensities, mount, m.frame_id, context);
    if (batch != nullptr) head->Process(std::move(batch));
  }
  if (head->Flush() != io::PointsProcessor::FlushResult::kFinished) std::abort();
}

static Output Run(bool on_device, double min_range, double max_range, const dliom::transform::TransformInterpolationBuffer& buffer,
                  const std::vector<Message>& messages, const dliom::transform::Rigid3d& mount, dliom::Context* context) {
  Output out;
  Sink sink;
  const std::unordered_set<std::string> drop{"dropped"};
  if (on_device) {
    io::XyzWriterPointsProcessor xyz(std::unique_ptr<io::FileWriter>(new MemoryFile(&out.file)), &sink, context);
    io::CountingPointsProcessor counter(&xyz, context);
    io::FrameIdFilteringPointsProcessor frames({}, drop, &counter);
    io::MinMaxRangeFiteringPointsProcessor range_filter(min_range, max_range, &frames, context);
    Stream(&range_filter, buffer, messages, mount, true, context);
    out.counted = counter.num_points();
  } else {
    HostXyz xyz(&out.file, &sink);
    HostCounter counter(&xyz);
    HostFrameDrop frames(drop, &counter);
    io::MinMaxRangeFiteringPointsProcessor range_filter(min_range, max_range, &frames, context);
    Stream(&range_filter, buffer, messages, mount, false, context);
    out.counted = counter.num_points();
  }
  return out;
}

static void Put(std::FILE* f, const Output& o) {
  const int64_t bytes = static_cast<int64_t>(o.file.size());
  std::fwrite(&bytes, 8, 1, f);
  std::fwrite(&o.counted, 8, 1, f);
  std::fwrite(o.file.data(), 1, o.file.size(), f);
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (in == nullptr || out == nullptr) return 2;
  const double min_range = std::atof(argv[3]), max_range = std::atof(argv[4]);
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
    int64_t n = 0, name = 0;
    if (std::fread(&m.cloud_time, 8, 1, in) != 1 || std::fread(&n, 8, 1, in) != 1 || n < 1 || std::fread(&name, 8, 1, in) != 1 ||
        name < 0 || name > 255)
      return 2;
    m.frame_id.resize(static_cast<size_t>(name));
    if (name > 0 && std::fread(&m.frame_id[0], 1, m.frame_id.size(), in) != m.frame_id.size()) return 2;
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
  const Output device = Run(true, min_range, max_range, buffer, messages, mount, &context);
  const int64_t uploads = io::internal::DeviceCloud::Uploads() - uploads0;
  const int64_t downloaded = io::internal::DeviceBatch::DownloadedBytes() - bytes0;
  const Output host = Run(false, min_range, max_range, buffer, messages, mount, &context);
  Put(out, device);
  Put(out, host);
  std::fwrite(&uploads, 8, 1, out);
  std::fwrite(&downloaded, 8, 1, out);
  std::fclose(out);
  return 0;
}
