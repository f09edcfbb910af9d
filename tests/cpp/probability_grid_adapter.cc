// The io:: map stages of dliom_cartographer.h driven the way the reference's assets writer drives a pipeline: a stream
// of batches through MinMaxRangeFiteringPointsProcessor -> ProbabilityGridPointsProcessor ("write_probability_grid") ->
// RosMapWritingPointsProcessor ("write_ros_map") -> a collecting sink, until Flush() reports kFinished.  The Python side
// (tests/test_gpu_probability_grid.py) compares the PGM and YAML bytes, the gray image and the forwarded batches with
// what it assembles from the CPU oracle.
//
//   probability_grid_adapter batches.bin out_dir resolution min_range max_range
//     batches.bin: int32 count; per batch float origin[3], int32 n, n * 3 floats
//     out_dir/map.pgm, out_dir/map.yaml: what write_ros_map wrote through its FileWriters
//     out_dir/grid.bin: int32 width, height, offset x, offset y, then the gray bytes of write_probability_grid
//     out_dir/forwarded.bin: per batch that reached the sink: int32 n, n * 3 floats, n intensities
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dliom_cartographer.h"

namespace io = dliom::io;

class StreamFileWriter : public io::FileWriter {  // io/file_writer.h:52-66
 public:
  StreamFileWriter(const std::string& directory, const std::string& filename)
      : filename_(filename), out_(std::fopen((directory + "/" + filename).c_str(), "wb")) {}
  ~StreamFileWriter() override {
    if (out_ != nullptr) std::fclose(out_);
  }
  bool Write(const char* data, size_t len) override { return out_ != nullptr && std::fwrite(data, 1, len, out_) == len; }
  bool Close() override {
    if (out_ == nullptr) return false;
    const bool ok = std::fclose(out_) == 0;
    out_ = nullptr;
    return ok;
  }
  std::string GetFilename() override { return filename_; }

 private:
  const std::string filename_;
  std::FILE* out_;
};

class Sink : public io::PointsProcessor {
 public:
  explicit Sink(std::FILE* out) : out_(out) {}
  void Process(std::unique_ptr<io::PointsBatch> batch) override {
    const int32_t n = static_cast<int32_t>(batch->points.size());
    if (batch->intensities.size() != batch->points.size()) std::abort();
    std::fwrite(&n, 4, 1, out_);
    std::fwrite(batch->points.data(), 12, batch->points.size(), out_);
    std::fwrite(batch->intensities.data(), 4, batch->intensities.size(), out_);
    ++batches;
  }
  FlushResult Flush() override {
    ++flushes;
    return FlushResult::kFinished;
  }
  int batches = 0, flushes = 0;

 private:
  std::FILE* out_;
};

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const std::string directory = argv[2];
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* forwarded = std::fopen((directory + "/forwarded.bin").c_str(), "wb");
  std::FILE* grid_out = std::fopen((directory + "/grid.bin").c_str(), "wb");
  if (in == nullptr || forwarded == nullptr || grid_out == nullptr) return 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, in) != 1) return 2;
  std::vector<io::PointsBatch> batches(static_cast<size_t>(count));
  for (io::PointsBatch& b : batches) {
    int32_t n = 0;
    if (std::fread(&b.origin.x, 4, 3, in) != 3 || std::fread(&n, 4, 1, in) != 1) return 2;
    b.points.resize(static_cast<size_t>(n));
    if (n > 0 && std::fread(&b.points[0].x, 12, b.points.size(), in) != b.points.size()) return 2;
    for (int32_t i = 0; i < n; ++i) b.intensities.push_back(static_cast<float>(i));
  }
  std::fclose(in);
  const double resolution = std::atof(argv[3]);
  dliom::Context context(0);
  Sink sink(forwarded);
  const io::ProbabilityGridRangeDataInserterOptions2D options;  // 0.55 / 0.49, free space: assets_writer_ros_map.lua
  io::RosMapWritingPointsProcessor ros_map(
      resolution, options,
      [&](const std::string& filename) { return std::unique_ptr<io::FileWriter>(new StreamFileWriter(directory, filename)); }, "map",
      &sink, &context);
  int images = 0;
  io::ProbabilityGridPointsProcessor grid(
      resolution, options,
      [&](const std::vector<uint8_t>& gray, int width, int height, const int32_t offset[2]) {
        const int32_t head[4] = {width, height, offset[0], offset[1]};
        std::fwrite(head, 4, 4, grid_out);
        std::fwrite(gray.data(), 1, gray.size(), grid_out);
        ++images;
      },
      &ros_map, &context);
  io::MinMaxRangeFiteringPointsProcessor range_filter(std::atof(argv[4]), std::atof(argv[5]), &grid, &context);
  if (std::strcmp(io::ProbabilityGridPointsProcessor::kConfigurationFileActionName, "write_probability_grid") != 0 ||
      std::strcmp(io::RosMapWritingPointsProcessor::kConfigurationFileActionName, "write_ros_map") != 0)
    return 4;
  int passes = 0;
  do {
    for (const io::PointsBatch& b : batches) range_filter.Process(std::make_unique<io::PointsBatch>(b));
    ++passes;
  } while (range_filter.Flush() == io::PointsProcessor::FlushResult::kRestartStream);
  std::fclose(forwarded);
  std::fclose(grid_out);
  // one pass, one image, every batch forwarded once, the last stage flushed once; both stages hold the same limits
  if (passes != 1 || images != 1 || sink.batches != count || sink.flushes != 1) return 3;
  double r1, r2, m1[2], m2[2];
  int32_t n1[2], n2[2];
  if (dliom_probability_grid_limits(grid.grid(), &r1, m1, n1) != DLIOM_OK || dliom_probability_grid_limits(ros_map.grid(), &r2, m2, n2) != DLIOM_OK)
    return 5;
  if (r1 != r2 || m1[0] != m2[0] || m1[1] != m2[1] || n1[0] != n2[0] || n1[1] != n2[1]) return 5;
  return 0;
}
