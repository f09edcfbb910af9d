// The io:: adapters of dliom_cartographer.h driven the way the reference's assets writer drives a pipeline
// (io/points_processor_pipeline_builder and assets_writer's do { ... } while (Flush() == kRestartStream)): a stream of
// batches through MinMaxRangeFiteringPointsProcessor -> OutlierRemovingPointsProcessor -> a collecting sink, restarted
// until Flush() reports kFinished.  Every point carries intensity = its index in the batch and color = (i, 2i, 3i), so
// that the Python side (tests/test_gpu_outlier.py) can check that they were filtered with the points.
//
//   outlier_adapter batches.bin out.bin voxel_size min_range max_range
//     batches.bin: int32 count; per batch float origin[3], int32 n, n * 3 floats
//     out.bin: per batch that reached the sink: int32 n, n * 3 floats, n intensities, n * 3 color floats
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "dliom_cartographer.h"

namespace io = dliom::io;

class Sink : public io::PointsProcessor {
 public:
  explicit Sink(std::FILE* out) : out_(out) {}
  void Process(std::unique_ptr<io::PointsBatch> batch) override {
    const int32_t n = static_cast<int32_t>(batch->points.size());
    if (batch->intensities.size() != batch->points.size() || batch->colors.size() != batch->points.size()) std::abort();
    std::fwrite(&n, 4, 1, out_);
    std::fwrite(batch->points.data(), 12, batch->points.size(), out_);
    std::fwrite(batch->intensities.data(), 4, batch->intensities.size(), out_);
    std::fwrite(batch->colors.data(), 12, batch->colors.size(), out_);
  }
  FlushResult Flush() override { return FlushResult::kFinished; }

 private:
  std::FILE* out_;
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
    if (n > 0 && std::fread(&b.points[0].x, 12, b.points.size(), in) != b.points.size()) return 2;
    for (int32_t i = 0; i < n; ++i) {
      b.intensities.push_back(static_cast<float>(i));
      b.colors.push_back(io::FloatColor{static_cast<float>(i), static_cast<float>(2 * i), static_cast<float>(3 * i)});
    }
  }
  dliom::Context context(0);
  Sink sink(out);
  io::OutlierRemovingPointsProcessor remover(std::atof(argv[3]), &sink, &context);
  io::MinMaxRangeFiteringPointsProcessor range_filter(std::atof(argv[4]), std::atof(argv[5]), &remover, &context);
  int restarts = 0;
  do {
    for (const io::PointsBatch& b : batches) range_filter.Process(std::make_unique<io::PointsBatch>(b));
    ++restarts;
  } while (range_filter.Flush() == io::PointsProcessor::FlushResult::kRestartStream);
  std::fclose(out);
  std::fclose(in);
  if (restarts != 3) return 3;  // kRestartStream twice, then kFinished
  return 0;
}
