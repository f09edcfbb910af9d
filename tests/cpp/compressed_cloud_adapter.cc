// sensor::CompressedPointCloud and mapping::ToProto / FromProto(TrajectoryNode::Data) through dliom_cartographer.h
// (tests/test_gpu_compressed_cloud.py compares the bytes with the Python side).
//
//   compressed_cloud_adapter in.bin out.bin
//     in.bin:  int32 nodes | per node: int64 time | double gravity wxyz[4] | double pose7[7] |
//              int32 n_high | float xyz[3 n_high] | int32 n_low | float xyz[3 n_low] | int32 n_hist | float hist[n_hist]
//     out.bin: per node six records (int64 bytes | the bytes): ToProto(node), the batched ToProto's entry for it,
//              CompressedPointCloud(device cloud).ToProto(), CompressedPointCloud(sensor::PointCloud).ToProto(),
//              the floats of Decompress(), ToProto(FromProto(ToProto(node)))
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "dliom_cartographer.h"

namespace {

template <class T>
T read_one(std::FILE* f) {
  T v;
  if (std::fread(&v, sizeof v, 1, f) != 1) std::abort();
  return v;
}
template <class T>
std::vector<T> read_many(std::FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n > 0 && std::fread(v.data(), sizeof(T), n, f) != n) std::abort();
  return v;
}
void write_record(std::FILE* f, const void* p, size_t n) {
  const int64_t size = static_cast<int64_t>(n);
  std::fwrite(&size, sizeof size, 1, f);
  if (n > 0) std::fwrite(p, 1, n, f);
}
void write_record(std::FILE* f, const std::string& s) { write_record(f, s.data(), s.size()); }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (in == nullptr || out == nullptr) return 2;
  dliom::Context context(0);
  const int count = read_one<int32_t>(in);
  std::vector<dliom::mapping::TrajectoryNode::Data> nodes(static_cast<size_t>(count));
  std::vector<dliom::sensor::PointCloud> high(static_cast<size_t>(count));
  for (int i = 0; i < count; ++i) {
    dliom::mapping::TrajectoryNode::Data& d = nodes[i];
    d.time = read_one<int64_t>(in);
    const std::vector<double> g = read_many<double>(in, 4), pose = read_many<double>(in, 7);
    d.gravity_alignment = dliom::transform::Quaterniond{{g[0], g[1], g[2], g[3]}};
    d.local_pose = dliom::transform::Rigid3d::FromArray(pose.data());
    high[i] = read_many<dliom::sensor::Vector3f>(in, static_cast<size_t>(read_one<int32_t>(in)));
    const dliom::sensor::PointCloud low = read_many<dliom::sensor::Vector3f>(in, static_cast<size_t>(read_one<int32_t>(in)));
    d.high_resolution_point_cloud = std::make_shared<dliom::io::internal::DeviceCloud>(&context, high[i]);
    d.low_resolution_point_cloud = std::make_shared<dliom::io::internal::DeviceCloud>(&context, low);
    d.rotational_scan_matcher_histogram = read_many<float>(in, static_cast<size_t>(read_one<int32_t>(in)));
  }
  std::vector<const dliom::mapping::TrajectoryNode::Data*> span;
  for (const auto& d : nodes) span.push_back(&d);
  const std::vector<std::string> batched = dliom::mapping::ToProto(&context, span.data(), span.size());
  for (int i = 0; i < count; ++i) {
    const std::string single = dliom::mapping::ToProto(&context, nodes[i]);
    write_record(out, single);
    write_record(out, batched[i]);
    const dliom::sensor::CompressedPointCloud from_device(&context, nodes[i].high_resolution_point_cloud->cloud);
    const dliom::sensor::CompressedPointCloud from_host(&context, high[i]);
    if (!(from_device == from_host) || from_device.size() != high[i].size() || from_device.empty() != high[i].empty()) return 3;
    write_record(out, from_device.ToProto());
    write_record(out, from_host.ToProto());
    if (!(dliom::sensor::CompressedPointCloud::FromProto(from_host.ToProto()) == from_host)) return 4;
    const dliom::sensor::PointCloud points = from_device.Decompress(&context);
    write_record(out, points.data(), 12 * points.size());
    write_record(out, dliom::mapping::ToProto(&context, dliom::mapping::FromProto(&context, single)));
  }
  std::fclose(out);
  std::fclose(in);
  return 0;
}
