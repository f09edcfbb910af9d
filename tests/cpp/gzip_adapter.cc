// The gzip adapters of d-liom_amd/cpp/dliom_cartographer.h next to the methods they extend:
//   Submap3D::ToResponseProto(pose, dliom::kGzipped) against ToResponseProto(pose), on two grids read from serialized
//   mapping::proto::HybridGrid files; NodeCloudCache::SerializeRangeDataFramed against SerializeRangeData, on scans made
//   here; common::FastGzipString.  Sizes and poses are compared here (exit 3 on a difference); the bytes go to <out> as
//   blobs (int64 size, bytes), where tests/test_gpu_gzip_adapter.py inflates the gzipped ones with zlib and compares:
//     per texture: cells, gzipped cells;  int64 records;  per record: message, framed record;  a string, FastGzipString of it
//   gzip_adapter hi.pb lo.pb out.bin
//   g++ -std=c++17 gzip_adapter.cc -L../../d-liom_amd -ldliom
#include <cstdio>
#include <string>
#include <vector>

#include "../../d-liom_amd/cpp/dliom_cartographer.h"

using namespace dliom;

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> b;
  FILE* f = std::fopen(path, "rb");
  if (f == nullptr) return b;
  uint8_t chunk[65536];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) b.insert(b.end(), chunk, chunk + got);
  std::fclose(f);
  return b;
}

static void write_blob(FILE* f, const void* data, size_t size) {
  const int64_t n = static_cast<int64_t>(size);
  std::fwrite(&n, 8, 1, f);
  if (size > 0) std::fwrite(data, 1, size, f);
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s hi.pb lo.pb out.bin\n", argv[0]);
    return 2;
  }
  Context context(0);
  dliom_grid* grids[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; ++k) {
    const std::vector<uint8_t> b = read_file(argv[1 + k]);
    Check(dliom_grid_from_proto(context.get(), b.data(), static_cast<int64_t>(b.size()), &grids[k]), "dliom_grid_from_proto");
  }
  FILE* out = std::fopen(argv[3], "wb");
  if (out == nullptr) return 2;

  const double pose[7] = {1.25, -3.5, 0.4, 0.9393727128473789, 0.0, 0.0, 0.3428978074554514};
  const transform::Rigid3d global_pose = transform::Rigid3d::FromArray(pose);
  const mapping::Submap3D submap(transform::Rigid3d(), 5, true, grids[0], grids[1]);
  const mapping::SubmapQueryResponse plain = submap.ToResponseProto(global_pose);
  const mapping::SubmapQueryResponse gzipped = submap.ToResponseProto(global_pose, kGzipped);
  if (plain.submap_version != gzipped.submap_version || plain.textures.size() != 2 || gzipped.textures.size() != 2) return 3;
  for (size_t k = 0; k < 2; ++k) {
    const mapping::SubmapTexture &a = plain.textures[k], &b = gzipped.textures[k];
    if (a.width != b.width || a.height != b.height || a.resolution != b.resolution || a.slice_pose.ToArray() != b.slice_pose.ToArray()) return 3;
    write_blob(out, a.cells.data(), a.cells.size());
    write_blob(out, b.cells.data(), b.cells.size());
  }

  cartographer_ros::NodeCloudCache cache(&context);
  const int sizes[5][2] = {{300, 9}, {0, 0}, {5000, 0}, {40, 40}, {1, 0}};
  for (int i = 0; i < 5; ++i) {
    sensor::RangeData range_data;
    range_data.origin = sensor::Vector3f(0.5f * i, -1.f, 0.25f);
    for (int k = 0; k < sizes[i][0]; ++k) range_data.returns.push_back(sensor::Vector3f(0.05f * (k % 97), 0.1f * (k % 13) - 0.6f, k % 5 == 0 ? 0.f : 0.01f * k));
    for (int k = 0; k < sizes[i][1]; ++k) range_data.misses.push_back(sensor::Vector3f(-0.5f * k, 2.f, 0.125f * i));
    const double local[7] = {0.1 * i, 0.2, -0.3, 1.0, 0.0, 0.0, 0.0};
    cache.OnLocalSlamResult(i % 2, 1000 + i, transform::Rigid3d::FromArray(local), range_data);
  }
  std::vector<std::vector<uint8_t>> messages, records;
  cache.SerializeRangeData([&](const uint8_t* data, size_t size) { messages.emplace_back(data, data + size); });
  cache.SerializeRangeDataFramed([&](const uint8_t* data, size_t size) { records.emplace_back(data, data + size); });
  if (messages.size() != 5 || records.size() != 5) return 3;
  const int64_t count = 5;
  std::fwrite(&count, 8, 1, out);
  for (size_t i = 0; i < 5; ++i) {
    write_blob(out, messages[i].data(), messages[i].size());
    write_blob(out, records[i].data(), records[i].size());
  }

  std::string header = "a SerializationHeader is a few bytes: format_version 2 ";
  header += header + header;
  std::string compressed;
  common::FastGzipString(header, &compressed);
  write_blob(out, header.data(), header.size());
  write_blob(out, compressed.data(), compressed.size());
  std::fclose(out);
  for (dliom_grid* g : grids) dliom_grid_destroy(g);
  std::printf("GZIP ADAPTER DONE textures 2 records %zu\n", records.size());
  return 0;
}
