// The adapter's host pieces of MatchByNDT (dliom_cartographer.h) beside the library's device calls, on a real device.
//
//   approx_voxel_adapter filter LEAF IN.bin HOST.bin DEVICE.bin
//       packed float xyz in; the cloud through registration::ApproximateVoxelGrid (the host loop) and through
//       dliom_cloud_approximate_voxel_filter (uploaded, filtered, downloaded): tests/test_gpu_approx_voxel.py wants the two
//       files equal
//   approx_voxel_adapter match GUESSES.bin OUT.bin SCAN0.bin SCAN1.bin ...
//       registration::MatchByNDT on every pair (scan k-1, scan k) from guess k-1 (16 floats each, row-major), and the same
//       stream through registration::NdtScanMatcher; OUT.bin gets 24 floats a pair, the rotation's nine and the
//       translation's three of the first, then of the second (tests/test_gpu_ndt_scan_matcher.py); exit status 3 if the
//       matcher's first scan returned a result
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "dliom_cartographer.h"

namespace {
namespace registration = dliom::registration;
using dliom::sensor::PointCloud;
using dliom::sensor::Vector3f;

bool read_cloud(const char* path, PointCloud* cloud) {
  std::FILE* in = std::fopen(path, "rb");
  if (in == nullptr) return false;
  float xyz[3];
  while (std::fread(xyz, sizeof(float), 3, in) == 3) cloud->push_back(Vector3f(xyz[0], xyz[1], xyz[2]));
  std::fclose(in);
  return true;
}

bool write_floats(const char* path, const float* values, size_t count) {
  std::FILE* file = std::fopen(path, "wb");
  if (file == nullptr) return false;
  const size_t written = count == 0 ? 0 : std::fwrite(values, sizeof(float), count, file);
  std::fclose(file);
  return written == count;
}

int filter_file(const char* leaf, const char* in_path, const char* host_path, const char* device_path) {
  PointCloud cloud, host;
  if (!read_cloud(in_path, &cloud)) return 2;
  const float edge = static_cast<float>(std::atof(leaf));
  registration::ApproximateVoxelGrid filter;
  filter.setLeafSize(edge, edge, edge);
  filter.setInputCloud(&cloud);
  filter.filter(&host);
  if (!write_floats(host_path, host.empty() ? nullptr : &host[0].x, 3 * host.size())) return 2;
  dliom::Context context(0);
  dliom_cloud *uploaded = nullptr, *filtered = nullptr;
  dliom::Check(dliom_cloud_create(context.get(), cloud.empty() ? nullptr : &cloud[0].x, static_cast<int64_t>(cloud.size()), &uploaded),
               "dliom_cloud_create");
  dliom::Check(dliom_cloud_approximate_voxel_filter(context.get(), uploaded, edge, &filtered), "dliom_cloud_approximate_voxel_filter");
  int64_t n = 0;
  dliom::Check(dliom_cloud_size(filtered, &n), "dliom_cloud_size");
  std::vector<float> device(3 * static_cast<size_t>(n));
  if (n > 0) dliom::Check(dliom_cloud_download(filtered, device.data()), "dliom_cloud_download");
  dliom_cloud_destroy(filtered);
  dliom_cloud_destroy(uploaded);
  return write_floats(device_path, device.data(), device.size()) ? 0 : 2;
}

int match_files(const char* guess_path, const char* out_path, int scans, char** scan_paths) {
  std::vector<PointCloud> clouds(scans);
  for (int k = 0; k < scans; ++k)
    if (!read_cloud(scan_paths[k], &clouds[k])) return 2;
  std::vector<float> guesses(16 * static_cast<size_t>(scans - 1));
  std::FILE* in = std::fopen(guess_path, "rb");
  if (in == nullptr) return 2;
  const size_t got = std::fread(guesses.data(), sizeof(float), guesses.size(), in);
  std::fclose(in);
  if (got != guesses.size()) return 2;
  dliom::Context context(0);
  registration::NdtScanMatcher matcher(&context);
  std::vector<float> out;
  bool first_is_quiet = false;
  for (int k = 0; k < scans; ++k) {
    registration::Matrix4f guess;
    if (k > 0)
      for (int e = 0; e < 16; ++e) guess.m[e] = guesses[16 * static_cast<size_t>(k - 1) + e];
    float rotation[9], translation[3];
    if (k > 0) {
      registration::MatchByNDT(&context, clouds[k - 1], clouds[k], guess, rotation, translation);
      out.insert(out.end(), rotation, rotation + 9);
      out.insert(out.end(), translation, translation + 3);
    }
    dliom_cloud* scan = nullptr;
    dliom::Check(dliom_cloud_create(context.get(), &clouds[k][0].x, static_cast<int64_t>(clouds[k].size()), &scan), "dliom_cloud_create");
    const bool matched = matcher.Match(scan, guess, rotation, translation);
    dliom_cloud_destroy(scan);
    if (k == 0) first_is_quiet = !matched;
    if (matched) {
      out.insert(out.end(), rotation, rotation + 9);
      out.insert(out.end(), translation, translation + 3);
    }
  }
  if (!first_is_quiet || out.size() != 24 * static_cast<size_t>(scans - 1)) return 3;
  return write_floats(out_path, out.data(), out.size()) ? 0 : 2;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 6 && std::string(argv[1]) == "filter") return filter_file(argv[2], argv[3], argv[4], argv[5]);
  if (argc >= 6 && std::string(argv[1]) == "match") return match_files(argv[2], argv[3], argc - 4, argv + 4);
  std::fprintf(stderr, "usage: approx_voxel_adapter filter LEAF IN HOST DEVICE | match GUESSES OUT SCAN0 SCAN1 ...\n");
  return 2;
}
