// The timed part of tools/approx_voxel_bench.py: one pair of raw scans (packed float xyz files), on one device.
//   filter: dliom_cloud_approximate_voxel_filter on the previous scan as it lies in HBM, against what the adapter did before
//           it -- download the cloud, registration::ApproximateVoxelGrid on one host thread, upload the result -- checked equal
//   pair:   registration::NdtScanMatcher (the previous scan's cells kept, the new scan filtered on the device) against
//           registration::MatchByNDT on the same host scans (both filtered on the host, a target a pair), checked equal; and
//           the matcher's stages one by one through the C calls
// Every timed call ends with dliom_ctx_synchronize.  Prints one JSON object.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dliom_cartographer.h"

namespace {
namespace registration = dliom::registration;
using dliom::sensor::PointCloud;
using dliom::sensor::Vector3f;
using Clock = std::chrono::steady_clock;

double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

bool read_cloud(const char* path, PointCloud* cloud) {
  std::FILE* in = std::fopen(path, "rb");
  if (in == nullptr) return false;
  float xyz[3];
  while (std::fread(xyz, sizeof(float), 3, in) == 3) cloud->push_back(Vector3f(xyz[0], xyz[1], xyz[2]));
  std::fclose(in);
  return true;
}

dliom_cloud* upload(dliom::Context* context, const PointCloud& cloud) {
  dliom_cloud* out = nullptr;
  dliom::Check(dliom_cloud_create(context->get(), cloud.empty() ? nullptr : &cloud[0].x, static_cast<int64_t>(cloud.size()), &out),
               "dliom_cloud_create");
  return out;
}

PointCloud download(const dliom_cloud* cloud) {
  int64_t n = 0;
  dliom::Check(dliom_cloud_size(cloud, &n), "dliom_cloud_size");
  PointCloud out(static_cast<size_t>(n));
  if (n > 0) dliom::Check(dliom_cloud_download(cloud, &out[0].x), "dliom_cloud_download");
  return out;
}

void print_list(const char* name, const std::vector<double>& v, const char* tail) {
  std::printf("\"%s\": [", name);
  for (size_t k = 0; k < v.size(); ++k) std::printf("%s%.4f", k == 0 ? "" : ", ", v[k]);
  std::printf("]%s", tail);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: approx_voxel_bench PREVIOUS.bin CURRENT.bin WARMUP REPEATS\n");
    return 2;
  }
  PointCloud previous, current;
  if (!read_cloud(argv[1], &previous) || !read_cloud(argv[2], &current)) return 2;
  const int warmup = std::atoi(argv[3]), repeats = std::atoi(argv[4]);
  const float leaf = 0.2f;
  dliom::Context context(0);
  dliom_ctx* const ctx = context.get();
  dliom_cloud* const d_previous = upload(&context, previous);
  dliom_cloud* const d_current = upload(&context, current);

  // ---- the filter
  std::vector<double> device_ms, host_ms, host_filter_only_ms;
  bool filter_equal = true;
  size_t filtered_points = 0;
  for (int r = 0; r < warmup + repeats; ++r) {
    auto t = Clock::now();
    dliom_cloud* filtered = nullptr;
    dliom::Check(dliom_cloud_approximate_voxel_filter(ctx, d_previous, leaf, &filtered), "dliom_cloud_approximate_voxel_filter");
    dliom::Check(dliom_ctx_synchronize(ctx), "dliom_ctx_synchronize");
    const double device = ms_since(t);
    t = Clock::now();
    const PointCloud down = download(d_previous);
    PointCloud host_filtered;
    registration::ApproximateVoxelGrid filter;
    filter.setLeafSize(leaf, leaf, leaf);
    filter.setInputCloud(&down);
    const auto t_loop = Clock::now();
    filter.filter(&host_filtered);
    const double loop = ms_since(t_loop);
    dliom_cloud* up = upload(&context, host_filtered);
    dliom::Check(dliom_ctx_synchronize(ctx), "dliom_ctx_synchronize");
    const double host = ms_since(t);
    const PointCloud got = download(filtered);
    filter_equal = filter_equal && got.size() == host_filtered.size() &&
                   (got.empty() || std::memcmp(&got[0].x, &host_filtered[0].x, sizeof(Vector3f) * got.size()) == 0);
    filtered_points = got.size();
    dliom_cloud_destroy(up);
    dliom_cloud_destroy(filtered);
    if (r >= warmup) {
      device_ms.push_back(device);
      host_ms.push_back(host);
      host_filter_only_ms.push_back(loop);
    }
  }

  // ---- a pair
  std::vector<double> matcher_ms, parent_ms, stage_filter_ms, stage_align_ms, stage_cells_ms;
  bool pair_equal = true;
  dliom_ndt_options options;
  dliom::Check(dliom_ndt_default_options(&options), "dliom_ndt_default_options");
  const registration::Matrix4f guess = registration::Matrix4f::Identity();
  double guess16[16];
  for (int k = 0; k < 16; ++k) guess16[k] = static_cast<double>(guess.m[k]);
  for (int r = 0; r < warmup + repeats; ++r) {
    float rotation[2][9], translation[2][3];
    auto t = Clock::now();
    registration::MatchByNDT(&context, previous, current, guess, rotation[0], translation[0]);
    dliom::Check(dliom_ctx_synchronize(ctx), "dliom_ctx_synchronize");
    const double parent = ms_since(t);
    registration::NdtScanMatcher matcher(&context, leaf);
    matcher.Match(d_previous, guess, rotation[1], translation[1]);  // the pair before this one left its cells
    t = Clock::now();
    matcher.Match(d_current, guess, rotation[1], translation[1]);
    dliom::Check(dliom_ctx_synchronize(ctx), "dliom_ctx_synchronize");
    const double kept = ms_since(t);
    pair_equal = pair_equal && std::memcmp(rotation[0], rotation[1], sizeof(rotation[0])) == 0 &&
                 std::memcmp(translation[0], translation[1], sizeof(translation[0])) == 0;
    // the matcher's stages, one C call each
    dliom_cloud *f_previous = nullptr, *f_current = nullptr;
    dliom_ndt_target *cells_previous = nullptr, *cells_current = nullptr;
    dliom::Check(dliom_cloud_approximate_voxel_filter(ctx, d_previous, leaf, &f_previous), "filter");
    dliom::Check(dliom_ndt_target_create(ctx, f_previous, &options, &cells_previous), "cells");
    t = Clock::now();
    dliom::Check(dliom_cloud_approximate_voxel_filter(ctx, d_current, leaf, &f_current), "filter");
    dliom::Check(dliom_ctx_synchronize(ctx), "dliom_ctx_synchronize");
    const double s_filter = ms_since(t);
    t = Clock::now();
    dliom_ndt_result result;
    dliom::Check(dliom_ndt_align(cells_previous, f_current, guess16, &options, nullptr, &result, nullptr), "align");
    const double s_align = ms_since(t);
    t = Clock::now();
    dliom::Check(dliom_ndt_target_create(ctx, f_current, &options, &cells_current), "cells");
    const double s_cells = ms_since(t);
    dliom_ndt_target_destroy(cells_previous);
    dliom_ndt_target_destroy(cells_current);
    dliom_cloud_destroy(f_previous);
    dliom_cloud_destroy(f_current);
    if (r >= warmup) {
      parent_ms.push_back(parent);
      matcher_ms.push_back(kept);
      stage_filter_ms.push_back(s_filter);
      stage_align_ms.push_back(s_align);
      stage_cells_ms.push_back(s_cells);
    }
  }
  dliom_cloud_destroy(d_previous);
  dliom_cloud_destroy(d_current);
  std::printf("{\"points\": %zu, \"filtered_points\": %zu, \"filter_equal\": %s, \"pair_equal\": %s, ", previous.size(), filtered_points,
              filter_equal ? "true" : "false", pair_equal ? "true" : "false");
  print_list("device_filter_ms", device_ms, ", ");
  print_list("host_download_filter_upload_ms", host_ms, ", ");
  print_list("host_filter_loop_ms", host_filter_only_ms, ", ");
  print_list("matcher_pair_ms", matcher_ms, ", ");
  print_list("match_by_ndt_pair_ms", parent_ms, ", ");
  print_list("stage_filter_ms", stage_filter_ms, ", ");
  print_list("stage_align_ms", stage_align_ms, ", ");
  print_list("stage_cells_ms", stage_cells_ms, "}\n");
  return filter_equal && pair_equal ? 0 : 1;
}
