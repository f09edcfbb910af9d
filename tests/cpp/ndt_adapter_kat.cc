// The host pieces of dliom::registration's NDT adapter (dliom_cartographer.h) that need no device.  The
// NormalDistributionsTransform class and MatchByNDT are instantiated only to prove that they compile; nothing of them runs
// (no context is created).
//
//   ndt_adapter_kat                            a hand-made stream through ApproximateVoxelGrid; "ok" and exit status 0
//   ndt_adapter_kat filter LEAF IN.bin OUT.bin packed float xyz in, the filtered cloud out (tests/test_ndt_host.py compares
//                                              it with the Python model of the header's statement)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dliom_cartographer.h"

namespace {
namespace registration = dliom::registration;
using dliom::sensor::PointCloud;
using dliom::sensor::Vector3f;

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++failures;
  }
}

// never called: the adapter's members must compile under -Wall -Werror
void instantiate(dliom::Context* context, const PointCloud* cloud) {
  auto ndt = registration::NormalDistributionsTransform::GroundTruthNdt(context);
  ndt->setTransformationEpsilon(0.01);
  ndt->setStepSize(0.1);
  ndt->setResolution(1.0f);
  ndt->setMaximumIterations(35);
  ndt->setOulierRatio(0.55);
  ndt->setStepMode(DLIOM_NDT_STEP_MORE_THUENTE);
  ndt->setInputSource(cloud);
  ndt->setInputTarget(cloud);
  PointCloud output;
  ndt->align(&output, registration::Matrix4f::Identity());
  (void)ndt->hasConverged();
  (void)ndt->getFitnessScore();
  (void)ndt->getTransformationProbability();
  (void)ndt->getFinalNumIteration();
  (void)ndt->getFinalTransformation();
  (void)ndt->result();
  float rotation[9], translation[3];
  registration::MatchByNDT(context, *cloud, *cloud, registration::Matrix4f::Identity(), rotation, translation);
}

int filter_file(const char* leaf, const char* in_path, const char* out_path) {
  std::FILE* in = std::fopen(in_path, "rb");
  if (in == nullptr) return 2;
  PointCloud cloud, out;
  float xyz[3];
  while (std::fread(xyz, sizeof(float), 3, in) == 3) cloud.push_back(Vector3f(xyz[0], xyz[1], xyz[2]));
  std::fclose(in);
  registration::ApproximateVoxelGrid filter;
  const float edge = static_cast<float>(std::atof(leaf));
  filter.setLeafSize(edge, edge, edge);
  filter.setInputCloud(&cloud);
  filter.filter(&out);
  std::FILE* file = std::fopen(out_path, "wb");
  if (file == nullptr) return 2;
  const size_t written = out.empty() ? 0 : std::fwrite(&out[0].x, sizeof(Vector3f), out.size(), file);
  std::fclose(file);
  return written == out.size() ? 0 : 2;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc > 1000) instantiate(nullptr, nullptr);
  if (argc == 5 && std::string(argv[1]) == "filter") return filter_file(argv[2], argv[3], argv[4]);
  // leaf 1: voxels (0,0,0) and (512,0,0) share slot 0 (512 * 7171 is a multiple of 512), voxel (1,0,0) has slot 7171 & 511 = 3
  PointCloud cloud = {Vector3f(0.25f, 0.5f, 0.5f), Vector3f(0.75f, 0.5f, 0.25f), Vector3f(1.5f, 0.5f, 0.5f),
                      Vector3f(512.5f, 0.5f, 0.5f), Vector3f(0.5f, 0.25f, 0.5f)};
  PointCloud out;
  registration::ApproximateVoxelGrid filter;
  filter.setLeafSize(1.f, 1.f, 1.f);
  filter.setInputCloud(&cloud);
  filter.filter(&out);
  expect(out.size() == 4, "two evictions of slot 0, then slots 0 and 3");
  if (out.size() == 4) {
    expect(out[0].x == 0.5f && out[0].y == 0.5f && out[0].z == 0.375f, "the first voxel's centroid leaves when (512,0,0) arrives");
    expect(out[1].x == 512.5f, "(512,0,0) leaves when (0,0,0) comes back");
    expect(out[2].x == 0.5f && out[2].y == 0.25f, "slot 0 at the end: the returned voxel, one point");
    expect(out[3].x == 1.5f, "slot 3 after slot 0");
  }
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
