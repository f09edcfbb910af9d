// LocalTrajectoryBuilder3D's initialisation modes (d-liom_amd/cpp/dliom_cartographer.h) fed from the first message, as
// cartographer feeds the reference: AddImuData at 200 Hz, AddRangeData at 10 Hz.  Input: a binary file written by
// tests/test_gpu_ltb3d_initialisation.py; output, a scan:
//   SCAN s result R frames N failures M initialised I       what AddRangeData returned and the initialisation's bookkeeping
//   STATE s <16 numbers>                                     once, after the scan that initialised: the state handed to
//                                                            InitializeIMU (pose7, velocity3, bias6), %.17g
// mode: 0 the default (SetInitialState after scan `set_state_after`, -1: never), 1 static, 2 NDT
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dliom_cartographer.h"

using namespace dliom;

static bool read_all(FILE* f, void* p, size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) return 2;
  int32_t header[8];  // num_scans, points_per_scan, imu_per_scan, mode, frames_dynamic, frames_static, set_state_after, 0
  double numbers[5];  // acc_noise, gyr_noise, acc_bias_noise, gyr_bias_noise, gravity
  if (!read_all(f, header, sizeof header)) return 2;
  Context context(0);
  mapping::LocalTrajectoryBuilderOptions3D options;
  std::memset(&options.front_end, 0, sizeof options.front_end);
  if (!read_all(f, &options.front_end, sizeof options.front_end) || !read_all(f, numbers, sizeof numbers)) return 2;
  options.imu.acc_noise = numbers[0];
  options.imu.gyr_noise = numbers[1];
  options.imu.acc_bias_noise = numbers[2];
  options.imu.gyr_bias_noise = numbers[3];
  options.imu.gravity = numbers[4];
  options.internal_initialization = header[3] != 0;
  options.enable_ndt_initialization = header[3] == 2;
  options.frames_for_dynamic_initialization = header[4];
  options.frames_for_static_initialization = header[5];
  mapping::LocalTrajectoryBuilder3D builder(&context, options, {"lidar"});
  int64_t t = 0;
  bool reported = false;
  for (int s = 0; s < header[0]; ++s) {
    std::vector<double> imu(static_cast<size_t>(header[2]) * 7);  // dt, acc3, gyr3
    if (!read_all(f, imu.data(), imu.size() * 8)) return 2;
    for (int k = 0; k < header[2]; ++k) {
      t += static_cast<int64_t>(imu[7 * k] * 1e7 + 0.5);
      sensor::ImuData d;
      d.time = t;
      std::memcpy(d.linear_acceleration, &imu[7 * k + 1], 24);
      std::memcpy(d.angular_velocity, &imu[7 * k + 4], 24);
      builder.AddImuData(d);
    }
    sensor::TimedPointCloudData cloud;
    cloud.time = t;
    cloud.origin = sensor::Vector3f{0.f, 0.f, 0.f};
    cloud.ranges.resize(static_cast<size_t>(header[1]));
    if (!read_all(f, cloud.ranges.data(), cloud.ranges.size() * 16)) return 2;
    const auto result = builder.AddRangeData("lidar", cloud);
    double state[16];
    const bool initialised = builder.InitialState(state);
    std::printf("SCAN %d result %d frames %d failures %lld initialised %d\n", s, result != nullptr ? 1 : 0, builder.initialization_frames(),
                static_cast<long long>(builder.initialization_failures()), initialised ? 1 : 0);
    if (initialised && !reported) {
      std::printf("STATE %d", s);
      for (double v : state) std::printf(" %.17g", v);
      std::printf("\n");
      reported = true;
    }
    if (header[3] == 0 && s == header[6]) {
      const double bias[6] = {0., 0., 0., 0., 0., 0.};
      builder.SetInitialState(transform::Rigid3d(), transform::Vector3d{{0., 0., 0.}}, bias);
    }
  }
  std::fclose(f);
  std::printf("LTB3D INIT ADAPTER DONE\n");
  return 0;
}
