// A stand-alone driver of csrc/imu_lidar_init.cc for the host sanitizers: built together with that file under
// -fsanitize=address,undefined and run as a program of its own (tests/test_imu_lidar_init_host.py); no library is loaded.
// It walks every way through dliom_imu_static_initialization: a tilted mean, the nearly-opposite rule on each of its three
// axis choices, one sample, many samples, and every refusal; and through dliom_imu_lidar_initialization and
// dliom_imu_lidar_align_with_world: eight frames of a motion with a constant jerk (exact preintegrations, no rotation),
// frame 0 without a preintegration, six frames, a platform at rest, a singular system, and the refusals.  "ok" and exit
// status 0.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "dliom.h"

namespace {
int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++failures;
  }
}

bool is_rotation(const double R[9]) {
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double d = 0.0;
      for (int k = 0; k < 3; ++k) d += R[3 * k + a] * R[3 * k + b];
      if (std::fabs(d - (a == b ? 1.0 : 0.0)) > 1e-12) return false;
    }
  return true;
}
}  // namespace

int main() {
  double R[9], ba[3], bg[3], P[3], V[3];
  const double g = 9.80511;
  for (int n : {1, 7, 1600}) {
    std::vector<double> acc(3 * static_cast<size_t>(n)), gyr(3 * static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
      acc[3 * i] = 1.0 + 1e-3 * (i % 7);
      acc[3 * i + 1] = -2.0;
      acc[3 * i + 2] = 9.5;
      gyr[3 * i] = 1e-3;
      gyr[3 * i + 1] = -2e-3 * (i % 3);
      gyr[3 * i + 2] = 3e-3;
    }
    expect(dliom_imu_static_initialization(n, acc.data(), gyr.data(), g, R, ba, bg, P, V) == DLIOM_OK, "a tilted mean");
    expect(is_rotation(R) && P[0] == 0.0 && V[2] == 0.0 && std::fabs(bg[0] - 1e-3) < 1e-15,  // (a sum of n, not n * 1e-3)
           "a rotation, the zero state and the gyroscope mean");
  }
  const double opposite[3][3] = {{0.0, 0.0, -g}, {1e-9, 0.0, -g}, {0.0, -1e-9, -g}};
  for (const auto& a : opposite) {
    const double zero[3] = {0.0, 0.0, 0.0};
    expect(dliom_imu_static_initialization(1, a, zero, g, R, ba, bg, P, V) == DLIOM_OK && is_rotation(R), "nearly opposite");
    expect(std::fabs(R[8] + 1.0) < 1e-9, "half a turn: z goes to -z");
  }
  const double one[3] = {0.1, 0.2, 9.7}, nan3[3] = {0.1, std::numeric_limits<double>::quiet_NaN(), 9.7}, none[3] = {0.0, 0.0, 0.0};
  expect(dliom_imu_static_initialization(0, one, one, g, R, ba, bg, P, V) == DLIOM_ERR_INVALID_ARGUMENT, "n = 0");
  expect(dliom_imu_static_initialization(1, nullptr, one, g, R, ba, bg, P, V) == DLIOM_ERR_INVALID_ARGUMENT, "no samples");
  expect(dliom_imu_static_initialization(1, one, one, g, nullptr, ba, bg, P, V) == DLIOM_ERR_INVALID_ARGUMENT, "no output");
  expect(dliom_imu_static_initialization(1, nan3, one, g, R, ba, bg, P, V) == DLIOM_ERR_INVALID_ARGUMENT, "a NaN sample");
  expect(dliom_imu_static_initialization(1, one, nan3, g, R, ba, bg, P, V) == DLIOM_ERR_INVALID_ARGUMENT, "a NaN rate");
  expect(dliom_imu_static_initialization(1, none, one, g, R, ba, bg, P, V) == DLIOM_ERR_INVALID_ARGUMENT, "no direction");
  expect(dliom_imu_static_initialization(1, one, one, 0.0, R, ba, bg, P, V) == DLIOM_ERR_INVALID_ARGUMENT, "gravity 0");
  expect(dliom_imu_static_initialization(1, one, one, std::numeric_limits<double>::infinity(), R, ba, bg, P, V) ==
             DLIOM_ERR_INVALID_ARGUMENT, "gravity inf");
  {
    // p(t) = c t^3 in a world whose gravity term is G = (0, 0, g): delta_p = p_j - p_i - v_i dt + G dt^2 / 2,
    // delta_v = v_j - v_i + G dt; identity rotations, no lever arm
    const double c[3] = {2.0, -1.0, 0.5}, lb[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}, dt = 0.1;
    dliom_init_frame frames[8] = {};
    for (int k = 0; k < 8; ++k) {
      const double t0 = 0.1 * (k - 1), t1 = 0.1 * k;
      frames[k].pose[3] = 1.0;
      frames[k].has_preintegration = k > 0 ? 1 : 0;
      frames[k].sum_dt = dt;
      for (int a = 0; a < 3; ++a) {
        const double G = a == 2 ? g : 0.0;
        frames[k].pose[a] = c[a] * t1 * t1 * t1;
        frames[k].delta_p[a] = c[a] * (t1 * t1 * t1 - t0 * t0 * t0) - 3.0 * c[a] * t0 * t0 * dt + G * dt * dt / 2.0;
        frames[k].delta_v[a] = 3.0 * c[a] * (t1 * t1 - t0 * t0) + G * dt;
      }
    }
    double Vs[24], grav[3], Ps[24], Rs[72], Rw[9], excitation = 0.0;
    int outcome = -1;
    expect(dliom_imu_lidar_initialization(frames, 8, lb, g, Vs, grav, &outcome) == DLIOM_OK && outcome == DLIOM_INIT_OK, "8 frames");
    expect(std::fabs(grav[2] - g) < 1e-6 && std::fabs(grav[0]) < 1e-6 && std::fabs(Vs[21] - 3.0 * c[0] * 0.49) < 1e-6, "g and V_7");
    expect(dliom_imu_lidar_align_with_world(frames, 8, lb, g, Ps, Rs, Vs, grav, Rw, &excitation, &outcome) == DLIOM_OK &&
               outcome == DLIOM_INIT_OK && excitation > 0.25 && is_rotation(Rw) && is_rotation(Rs + 63),
           "aligned with the world");
    expect(dliom_imu_lidar_align_with_world(frames, 6, lb, g, Ps, Rs, Vs, grav, Rw, &excitation, &outcome) == DLIOM_OK &&
               outcome == DLIOM_INIT_TOO_FEW_FRAMES, "six frames");
    dliom_init_frame still[8];
    for (int k = 0; k < 8; ++k) {
      still[k] = frames[0];
      still[k].has_preintegration = 1;
      for (int a = 0; a < 3; ++a) {
        still[k].delta_p[a] = a == 2 ? g * dt * dt / 2.0 : 0.0;
        still[k].delta_v[a] = a == 2 ? g * dt : 0.0;
      }
    }
    expect(dliom_imu_lidar_align_with_world(still, 8, lb, g, Ps, Rs, Vs, grav, Rw, &excitation, &outcome) == DLIOM_OK &&
               outcome == DLIOM_INIT_NO_EXCITATION, "at rest");
    still[4].has_preintegration = 0;  // frame 4's velocity is tied to nothing on one side: the system may be singular or not
    expect(dliom_imu_lidar_initialization(still, 8, lb, g, Vs, grav, &outcome) == DLIOM_OK, "a pair skipped");
    for (int k = 1; k < 8; ++k) still[k].has_preintegration = 0;
    expect(dliom_imu_lidar_initialization(still, 8, lb, g, Vs, grav, &outcome) == DLIOM_OK && outcome == DLIOM_INIT_SINGULAR, "no pair");
    expect(dliom_imu_lidar_initialization(nullptr, 8, lb, g, Vs, grav, &outcome) == DLIOM_ERR_INVALID_ARGUMENT, "no frames");
    expect(dliom_imu_lidar_initialization(frames, 65, lb, g, Vs, grav, &outcome) == DLIOM_ERR_INVALID_ARGUMENT, "too many frames");
    expect(dliom_imu_lidar_align_with_world(frames, 1, lb, g, Ps, Rs, Vs, grav, Rw, &excitation, &outcome) == DLIOM_ERR_INVALID_ARGUMENT,
           "one frame");
    frames[3].sum_dt = 0.0;
    expect(dliom_imu_lidar_initialization(frames, 8, lb, g, Vs, grav, &outcome) == DLIOM_ERR_INVALID_ARGUMENT, "sum_dt 0");
  }
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
