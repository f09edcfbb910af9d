// The IMU-LiDAR initialisation's arithmetic on the host (dliom.h "IMU-LiDAR initialisation"): no device is involved.
//   dliom_imu_static_initialization   LocalTrajectoryBuilder3D::InitializeStatic (local_trajectory_builder_3d.cc:203-229)
//   dliom_imu_lidar_initialization    Initializer::Initialization (initialization/imu_lidar_initializer.cc:50-229)
//   dliom_imu_lidar_align_with_world  LocalTrajectoryBuilder3D::AlignWithWorld (local_trajectory_builder_3d.cc:1010-1086)
// Every operation is a double operation of its own, in the order dliom.h writes (built with -ffp-contract=off).
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/dliom.h"
#include "sym_solve.h"

namespace {

struct V3 {
  double x, y, z;
};

inline bool finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
inline double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// v / sqrt(v . v); false for a vector without a direction
inline bool normalized(V3 v, V3* out) {
  const double z = dot(v, v);
  if (!(z > 0.0) || !std::isfinite(z)) return false;
  const double n = std::sqrt(z);
  *out = V3{v.x / n, v.y / n, v.z / n};
  return true;
}

// dliom.h, FROM TWO VECTORS: the quaternion (w, x, y, z) that turns a onto b
bool from_two_vectors(V3 a, V3 b, double q[4]) {
  V3 v0, v1;
  if (!normalized(a, &v0) || !normalized(b, &v1)) return false;
  const double c = dot(v1, v0);
  if (c < -1.0 + 1e-12) {
    // nearly opposite (parity unpinned against Eigen, which takes an SVD here): half a turn about v0 x e_k, e_k the
    // coordinate axis v0 has the least of (ties: the lowest k)
    const double m[3] = {std::fabs(v0.x), std::fabs(v0.y), std::fabs(v0.z)};
    int k = 0;
    if (m[1] < m[k]) k = 1;
    if (m[2] < m[k]) k = 2;
    V3 axis;
    if (!normalized(cross(v0, V3{k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0}), &axis)) return false;
    q[0] = 0.0;
    q[1] = axis.x;
    q[2] = axis.y;
    q[3] = axis.z;
    return true;
  }
  const V3 axis = cross(v0, v1);
  const double s = std::sqrt((1.0 + c) * 2.0);
  const double invs = 1.0 / s;
  q[0] = s * 0.5;
  q[1] = axis.x * invs;
  q[2] = axis.y * invs;
  q[3] = axis.z * invs;
  return true;
}

// Eigen's Quaternion::toRotationMatrix, row-major
void rotation_of(const double q[4], double R[9]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz);
  R[1] = txy - twz;
  R[2] = txz + twy;
  R[3] = txy + twz;
  R[4] = 1.0 - (txx + tzz);
  R[5] = tyz - twx;
  R[6] = txz - twy;
  R[7] = tyz + twx;
  R[8] = 1.0 - (txx + tyy);
}


inline V3 mul(const double R[9], V3 v) {
  return V3{(R[0] * v.x + R[1] * v.y) + R[2] * v.z, (R[3] * v.x + R[4] * v.y) + R[5] * v.z, (R[6] * v.x + R[7] * v.y) + R[8] * v.z};
}
inline void transpose(const double R[9], double T[9]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) T[3 * r + c] = R[3 * c + r];
}
inline void matmul(const double A[9], const double B[9], double C[9]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

// TangentBasis (imu_lidar_initializer.cc:36-48)
bool tangent_basis(V3 g0, V3* b, V3* c) {
  V3 a;
  if (!normalized(g0, &a)) return false;
  V3 tmp{0.0, 0.0, 1.0};
  if (a.x == tmp.x && a.y == tmp.y && a.z == tmp.z) tmp = V3{1.0, 0.0, 0.0};
  const double d = dot(a, tmp);
  if (!normalized(V3{tmp.x - a.x * d, tmp.y - a.y * d, tmp.z - a.z * d}, b)) return false;
  *c = cross(a, *b);
  return true;
}

struct Frames {
  const dliom_init_frame* f;
  int n;
  V3 tlb;
  std::vector<double> R;  // n x 9: the frames' rotation matrices
};

// One pair's 6 x (6 + G) block and right-hand side, squared and added into the (3 n + G)-column system: the scatter of
// ApproximateGravity (:105-115, G = 3, basis = identity, g0 = 0) and RefineGravity (:189-199, G = 2, basis = lxly)
template <int G>
void add_pair(const Frames& F, int i, const double basis[3][G], V3 g0, bool with_g0, std::vector<double>* A, std::vector<double>* b) {
  constexpr int W = 6 + G;
  const int n_state = 3 * F.n + G;
  const dliom_init_frame &fi = F.f[i], &fj = F.f[i + 1];
  const double dt = fj.sum_dt;
  const double *Ri = &F.R[9 * static_cast<size_t>(i)], *Rj = &F.R[9 * static_cast<size_t>(i + 1)];
  double RiT[9], RiTRj[9];
  transpose(Ri, RiT);
  matmul(RiT, Rj, RiTRj);
  double tA[6][W] = {}, tb[6];
  for (int r = 0; r < 3; ++r) {
    tA[r][r] = -dt;
    tA[3 + r][r] = -1.0;
    for (int c = 0; c < 3; ++c) tA[3 + r][3 + c] = RiTRj[3 * r + c];
    for (int c = 0; c < G; ++c) {
      const double col = (RiT[3 * r] * basis[0][c] + RiT[3 * r + 1] * basis[1][c]) + RiT[3 * r + 2] * basis[2][c];
      tA[r][6 + c] = col * (dt * dt / 2.0);
      tA[3 + r][6 + c] = col * dt;
    }
  }
  const V3 moved = mul(RiTRj, F.tlb);
  const V3 apart = mul(RiT, V3{fj.pose[0] - fi.pose[0], fj.pose[1] - fi.pose[1], fj.pose[2] - fi.pose[2]});
  const V3 pull = with_g0 ? mul(RiT, g0) : V3{0.0, 0.0, 0.0};
  const double dP[3] = {fj.delta_p[0], fj.delta_p[1], fj.delta_p[2]}, dV[3] = {fj.delta_v[0], fj.delta_v[1], fj.delta_v[2]};
  const double mv[3] = {moved.x, moved.y, moved.z}, ap[3] = {apart.x, apart.y, apart.z}, pl[3] = {pull.x, pull.y, pull.z};
  const double lb[3] = {F.tlb.x, F.tlb.y, F.tlb.z};
  for (int r = 0; r < 3; ++r) {
    tb[r] = with_g0 ? (((dP[r] + mv[r]) - lb[r]) - pl[r] * (dt * dt / 2.0)) - ap[r] : ((dP[r] + mv[r]) - lb[r]) - ap[r];
    tb[3 + r] = with_g0 ? dV[r] - pl[r] * dt : dV[r];
  }
  double rA[W][W], rb[W];
  for (int a = 0; a < W; ++a) {
    for (int c = 0; c < W; ++c) {
      double v = 0.0;
      for (int k = 0; k < 6; ++k) v += tA[k][a] * tA[k][c];
      rA[a][c] = v;
    }
    double v = 0.0;
    for (int k = 0; k < 6; ++k) v += tA[k][a] * tb[k];
    rb[a] = v;
  }
  const int at = 3 * i, tail = n_state - G;
  auto col = [&](int a) { return a < 6 ? at + a : tail + (a - 6); };
  for (int a = 0; a < W; ++a) {
    for (int c = 0; c < W; ++c) (*A)[static_cast<size_t>(col(a)) * n_state + col(c)] += rA[a][c];
    (*b)[col(a)] += rb[a];
  }
}

// Initializer::Initialization.  Vs: 3 n.  -> DLIOM_INIT_*
int initialization(const Frames& F, double g_norm, double* Vs, V3* g) {
  const int n = F.n;
  if (n < 7) return DLIOM_INIT_TOO_FEW_FRAMES;
  {  // ApproximateGravity
    const int n_state = 3 * n + 3;
    std::vector<double> A(static_cast<size_t>(n_state) * n_state, 0.0), b(n_state, 0.0), x(n_state, 0.0);
    const double identity[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int i = 0; i + 1 < n; ++i)
      if (F.f[i + 1].has_preintegration != 0) add_pair<3>(F, i, identity, V3{0.0, 0.0, 0.0}, false, &A, &b);
    for (double& v : A) v *= 1000.0;
    for (double& v : b) v *= 1000.0;
    if (!dliom::solve_sym(A.data(), b.data(), n_state, x.data())) return DLIOM_INIT_SINGULAR;
    *g = V3{x[n_state - 3], x[n_state - 2], x[n_state - 1]};
    if (!(std::fabs(std::sqrt(dot(*g, *g)) - g_norm) < 1.0)) return DLIOM_INIT_GRAVITY_NORM;
  }
  {  // RefineGravity: A and b are NOT cleared between the four passes (the reference's binary)
    const int n_state = 3 * n + 2;
    std::vector<double> A(static_cast<size_t>(n_state) * n_state, 0.0), b(n_state, 0.0), x(n_state, 0.0);
    V3 g0;
    if (!normalized(*g, &g0)) return DLIOM_INIT_SINGULAR;
    g0 = V3{g0.x * g_norm, g0.y * g_norm, g0.z * g_norm};
    for (int pass = 0; pass < 4; ++pass) {
      V3 lx, ly;
      if (!tangent_basis(g0, &lx, &ly)) return DLIOM_INIT_SINGULAR;
      const double basis[3][2] = {{lx.x, ly.x}, {lx.y, ly.y}, {lx.z, ly.z}};
      for (int i = 0; i + 1 < n; ++i)
        if (F.f[i + 1].has_preintegration != 0) add_pair<2>(F, i, basis, g0, true, &A, &b);
      for (double& v : A) v *= 1000.0;
      for (double& v : b) v *= 1000.0;
      if (!dliom::solve_sym(A.data(), b.data(), n_state, x.data())) return DLIOM_INIT_SINGULAR;
      const double d0 = x[n_state - 2], d1 = x[n_state - 1];
      V3 next;
      if (!normalized(V3{g0.x + (lx.x * d0 + ly.x * d1), g0.y + (lx.y * d0 + ly.y * d1), g0.z + (lx.z * d0 + ly.z * d1)}, &next))
        return DLIOM_INIT_SINGULAR;
      g0 = V3{next.x * g_norm, next.y * g_norm, next.z * g_norm};
    }
    *g = g0;
    for (int k = 0; k < 3 * n; ++k) Vs[k] = x[k];
    if (!(std::fabs(std::sqrt(dot(*g, *g)) - g_norm) < 0.2)) return DLIOM_INIT_GRAVITY_NORM;
  }
  return DLIOM_INIT_OK;
}

bool frames_ok(const dliom_init_frame* frames, int n, const double* transform_lb, double g_norm, Frames* F) {
  if (frames == nullptr || n < 1 || n > DLIOM_INIT_MAX_FRAMES || transform_lb == nullptr || !std::isfinite(g_norm) || !(g_norm > 0.0))
    return false;
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(transform_lb[k])) return false;
  F->f = frames;
  F->n = n;
  F->tlb = V3{transform_lb[0], transform_lb[1], transform_lb[2]};
  F->R.resize(9 * static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) {
    const dliom_init_frame& f = frames[i];
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(f.pose[k])) return false;
    if (f.has_preintegration != 0) {
      if (!std::isfinite(f.sum_dt) || !(f.sum_dt > 0.0) || !finite3(f.delta_p) || !finite3(f.delta_v)) return false;
    }
    rotation_of(&f.pose[3], &F->R[9 * static_cast<size_t>(i)]);
  }
  return true;
}

}  // namespace

extern "C" int dliom_imu_static_initialization(int64_t n, const double* acc, const double* gyr, double gravity_norm, double rotation9[9],
                                               double ba[3], double bg[3], double position[3], double velocity[3]) {
  if (n <= 0 || acc == nullptr || gyr == nullptr || rotation9 == nullptr || ba == nullptr || bg == nullptr || position == nullptr ||
      velocity == nullptr || !std::isfinite(gravity_norm) || !(gravity_norm > 0.0))
    return DLIOM_ERR_INVALID_ARGUMENT;
  double acc_sum[3] = {0.0, 0.0, 0.0}, gyr_sum[3] = {0.0, 0.0, 0.0};
  for (int64_t i = 0; i < n; ++i) {
    if (!finite3(acc + 3 * i) || !finite3(gyr + 3 * i)) return DLIOM_ERR_INVALID_ARGUMENT;
    for (int a = 0; a < 3; ++a) {
      acc_sum[a] += acc[3 * i + a];
      gyr_sum[a] += gyr[3 * i + a];
    }
  }
  const double count = static_cast<double>(n);
  const V3 acc_mean{acc_sum[0] / count, acc_sum[1] / count, acc_sum[2] / count};
  const V3 g_vec{0.0, 0.0, -gravity_norm};
  double q[4], R[9];
  if (!from_two_vectors(acc_mean, V3{-g_vec.x, -g_vec.y, -g_vec.z}, q)) return DLIOM_ERR_INVALID_ARGUMENT;  // no direction
  rotation_of(q, R);
  const double g[3] = {g_vec.x, g_vec.y, g_vec.z}, mean[3] = {acc_mean.x, acc_mean.y, acc_mean.z};
  for (int a = 0; a < 3; ++a) {
    // (R^T g_vec)_a + acc_mean_a, the product's sum left to right
    ba[a] = ((R[a] * g[0] + R[3 + a] * g[1]) + R[6 + a] * g[2]) + mean[a];
    bg[a] = gyr_sum[a] / count;
    position[a] = 0.0;
    velocity[a] = 0.0;
  }
  for (int k = 0; k < 9; ++k) rotation9[k] = R[k];
  return DLIOM_OK;
}

extern "C" int dliom_imu_lidar_initialization(const dliom_init_frame* frames, int num_frames, const double transform_lb[7],
                                              double gravity_norm, double* velocities, double gravity[3], int* outcome) {
  Frames F;
  if (velocities == nullptr || gravity == nullptr || outcome == nullptr || !frames_ok(frames, num_frames, transform_lb, gravity_norm, &F))
    return DLIOM_ERR_INVALID_ARGUMENT;
  V3 g{0.0, 0.0, 0.0};
  std::vector<double> Vs(3 * static_cast<size_t>(num_frames), 0.0);
  *outcome = initialization(F, gravity_norm, Vs.data(), &g);
  for (size_t k = 0; k < Vs.size(); ++k) velocities[k] = Vs[k];
  gravity[0] = g.x;
  gravity[1] = g.y;
  gravity[2] = g.z;
  return DLIOM_OK;
}

extern "C" int dliom_imu_lidar_align_with_world(const dliom_init_frame* frames, int num_frames, const double transform_lb[7],
                                                double gravity_norm, double* positions, double* rotations, double* velocities,
                                                double gravity_in_laser[3], double world_rotation9[9], double* excitation,
                                                int* outcome) {
  Frames F;
  if (positions == nullptr || rotations == nullptr || velocities == nullptr || gravity_in_laser == nullptr || world_rotation9 == nullptr ||
      excitation == nullptr || outcome == nullptr || num_frames < 2 || !frames_ok(frames, num_frames, transform_lb, gravity_norm, &F))
    return DLIOM_ERR_INVALID_ARGUMENT;
  const int n = num_frames, later = n - 1;  // frames_for_dynamic_initialization
  // the excitation test (:1012-1043); the reference leaves sum_g uninitialised, here it starts at zero
  const double count = static_cast<double>(later);
  V3 sum{0.0, 0.0, 0.0};
  for (int i = 0; i < later; ++i) {
    const dliom_init_frame& f = frames[i + 1];
    if (f.has_preintegration == 0) continue;
    sum = V3{sum.x + f.delta_v[0] / f.sum_dt, sum.y + f.delta_v[1] / f.sum_dt, sum.z + f.delta_v[2] / f.sum_dt};
  }
  const V3 mean{sum.x * 1.0 / count, sum.y * 1.0 / count, sum.z * 1.0 / count};
  double var = 0.0;
  for (int i = 0; i < later; ++i) {
    const dliom_init_frame& f = frames[i + 1];
    if (f.has_preintegration == 0) continue;
    const V3 d{f.delta_v[0] / f.sum_dt - mean.x, f.delta_v[1] / f.sum_dt - mean.y, f.delta_v[2] / f.sum_dt - mean.z};
    var += dot(d, d);
  }
  *excitation = std::sqrt(var / count);
  if (*excitation < 0.25) {
    *outcome = DLIOM_INIT_NO_EXCITATION;
    return DLIOM_OK;
  }
  V3 g{0.0, 0.0, 0.0};
  std::vector<double> Vs(3 * static_cast<size_t>(n), 0.0);
  *outcome = initialization(F, gravity_norm, Vs.data(), &g);
  gravity_in_laser[0] = g.x;
  gravity_in_laser[1] = g.y;
  gravity_in_laser[2] = g.z;
  if (*outcome != DLIOM_INIT_OK) return DLIOM_OK;
  // frame I to frame G (:1063-1071): the estimate is negated, then turned onto (0, 0, -1)
  V3 down;
  double q[4], Rw[9];
  if (!normalized(V3{-g.x, -g.y, -g.z}, &down) || !from_two_vectors(down, V3{0.0, 0.0, -1.0}, q)) return DLIOM_ERR_INVALID_ARGUMENT;
  rotation_of(q, Rw);
  const double* lb = transform_lb;
  for (int i = 0; i < n; ++i) {
    const double* li = frames[i].pose;
    const double* Rli = &F.R[9 * static_cast<size_t>(i)];
    // T_li * T_lb: translation R_li t_lb + t_li, rotation q_li q_lb, normalised
    const V3 t = mul(Rli, F.tlb);
    const V3 P{t.x + li[0], t.y + li[1], t.z + li[2]};
    double qq[4] = {((li[3] * lb[3] - li[4] * lb[4]) - li[5] * lb[5]) - li[6] * lb[6],
                    ((li[3] * lb[4] + li[4] * lb[3]) + li[5] * lb[6]) - li[6] * lb[5],
                    ((li[3] * lb[5] + li[5] * lb[3]) + li[6] * lb[4]) - li[4] * lb[6],
                    ((li[3] * lb[6] + li[6] * lb[3]) + li[4] * lb[5]) - li[5] * lb[4]};
    const double norm = std::sqrt(((qq[0] * qq[0] + qq[1] * qq[1]) + qq[2] * qq[2]) + qq[3] * qq[3]);
    if (!(norm > 0.0)) return DLIOM_ERR_INVALID_ARGUMENT;
    for (double& v : qq) v = v / norm;
    double Ri[9], Rout[9];
    rotation_of(qq, Ri);
    const V3 V = mul(Ri, V3{Vs[3 * i], Vs[3 * i + 1], Vs[3 * i + 2]});
    const V3 Pw = mul(Rw, P), Vw = mul(Rw, V);
    matmul(Rw, Ri, Rout);
    positions[3 * i] = Pw.x;
    positions[3 * i + 1] = Pw.y;
    positions[3 * i + 2] = Pw.z;
    velocities[3 * i] = Vw.x;
    velocities[3 * i + 1] = Vw.y;
    velocities[3 * i + 2] = Vw.z;
    for (int k = 0; k < 9; ++k) rotations[9 * i + k] = Rout[k];
  }
  for (int k = 0; k < 9; ++k) world_rotation9[k] = Rw[k];
  return DLIOM_OK;
}
