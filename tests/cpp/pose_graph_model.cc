// CPU model of the pose graph solve (test infrastructure, NOT product code): OptimizationProblem3D::Solve of the
// reference's fork (mapping/internal/optimization/optimization_problem_3d.cc:124-186 and :259-589, upstream's :335-338)
// on the oracle's restatement of Ceres 1.13 (oracle/src/om_jet.h, om_ceres.h, included unmodified).
//   * residual: the functor of cost_functions/cost_helpers_impl.h:57-101 with transform/transform.h:59-81 on Jet<14>
//     (submap rotation 0..3, submap translation 4..6, node rotation 7..10, node translation 11..13, the order of
//     SpaCostFunction3D's parameter blocks); sqrt / atan2 / sin / acos / abs of a Jet are added here (ceres/jet.h);
//   * local parameterisations, a kind per submap and fixed frame: QuaternionParameterization, SubsetParameterization(3,
//     {2}) under fix_z, the autodiff Jacobian of ConstantYawQuaternionPlus (rotation_parameterization.h:41-62) for the
//     gravity-aligned submap, YawOnlyQuaternionPlus for a fixed frame (:27-39: one column, slot 3, the step clamped to
//     +-0.5);
//   * fixed-frame blocks behind the submaps (translation without a parameterisation: mask 15 also under fix_z; never
//     constant) and their constraints behind the constraints, the same SpaCostFunction3D;
//   * ceres::HuberLoss and Corrector (Ceres 1.13 loss_function.cc, corrector.cc, residual_block.cc -- third-party
//     behaviour, restated) in the residual block's evaluation: after the tangent-space Jacobian is formed, s = ||r||^2,
//     the Jacobian and then the residual scaled by sqrt(rho'), the block's cost 1/2 rho;
//   * landmark blocks behind the nodes (translation without a parameterisation: six columns also under fix_z;
//     QuaternionParameterization) and one LandmarkCostFunction3D a used observation behind the other residual blocks,
//     without a loss.  The functor has the reference's shape (landmark_cost_function_3d.h:55-75 on cost_helpers_impl.h:
//     57-153) and runs on Jets over its 21 parameters;
//   * what leaves the reduced problem (Ceres' Program::RemoveFixedBlocks, third-party behaviour restated): constant
//     blocks, blocks no remaining residual uses, residuals whose blocks are all constant (-> fixed cost);
//   * the promoted layout: a non-constant node that a remaining observation names is a kept block.  The columns are the
//     submaps', the fixed frames', the promoted nodes', the landmarks', then the eliminated nodes'.  A residual block
//     between kept blocks only (a constraint of a promoted node, an observation) adds its J^T J to the reduced system
//     directly (eliminated normal equations) or joins the kept blocks' dense problem as six rows (structured QR);
//   * minimiser: om_ceres.h's Solve generalised to many blocks, with its LevenbergMarquardtStrategy and
//     TrustRegionStepEvaluator; three linear solvers: the strategy's own dense QR of [J; D] (solver 0), normal
//     equations with the nodes eliminated (solver 1), and the Householder QR of [J; D] with the nodes' columns first and
//     the operations on structural zeros left out (solver 2: no J^T J, no Cholesky; affordable on every case).
// Zero fixed frames, landmarks and observations and a zero huber_scale are ordinary values.  Honesty margins of a solve:
// loss_margin, the least |s - b| / b over the tagged constraints at every evaluated point; clamp_margin, the least
// ||delta| - 0.5| / 0.5 over every yaw step; slerp_margin, the least distance of |cos theta| from 1 - 1e-5 and of
// cos theta from 0 over every evaluated observation; each 1e300 where its term is absent.
// usage: pose_graph_model <in> <out> | pose_graph_model --reduces-noise <out-problem>
#include <cfloat>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../oracle/src/om_ceres.h"
#include "../../oracle/src/om_jet.h"

namespace oracle {
template <int N>
Jet<N> sqrt(const Jet<N>& f) {
  Jet<N> r;
  r.a = std::sqrt(f.a);
  const double two_a_inverse = 1.0 / (2.0 * r.a);
  for (int i = 0; i < N; ++i) r.v[i] = f.v[i] * two_a_inverse;
  return r;
}
template <int N>
Jet<N> atan2(const Jet<N>& g, const Jet<N>& f) {
  Jet<N> r;
  r.a = std::atan2(g.a, f.a);
  const double tmp = 1.0 / (f.a * f.a + g.a * g.a);
  for (int i = 0; i < N; ++i) r.v[i] = tmp * (-g.a * f.v[i] + f.a * g.v[i]);
  return r;
}
template <int N>
Jet<N> sin(const Jet<N>& f) {
  Jet<N> r;
  r.a = std::sin(f.a);
  const double c = std::cos(f.a);
  for (int i = 0; i < N; ++i) r.v[i] = c * f.v[i];
  return r;
}
template <int N>
Jet<N> acos(const Jet<N>& f) {
  Jet<N> r;
  r.a = std::acos(f.a);
  const double tmp = -1.0 / std::sqrt(1.0 - f.a * f.a);
  for (int i = 0; i < N; ++i) r.v[i] = tmp * f.v[i];
  return r;
}
template <int N>
Jet<N> abs(const Jet<N>& f) {
  return f.a < 0.0 ? -f : f;
}
template <int N>
bool operator<(const Jet<N>& f, double s) {
  return f.a < s;
}
}  // namespace oracle

namespace {
using oracle::ceres_like::DenseMatrix;
using oracle::ceres_like::LevenbergMarquardtStrategy;
using oracle::ceres_like::Options;
using oracle::ceres_like::TrustRegionStepEvaluator;
using std::abs;
using std::acos;
using std::atan2;
using std::sin;
using std::sqrt;

template <typename T>
T Make(double v);
template <>
double Make<double>(double v) {
  return v;
}
template <>
oracle::Jet<14> Make<oracle::Jet<14>>(double v) {
  return oracle::Jet<14>(v);
}

template <>
oracle::Jet<21> Make<oracle::Jet<21>>(double v) {
  return oracle::Jet<21>(v);
}

template <typename T>
struct Quat {  // Eigen::Quaternion<T>, w x y z
  T w, x, y, z;
};
template <typename T>
Quat<T> Mul(const Quat<T>& a, const Quat<T>& b) {
  return Quat<T>{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                 a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
// Eigen's QuaternionBase::_transformVector
template <typename T>
void Rotate(const Quat<T>& q, const T v[3], T out[3]) {
  const T vec[3] = {q.x, q.y, q.z};
  T uv[3] = {vec[1] * v[2] - vec[2] * v[1], vec[2] * v[0] - vec[0] * v[2], vec[0] * v[1] - vec[1] * v[0]};
  for (int k = 0; k < 3; ++k) uv[k] = uv[k] + uv[k];
  out[0] = v[0] + q.w * uv[0] + (vec[1] * uv[2] - vec[2] * uv[1]);
  out[1] = v[1] + q.w * uv[1] + (vec[2] * uv[0] - vec[0] * uv[2]);
  out[2] = v[2] + q.w * uv[2] + (vec[0] * uv[1] - vec[1] * uv[0]);
}
// transform.h:59-81
template <typename T>
void RotationQuaternionToAngleAxisVector(Quat<T> q, T out[3]) {
  const T squared = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
  if (oracle::ScalarPart(squared) > 0.) {
    const T norm = sqrt(squared);
    q = Quat<T>{q.w / norm, q.x / norm, q.y / norm, q.z / norm};
  }
  if (q.w < 0.) q = Quat<T>{-1. * q.w, -1. * q.x, -1. * q.y, -1. * q.z};
  const T angle = 2. * atan2(sqrt(q.x * q.x + q.y * q.y + q.z * q.z), q.w);
  constexpr double kCutoffAngle = 1e-7;
  const T scale = angle < kCutoffAngle ? Make<T>(2.) : angle / sin(angle / 2.);
  out[0] = scale * q.x;
  out[1] = scale * q.y;
  out[2] = scale * q.z;
}
// SpaCostFunction3D::operator() (spa_cost_function_3d.h:46-56)
template <typename T>
void SpaResidual(const double zbar[7], double translation_weight, double rotation_weight, const T* c_i_rotation,
                 const T* c_i_translation, const T* c_j_rotation, const T* c_j_translation, T* e) {
  const Quat<T> R_i_inverse{c_i_rotation[0], -c_i_rotation[1], -c_i_rotation[2], -c_i_rotation[3]};
  const T delta[3] = {c_j_translation[0] - c_i_translation[0], c_j_translation[1] - c_i_translation[1],
                      c_j_translation[2] - c_i_translation[2]};
  T h_translation[3];
  Rotate(R_i_inverse, delta, h_translation);
  const Quat<T> h_rotation_inverse = Mul(Quat<T>{c_j_rotation[0], -c_j_rotation[1], -c_j_rotation[2], -c_j_rotation[3]},
                                         Quat<T>{c_i_rotation[0], c_i_rotation[1], c_i_rotation[2], c_i_rotation[3]});
  T angle_axis[3];
  RotationQuaternionToAngleAxisVector(
      Mul(h_rotation_inverse, Quat<T>{Make<T>(zbar[3]), Make<T>(zbar[4]), Make<T>(zbar[5]), Make<T>(zbar[6])}), angle_axis);
  for (int k = 0; k < 3; ++k) {
    e[k] = (Make<T>(zbar[k]) - h_translation[k]) * translation_weight;
    e[3 + k] = angle_axis[k] * rotation_weight;
  }
}

// SlerpQuaternions and InterpolateNodes3D (cost_helpers_impl.h:103-153); *cos_theta_out: the scalar part, for the margin
template <typename T>
void InterpolateNodes3D(const T* prev_rotation, const T* prev_translation, const T* next_rotation, const T* next_translation,
                        double factor, T rotation[4], T translation[3], double* cos_theta_out) {
  const T* start = prev_rotation;
  const T* end = next_rotation;
  const T cos_theta = start[0] * end[0] + start[1] * end[1] + start[2] * end[2] + start[3] * end[3];
  *cos_theta_out = oracle::ScalarPart(cos_theta);
  const T abs_cos_theta = abs(cos_theta);
  T prev_scale = Make<T>(1. - factor);
  T next_scale = Make<T>(factor);
  if (abs_cos_theta < 1. - 1e-5) {
    const T theta = acos(abs_cos_theta);
    const T sin_theta = sin(theta);
    prev_scale = sin((1. - factor) * theta) / sin_theta;
    next_scale = sin(factor * theta) / sin_theta;
  }
  if (cos_theta < 0.) next_scale = -next_scale;
  for (int k = 0; k < 4; ++k) rotation[k] = prev_scale * start[k] + next_scale * end[k];
  for (int k = 0; k < 3; ++k) translation[k] = prev_translation[k] + factor * (next_translation[k] - prev_translation[k]);
}
// LandmarkCostFunction3D::operator() (landmark_cost_function_3d.h:55-75): ComputeUnscaledError's start is the interpolated
// pose, its end the landmark
template <typename T>
void LandmarkResidual(const double landmark_to_tracking[7], double translation_weight, double rotation_weight, double factor,
                      const T* prev_rotation, const T* prev_translation, const T* next_rotation, const T* next_translation,
                      const T* landmark_rotation, const T* landmark_translation, T* e, double* cos_theta) {
  T rotation[4], translation[3];
  InterpolateNodes3D(prev_rotation, prev_translation, next_rotation, next_translation, factor, rotation, translation, cos_theta);
  SpaResidual<T>(landmark_to_tracking, translation_weight, rotation_weight, rotation, translation, landmark_rotation,
                 landmark_translation, e);
}

struct Observation {
  int32_t landmark, prev_node, next_node;
  int32_t pad;
  double interpolation_parameter;
  double landmark_to_tracking[7];
  double translation_weight, rotation_weight;
};
static_assert(sizeof(Observation) == 96, "the layout of dliom_pose_graph_landmark_observation");

struct Constraint {
  int32_t submap, node;
  double zbar[7];
  double translation_weight, rotation_weight;
};
static_assert(sizeof(Constraint) == 80, "the layout of dliom_pose_graph_constraint");

struct Graph {
  int S = 0, N = 0, gravity = -1, fix_z = 0;  // S: the submaps and then the fixed frames
  int L = 0;                                  // landmarks: poses S + N ..
  std::vector<Observation> observations;      // residual blocks constraints.size() ..
  std::vector<char> observation_fixed, promoted;  // promoted: per node
  mutable double slerp_margin = 1e300;
  int P() const { return S + N + L; }
  bool Kept(int p) const { return p < S || p >= S + N || promoted[p - S]; }
  int ObservedPose(const Observation& o, int which) const { return which == 2 ? S + N + o.landmark : S + (which == 0 ? o.prev_node : o.next_node); }
  void SlerpMargin(double cos_theta) const {
    slerp_margin = std::min(slerp_margin, std::min(std::fabs(std::fabs(cos_theta) - (1. - 1e-5)), std::fabs(cos_theta)));
  }
  int submaps = 0;                            // how many of the kept blocks are submaps
  double huber_scale = 0;
  std::vector<char> lossy;                    // per constraint (the fixed frames' follow the submaps', submap = kept index)
  mutable double loss_margin = 1e300, clamp_margin = 1e300;
  int clamped_steps = 0;                      // yaw steps beyond +-0.5
  std::vector<double> x;  // 7 a pose [t, q], kept blocks first
  std::vector<int32_t> constant;
  std::vector<Constraint> constraints;
  // derived
  std::vector<int> mask;      // per pose: slots 0..2 translation, 3..5 rotation
  std::vector<int> column;    // 6 a pose: column of the reduced problem or -1
  std::vector<char> fixed;
  std::vector<int> rows;      // the constraints that stay
  int num_eff = 0;
  enum { kQuaternion = 0, kConstantYaw = 1, kYawOnly = 2 };
  int Kind(int p) const { return p == gravity ? kConstantYaw : (p >= submaps && p < S ? kYawOnly : kQuaternion); }
  // 1/2 rho(s) of constraint c and the corrector's scaling sqrt(rho') (rho'' <= 0: a pure scaling)
  double Loss(int c, double s, double* scaling) const {
    *scaling = 1.;
    if (!(huber_scale > 0.) || !lossy[c]) return 0.5 * s;
    const double b = huber_scale * huber_scale;
    loss_margin = std::min(loss_margin, std::fabs(s - b) / b);
    if (s <= b) return 0.5 * s;
    const double r = std::sqrt(s);
    *scaling = std::sqrt(std::max(DBL_MIN, huber_scale / r));
    return 0.5 * (2. * huber_scale * r - b);
  }

  void Derive() {
    const int P = S + N + L;
    mask.assign(P, 0);
    for (int p = 0; p < P; ++p) {
      if (constant[p]) continue;
      mask[p] = p == gravity ? 24 : (p >= submaps && p < S ? 15 : p >= S + N ? 63 : ((fix_z ? 3 : 7) | 56));
    }
    std::vector<int> used(P, 0);
    fixed.assign(constraints.size(), 0);
    rows.clear();
    for (size_t c = 0; c < constraints.size(); ++c) {
      const int a = constraints[c].submap, n = S + constraints[c].node;
      if (mask[a] == 0 && mask[n] == 0) {
        fixed[c] = 1;
        continue;
      }
      used[a] = used[n] = 1;
      rows.push_back(static_cast<int>(c));
    }
    observation_fixed.assign(observations.size(), 0);
    promoted.assign(N, 0);
    for (size_t o = 0; o < observations.size(); ++o) {
      const int p[3] = {ObservedPose(observations[o], 0), ObservedPose(observations[o], 1), ObservedPose(observations[o], 2)};
      if (mask[p[0]] == 0 && mask[p[1]] == 0 && mask[p[2]] == 0) {
        observation_fixed[o] = 1;
        continue;
      }
      for (int which = 0; which < 3; ++which) {
        used[p[which]] = 1;
        if (which < 2 && mask[p[which]] != 0) promoted[p[which] - S] = 1;
      }
    }
    column.assign(static_cast<size_t>(P) * 6, -1);
    num_eff = 0;
    for (int pass = 0; pass < 2; ++pass)  // the kept blocks' columns, then the eliminated nodes'
      for (int p = 0; p < P; ++p) {
        if (Kept(p) != (pass == 0)) continue;
        if (!used[p]) mask[p] = 0;
        for (int i = 0; i < 6; ++i)
          if ((mask[p] >> i) & 1) column[p * 6 + i] = num_eff++;
      }
  }
};

// d Plus / d delta at 0, 4 x 3 row-major (third column unused for the gravity-aligned submap)
void PlusJacobian(const double* q, int kind, double* j) {
  if (kind == Graph::kYawOnly) {
    // AutoDiffLocalParameterization<YawOnlyQuaternionPlus, 4, 1> at delta = 0: d sqrt(1 - d^2) = 0, so the column is
    // [0 0 0 1] (x) q
    const double e3[4] = {0, 0, 0, 1};
    double c[4];
    oracle::ceres_like::QuaternionProductD(e3, q, c);
    for (int k = 0; k < 4; ++k) j[k * 3] = c[k], j[k * 3 + 1] = 0., j[k * 3 + 2] = 0.;
  } else if (kind == Graph::kConstantYaw) {
    // AutoDiffLocalParameterization<ConstantYawQuaternionPlus, 4, 2> at delta = 0: the 1e-6 branch makes q_delta =
    // [1, d0, d1, 0], so the columns are q (x) [0 1 0 0] and q (x) [0 0 1 0]
    const double e1[4] = {0, 1, 0, 0}, e2[4] = {0, 0, 1, 0};
    double c1[4], c2[4];
    oracle::ceres_like::QuaternionProductD(q, e1, c1);
    oracle::ceres_like::QuaternionProductD(q, e2, c2);
    for (int k = 0; k < 4; ++k) j[k * 3] = c1[k], j[k * 3 + 1] = c2[k], j[k * 3 + 2] = 0.;
  } else {
    oracle::ceres_like::QuaternionParameterization().ComputeJacobian(q, j);
  }
}
void PosePlus(const double* x, const double* delta, int mask, int kind, double* out) {
  for (int k = 0; k < 3; ++k) out[k] = (mask >> k) & 1 ? x[k] + delta[k] : x[k];
  for (int k = 3; k < 7; ++k) out[k] = x[k];
  if ((mask & 56) == 0) return;
  if (kind == Graph::kYawOnly) {
    const double clamped = delta[3] > 0.5 ? 0.5 : (delta[3] < -0.5 ? -0.5 : delta[3]);  // common::Clamp
    const double q_delta[4] = {std::sqrt(1. - clamped * clamped), 0., 0., clamped};
    oracle::ceres_like::QuaternionProductD(q_delta, x + 3, out + 3);
  } else if (kind == Graph::kConstantYaw) {
    const double norm = std::sqrt(delta[3] * delta[3] + delta[4] * delta[4]);
    const double sin_over = norm < 1e-6 ? 1. : std::sin(norm) / norm;
    const double q_delta[4] = {norm < 1e-6 ? 1. : std::cos(norm), sin_over * delta[3], sin_over * delta[4], 0.};
    oracle::ceres_like::QuaternionProductD(x + 3, q_delta, out + 3);
  } else {
    oracle::ceres_like::QuaternionParameterization().Plus(x + 3, delta + 3, out + 3);
  }
}

struct RowBlock {  // one residual block's 6 rows in the tangent space, on the slots of its poses
  int c;            // constraints, then observations
  int num, pose[3];  // a constraint: the kept block and the node; an observation: prev, next, the landmark
  double r[6], j[3][36];
  bool direct;      // between kept blocks only: never in the elimination
};
struct Linearisation {
  double cost = 0, fixed_cost = 0;
  std::vector<RowBlock> blocks;
  std::vector<double> all_residuals;  // 6 a constraint, fixed ones included
};

void Residual(const Graph& g, const std::vector<double>& x, int c, double e[6]) {
  const Constraint& k = g.constraints[c];
  const double* a = &x[7 * k.submap];
  const double* n = &x[7 * (g.S + k.node)];
  SpaResidual<double>(k.zbar, k.translation_weight, k.rotation_weight, a + 3, a, n + 3, n, e);
}
bool Finite6(const double* e) {
  for (int k = 0; k < 6; ++k)
    if (!std::isfinite(e[k])) return false;
  return true;
}
// cost only; false: a non-finite residual (Ceres: the evaluation failed)
bool Cost(const Graph& g, const std::vector<double>& x, double* cost) {
  *cost = 0;
  for (int c : g.rows) {
    double e[6], sq = 0;
    Residual(g, x, c, e);
    if (!Finite6(e)) return false;
    for (int k = 0; k < 6; ++k) sq += e[k] * e[k];
    double scaling;
    *cost += g.Loss(c, sq, &scaling);
  }
  for (size_t o = 0; o < g.observations.size(); ++o) {
    if (g.observation_fixed[o]) continue;
    const Observation& k = g.observations[o];
    const double *a = &x[7 * g.ObservedPose(k, 0)], *b = &x[7 * g.ObservedPose(k, 1)], *l = &x[7 * g.ObservedPose(k, 2)];
    double e[6], sq = 0, cos_theta;
    LandmarkResidual<double>(k.landmark_to_tracking, k.translation_weight, k.rotation_weight, k.interpolation_parameter, a + 3, a,
                             b + 3, b, l + 3, l, e, &cos_theta);
    g.SlerpMargin(cos_theta);
    if (!Finite6(e)) return false;
    for (int i = 0; i < 6; ++i) sq += e[i] * e[i];
    *cost += 0.5 * sq;
  }
  return true;
}
bool Linearise(const Graph& g, const std::vector<double>& x, Linearisation* out) {
  using J = oracle::Jet<14>;
  out->cost = out->fixed_cost = 0;
  out->blocks.clear();
  out->all_residuals.assign((g.constraints.size() + g.observations.size()) * 6, 0.);
  for (size_t c = 0; c < g.constraints.size(); ++c) {
    const Constraint& k = g.constraints[c];
    const int pa = k.submap, pn = g.S + k.node;
    const double* a = &x[7 * pa];
    const double* n = &x[7 * pn];
    J qi[4], ti[3], qj[4], tj[3], e[6];
    for (int i = 0; i < 4; ++i) qi[i] = J(a[3 + i], i), qj[i] = J(n[3 + i], 7 + i);
    for (int i = 0; i < 3; ++i) ti[i] = J(a[i], 4 + i), tj[i] = J(n[i], 11 + i);
    SpaResidual<J>(k.zbar, k.translation_weight, k.rotation_weight, qi, ti, qj, tj, e);
    RowBlock b;
    b.c = static_cast<int>(c);
    b.num = 2, b.pose[0] = pa, b.pose[1] = pn, b.pose[2] = -1;
    b.direct = g.promoted[k.node] != 0;
    double sq = 0;
    for (int i = 0; i < 6; ++i) b.r[i] = e[i].a, sq += e[i].a * e[i].a;
    if (!Finite6(b.r)) return false;
    double scaling;
    const double cost = g.Loss(static_cast<int>(c), sq, &scaling);
    for (int i = 0; i < 6; ++i) out->all_residuals[6 * c + i] = e[i].a * scaling;
    if (g.fixed[c]) {
      out->fixed_cost += cost;
      continue;
    }
    out->cost += cost;
    double ja[12], jn[12];
    PlusJacobian(a + 3, g.Kind(pa), ja);
    PlusJacobian(n + 3, Graph::kQuaternion, jn);
    for (int row = 0; row < 6; ++row)
      for (int slot = 0; slot < 6; ++slot) {
        double vs = 0, vn = 0;
        if (slot < 3) {
          vs = e[row].v[4 + slot];
          vn = e[row].v[11 + slot];
        } else {
          for (int q = 0; q < 4; ++q) vs += e[row].v[q] * ja[q * 3 + slot - 3], vn += e[row].v[7 + q] * jn[q * 3 + slot - 3];
        }
        b.j[0][row * 6 + slot] = (g.mask[pa] >> slot) & 1 ? vs : 0.;
        b.j[1][row * 6 + slot] = (g.mask[pn] >> slot) & 1 ? vn : 0.;
      }
    // Corrector: the Jacobian first, then the residual
    for (int k = 0; k < 36; ++k) b.j[0][k] *= scaling, b.j[1][k] *= scaling;
    for (int k = 0; k < 6; ++k) b.r[k] *= scaling;
    out->blocks.push_back(b);
  }
  using J21 = oracle::Jet<21>;
  for (size_t o = 0; o < g.observations.size(); ++o) {
    const Observation& k = g.observations[o];
    // parameter order of the AutoDiffCostFunction: per pose rotation (4), translation (3)
    J21 q[3][4], t[3][3], e[6];
    RowBlock b;
    b.c = static_cast<int>(g.constraints.size() + o);
    b.num = 3;
    b.direct = true;
    for (int which = 0; which < 3; ++which) {
      b.pose[which] = g.ObservedPose(k, which);
      const double* p = &x[7 * b.pose[which]];
      for (int i = 0; i < 4; ++i) q[which][i] = J21(p[3 + i], 7 * which + i);
      for (int i = 0; i < 3; ++i) t[which][i] = J21(p[i], 7 * which + 4 + i);
    }
    double cos_theta;
    LandmarkResidual<J21>(k.landmark_to_tracking, k.translation_weight, k.rotation_weight, k.interpolation_parameter, q[0], t[0], q[1],
                          t[1], q[2], t[2], e, &cos_theta);
    g.SlerpMargin(cos_theta);
    double sq = 0;
    for (int i = 0; i < 6; ++i) b.r[i] = e[i].a, sq += e[i].a * e[i].a;
    if (!Finite6(b.r)) return false;
    for (int i = 0; i < 6; ++i) out->all_residuals[6 * b.c + i] = e[i].a;
    if (g.observation_fixed[o]) {
      out->fixed_cost += 0.5 * sq;
      continue;
    }
    out->cost += 0.5 * sq;
    for (int which = 0; which < 3; ++which) {
      double jq[12];
      PlusJacobian(&x[7 * b.pose[which] + 3], Graph::kQuaternion, jq);
      for (int row = 0; row < 6; ++row)
        for (int slot = 0; slot < 6; ++slot) {
          double v = 0;
          if (slot < 3) {
            v = e[row].v[7 * which + 4 + slot];
          } else {
            for (int i = 0; i < 4; ++i) v += e[row].v[7 * which + i] * jq[i * 3 + slot - 3];
          }
          b.j[which][row * 6 + slot] = (g.mask[b.pose[which]] >> slot) & 1 ? v : 0.;
        }
    }
    out->blocks.push_back(b);
  }
  return true;
}

// ---- the two linear solvers ------------------------------------------------------------------------------------------------
// scaled Jacobian as a dense matrix (solver 0)
void Dense(const Graph& g, const Linearisation& lin, const std::vector<double>& scale, DenseMatrix* jac, std::vector<double>* r) {
  jac->Resize(static_cast<int>(lin.blocks.size()) * 6, g.num_eff);
  r->assign(lin.blocks.size() * 6, 0.);
  for (size_t b = 0; b < lin.blocks.size(); ++b) {
    const RowBlock& k = lin.blocks[b];
    for (int row = 0; row < 6; ++row) {
      (*r)[b * 6 + row] = k.r[row];
      for (int slot = 0; slot < 6; ++slot)
        for (int which = 0; which < k.num; ++which) {
          const int col = g.column[k.pose[which] * 6 + slot];
          if (col >= 0) (*jac)(static_cast<int>(b) * 6 + row, col) = k.j[which][row * 6 + slot] * scale[col];
        }
    }
  }
}
bool CholeskySolve(std::vector<double>* a, int n, std::vector<double>* b) {  // a: row-major, lower used; in place
  std::vector<double>& A = *a;
  for (int j = 0; j < n; ++j) {
    double d = A[static_cast<size_t>(j) * n + j];
    for (int k = 0; k < j; ++k) d -= A[static_cast<size_t>(j) * n + k] * A[static_cast<size_t>(j) * n + k];
    if (!(d > 0.)) return false;
    d = std::sqrt(d);
    A[static_cast<size_t>(j) * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double t = A[static_cast<size_t>(i) * n + j];
      const double* ri = &A[static_cast<size_t>(i) * n];
      const double* rj = &A[static_cast<size_t>(j) * n];
      for (int k = 0; k < j; ++k) t -= ri[k] * rj[k];
      A[static_cast<size_t>(i) * n + j] = t / d;
    }
  }
  std::vector<double>& y = *b;
  for (int i = 0; i < n; ++i) {
    double t = y[i];
    for (int k = 0; k < i; ++k) t -= A[static_cast<size_t>(i) * n + k] * y[k];
    y[i] = t / A[static_cast<size_t>(i) * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double t = y[i];
    for (int k = i + 1; k < n; ++k) t -= A[static_cast<size_t>(k) * n + i] * y[k];
    y[i] = t / A[static_cast<size_t>(i) * n + i];
  }
  return true;
}
// Normal equations (J^T J + D^2) y = -J^T r on the scaled columns with the nodes eliminated (solver 1).
bool EliminatedStep(const Graph& g, const Linearisation& lin, const std::vector<double>& scale, double radius, double min_diagonal,
                    double max_diagonal, std::vector<double>* step) {
  const int n_all = g.num_eff;
  int ns = 0;  // the submaps' columns come first
  for (int p = 0; p < g.P(); ++p)
    for (int i = 0; i < 6; ++i) ns += g.Kept(p) && g.column[p * 6 + i] >= 0;
  std::vector<double> diagonal(n_all, 0.), gradient(n_all, 0.);
  std::vector<double> S(static_cast<size_t>(ns) * ns, 0.), rhs(ns, 0.);
  std::vector<double> hnn(static_cast<size_t>(g.N) * 36, 0.);
  std::vector<std::vector<int>> of_node(g.N);
  auto scaled_at = [&](const RowBlock& k, int which, int row, int slot) {
    const int col = g.column[k.pose[which] * 6 + slot];
    return col < 0 ? 0. : k.j[which][row * 6 + slot] * scale[col];
  };
  auto scaled = [&](const RowBlock& k, bool node, int row, int slot) { return scaled_at(k, node ? 1 : 0, row, slot); };
  for (size_t b = 0; b < lin.blocks.size(); ++b) {
    const RowBlock& k = lin.blocks[b];
    if (k.direct) {  // J^T J and J^T r of a block between kept blocks, straight into the reduced system
      for (int x = 0; x < k.num; ++x)
        for (int i = 0; i < 6; ++i) {
          const int ci = g.column[k.pose[x] * 6 + i];
          if (ci < 0) continue;
          for (int row = 0; row < 6; ++row) gradient[ci] += scaled_at(k, x, row, i) * k.r[row];
          for (int y = 0; y < k.num; ++y)
            for (int j = 0; j < 6; ++j) {
              const int cj = g.column[k.pose[y] * 6 + j];
              if (cj < 0) continue;
              double t = 0;
              for (int row = 0; row < 6; ++row) t += scaled_at(k, x, row, i) * scaled_at(k, y, row, j);
              S[static_cast<size_t>(ci) * ns + cj] += t;
            }
        }
      continue;
    }
    const int pa = k.pose[0], node = (k.pose[1] - g.S);
    of_node[node].push_back(static_cast<int>(b));
    for (int i = 0; i < 6; ++i) {
      const int ci = g.column[pa * 6 + i], cn = g.column[(g.S + node) * 6 + i];
      for (int row = 0; row < 6; ++row) {
        if (ci >= 0) gradient[ci] += scaled(k, false, row, i) * k.r[row];
        if (cn >= 0) gradient[cn] += scaled(k, true, row, i) * k.r[row];
      }
      for (int j = 0; j < 6; ++j) {
        const int cj = g.column[pa * 6 + j];
        double ss = 0, nn = 0;
        for (int row = 0; row < 6; ++row) ss += scaled(k, false, row, i) * scaled(k, false, row, j), nn += scaled(k, true, row, i) * scaled(k, true, row, j);
        if (ci >= 0 && cj >= 0) S[static_cast<size_t>(ci) * ns + cj] += ss;
        hnn[static_cast<size_t>(node) * 36 + i * 6 + j] += nn;
      }
    }
  }
  for (int c = 0; c < ns; ++c) diagonal[c] = S[static_cast<size_t>(c) * ns + c];
  for (int node = 0; node < g.N; ++node)
    for (int i = 0; i < 6; ++i)
      if (!g.promoted[node] && g.column[(g.S + node) * 6 + i] >= 0) diagonal[g.column[(g.S + node) * 6 + i]] = hnn[static_cast<size_t>(node) * 36 + i * 7];
  for (int c = 0; c < n_all; ++c) diagonal[c] = std::min(std::max(diagonal[c], min_diagonal), max_diagonal) / radius;
  for (int c = 0; c < ns; ++c) S[static_cast<size_t>(c) * ns + c] += diagonal[c], rhs[c] = -gradient[c];
  std::vector<double> V(static_cast<size_t>(g.N) * 36, 0.);
  for (int node = 0; node < g.N; ++node) {
    if (of_node[node].empty() || g.mask[g.S + node] == 0) continue;
    // V = (H_nn + D^2)^-1 on the node's columns
    int cols[6], m = 0;
    for (int i = 0; i < 6; ++i)
      if (g.column[(g.S + node) * 6 + i] >= 0) cols[m++] = i;
    for (int col = 0; col < m; ++col) {
      std::vector<double> a(static_cast<size_t>(m) * m), e(m, 0.);
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j)
          a[i * m + j] = hnn[static_cast<size_t>(node) * 36 + cols[i] * 6 + cols[j]] + (i == j ? diagonal[g.column[(g.S + node) * 6 + cols[i]]] : 0.);
      e[col] = 1.;
      if (!CholeskySolve(&a, m, &e)) return false;
      for (int i = 0; i < m; ++i) V[static_cast<size_t>(node) * 36 + cols[i] * 6 + cols[col]] = e[i];
    }
    // S -= W V W^T, rhs += W V g_n over the node's constraints
    double vg[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j)
        if (g.column[(g.S + node) * 6 + j] >= 0) vg[i] += V[static_cast<size_t>(node) * 36 + i * 6 + j] * gradient[g.column[(g.S + node) * 6 + j]];
    for (int b1 : of_node[node]) {
      const RowBlock& k1 = lin.blocks[b1];
      double w1[36], w1v[36];
      for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
          double t = 0;
          for (int row = 0; row < 6; ++row) t += scaled(k1, false, row, i) * scaled(k1, true, row, j);
          w1[i * 6 + j] = t;
        }
      for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
          double t = 0;
          for (int q = 0; q < 6; ++q) t += w1[i * 6 + q] * V[static_cast<size_t>(node) * 36 + q * 6 + j];
          w1v[i * 6 + j] = t;
        }
      const int pa = k1.pose[0];
      for (int i = 0; i < 6; ++i) {
        const int ci = g.column[pa * 6 + i];
        if (ci < 0) continue;
        for (int q = 0; q < 6; ++q) rhs[ci] += w1[i * 6 + q] * vg[q];
      }
      for (int b2 : of_node[node]) {
        const RowBlock& k2 = lin.blocks[b2];
        const int pb = k2.pose[0];
        for (int i = 0; i < 6; ++i) {
          const int ci = g.column[pa * 6 + i];
          if (ci < 0) continue;
          for (int j = 0; j < 6; ++j) {
            const int cj = g.column[pb * 6 + j];
            if (cj < 0) continue;
            double t = 0;
            for (int q = 0; q < 6; ++q) {
              double w2 = 0;
              for (int row = 0; row < 6; ++row) w2 += scaled(k2, false, row, j) * scaled(k2, true, row, q);
              t += w1v[i * 6 + q] * w2;
            }
            S[static_cast<size_t>(ci) * ns + cj] -= t;
          }
        }
      }
    }
  }
  if (ns > 0 && !CholeskySolve(&S, ns, &rhs)) return false;
  step->assign(n_all, 0.);
  for (int c = 0; c < ns; ++c) (*step)[c] = rhs[c];
  for (int node = 0; node < g.N; ++node) {
    if (of_node[node].empty() || g.mask[g.S + node] == 0) continue;
    double w[6];
    for (int j = 0; j < 6; ++j) w[j] = g.column[(g.S + node) * 6 + j] >= 0 ? gradient[g.column[(g.S + node) * 6 + j]] : 0.;
    for (int b : of_node[node]) {
      const RowBlock& k = lin.blocks[b];
      const int pa = k.pose[0];
      for (int i = 0; i < 6; ++i) {
        const int ci = g.column[pa * 6 + i];
        if (ci < 0) continue;
        for (int j = 0; j < 6; ++j) {
          double t = 0;
          for (int row = 0; row < 6; ++row) t += scaled(k, false, row, i) * scaled(k, true, row, j);
          w[j] += t * rhs[ci];
        }
      }
    }
    for (int i = 0; i < 6; ++i) {
      const int ci = g.column[(g.S + node) * 6 + i];
      if (ci < 0) continue;
      double t = 0;
      for (int j = 0; j < 6; ++j) t += V[static_cast<size_t>(node) * 36 + i * 6 + j] * w[j];
      (*step)[ci] = -t;
    }
  }
  for (double v : *step)
    if (!std::isfinite(v)) return false;
  return true;
}

// Householder QR of the first `factor` columns of a column-major rows x cols matrix (the formulas of om_ceres.h's
// HouseholderQrSolve), applied to all its columns.
void HouseholderColumns(std::vector<double>* matrix, int rows, int cols, int factor) {
  std::vector<double>& a = *matrix;
  auto at = [&](int i, int j) -> double& { return a[static_cast<size_t>(j) * rows + i]; };
  for (int k = 0; k < factor && k < rows; ++k) {
    double tail_sq = 0.0;
    for (int i = k + 1; i < rows; ++i) tail_sq += at(i, k) * at(i, k);
    const double c0 = at(k, k);
    double beta, tau;
    if (tail_sq <= std::numeric_limits<double>::min()) {
      tau = 0.0;
      beta = c0;
      for (int i = k + 1; i < rows; ++i) at(i, k) = 0.0;
    } else {
      beta = std::sqrt(c0 * c0 + tail_sq);
      if (c0 >= 0.0) beta = -beta;
      for (int i = k + 1; i < rows; ++i) at(i, k) /= (c0 - beta);
      tau = (beta - c0) / beta;
    }
    at(k, k) = beta;
    if (tau == 0.0) continue;
    for (int j = k + 1; j < cols; ++j) {
      double* cj = &a[static_cast<size_t>(j) * rows];
      const double* ck = &a[static_cast<size_t>(k) * rows];
      double sum = cj[k];
      for (int i = k + 1; i < rows; ++i) sum += ck[i] * cj[i];
      sum *= tau;
      cj[k] -= sum;
      for (int i = k + 1; i < rows; ++i) cj[i] -= sum * ck[i];
    }
  }
}
// min ||[J; D] y - [r; 0]|| by Householder QR with the nodes' columns first.  The rows of a node's columns are its own
// constraints' and its own D rows, so each node is factorised in a small dense matrix over its columns and those of the
// submaps it touches; what is left of its rows joins the submaps' dense problem.  step = -y.
bool SparseQrStep(const Graph& g, const Linearisation& lin, const std::vector<double>& scale, double radius, double min_diagonal,
                  double max_diagonal, std::vector<double>* step) {
  const int n_all = g.num_eff;
  int ns = 0;
  for (int p = 0; p < g.P(); ++p)
    for (int i = 0; i < 6; ++i) ns += g.Kept(p) && g.column[p * 6 + i] >= 0;
  std::vector<double> diagonal(n_all, 0.);
  std::vector<std::vector<int>> of_node(g.N);
  auto scaled_at = [&](const RowBlock& k, int which, int row, int slot) {
    const int col = g.column[k.pose[which] * 6 + slot];
    return col < 0 ? 0. : k.j[which][row * 6 + slot] * scale[col];
  };
  auto scaled = [&](const RowBlock& k, bool node, int row, int slot) { return scaled_at(k, node ? 1 : 0, row, slot); };
  for (size_t b = 0; b < lin.blocks.size(); ++b) {
    const RowBlock& k = lin.blocks[b];
    if (!k.direct) of_node[(k.pose[1] - g.S)].push_back(static_cast<int>(b));
    for (int which = 0; which < k.num; ++which)
      for (int slot = 0; slot < 6; ++slot) {
        const int col = g.column[k.pose[which] * 6 + slot];
        if (col < 0) continue;
        for (int row = 0; row < 6; ++row) diagonal[col] += scaled_at(k, which, row, slot) * scaled_at(k, which, row, slot);
      }
  }
  std::vector<double> lm(n_all);
  for (int c = 0; c < n_all; ++c) lm[c] = std::sqrt(std::min(std::max(diagonal[c], min_diagonal), max_diagonal) / radius);
  // the submaps' problem: rows appended as (dense row over ns columns, rhs)
  std::vector<std::vector<double>> reduced_rows;
  struct NodeFactor {
    int m, q;
    std::vector<int> node_cols, submap_cols;
    std::vector<double> r;  // m x (m + q + 1): R_nn | R_ns | c
  };
  std::vector<NodeFactor> factors(g.N);
  for (int node = 0; node < g.N; ++node) {
    if (of_node[node].empty()) continue;
    NodeFactor& f = factors[node];
    for (int i = 0; i < 6; ++i)
      if (g.column[(g.S + node) * 6 + i] >= 0) f.node_cols.push_back(i);
    f.m = static_cast<int>(f.node_cols.size());
    for (int b : of_node[node]) {
      const int pa = lin.blocks[b].pose[0];
      for (int i = 0; i < 6; ++i) {
        const int c = g.column[pa * 6 + i];
        if (c >= 0 && std::find(f.submap_cols.begin(), f.submap_cols.end(), c) == f.submap_cols.end()) f.submap_cols.push_back(c);
      }
    }
    f.q = static_cast<int>(f.submap_cols.size());
    const int rows = 6 * static_cast<int>(of_node[node].size()) + f.m, cols = f.m + f.q + 1;
    std::vector<double> a(static_cast<size_t>(rows) * cols, 0.);
    auto at = [&](int i, int j) -> double& { return a[static_cast<size_t>(j) * rows + i]; };
    int row0 = 0;
    for (int b : of_node[node]) {
      const RowBlock& k = lin.blocks[b];
      const int pa = k.pose[0];
      for (int row = 0; row < 6; ++row) {
        for (int j = 0; j < f.m; ++j) at(row0 + row, j) = scaled(k, true, row, f.node_cols[j]);
        for (int i = 0; i < 6; ++i) {
          const int c = g.column[pa * 6 + i];
          if (c < 0) continue;
          const int j = static_cast<int>(std::find(f.submap_cols.begin(), f.submap_cols.end(), c) - f.submap_cols.begin());
          at(row0 + row, f.m + j) += scaled(k, false, row, i);
        }
        at(row0 + row, cols - 1) = k.r[row];
      }
      row0 += 6;
    }
    for (int j = 0; j < f.m; ++j) at(row0 + j, j) = lm[g.column[(g.S + node) * 6 + f.node_cols[j]]];
    HouseholderColumns(&a, rows, cols, f.m);
    f.r.assign(static_cast<size_t>(f.m) * cols, 0.);
    for (int i = 0; i < f.m; ++i)
      for (int j = i; j < cols; ++j) f.r[static_cast<size_t>(i) * cols + j] = at(i, j);
    for (int i = f.m; i < rows; ++i) {
      std::vector<double> dense(ns + 1, 0.);
      for (int j = 0; j < f.q; ++j) dense[f.submap_cols[j]] = at(i, f.m + j);
      dense[ns] = at(i, cols - 1);
      reduced_rows.push_back(dense);
    }
  }
  // a block between kept blocks only: its six rows as they are
  for (const RowBlock& k : lin.blocks) {
    if (!k.direct) continue;
    for (int row = 0; row < 6; ++row) {
      std::vector<double> dense(ns + 1, 0.);
      for (int which = 0; which < k.num; ++which)
        for (int slot = 0; slot < 6; ++slot)
          if (g.column[k.pose[which] * 6 + slot] >= 0) dense[g.column[k.pose[which] * 6 + slot]] = scaled_at(k, which, row, slot);
      dense[ns] = k.r[row];
      reduced_rows.push_back(dense);
    }
  }
  step->assign(n_all, 0.);
  std::vector<double> ys(ns, 0.);
  if (ns > 0) {
    const int rows = static_cast<int>(reduced_rows.size()) + ns, cols = ns + 1;
    std::vector<double> a(static_cast<size_t>(rows) * cols, 0.);
    for (size_t i = 0; i < reduced_rows.size(); ++i)
      for (int j = 0; j < cols; ++j) a[static_cast<size_t>(j) * rows + i] = reduced_rows[i][j];
    for (int j = 0; j < ns; ++j) a[static_cast<size_t>(j) * rows + reduced_rows.size() + j] = lm[j];
    HouseholderColumns(&a, rows, cols, ns);
    for (int k = ns - 1; k >= 0; --k) {
      double t = a[static_cast<size_t>(ns) * rows + k];
      for (int j = k + 1; j < ns; ++j) t -= a[static_cast<size_t>(j) * rows + k] * ys[j];
      if (a[static_cast<size_t>(k) * rows + k] == 0.0) return false;
      ys[k] = t / a[static_cast<size_t>(k) * rows + k];
    }
    for (int c = 0; c < ns; ++c) (*step)[c] = -ys[c];
  }
  for (int node = 0; node < g.N; ++node) {
    const NodeFactor& f = factors[node];
    if (of_node[node].empty() || f.m == 0) continue;
    const int cols = f.m + f.q + 1;
    std::vector<double> y(f.m, 0.);
    for (int k = f.m - 1; k >= 0; --k) {
      double t = f.r[static_cast<size_t>(k) * cols + cols - 1];
      for (int j = 0; j < f.q; ++j) t -= f.r[static_cast<size_t>(k) * cols + f.m + j] * ys[f.submap_cols[j]];
      for (int j = k + 1; j < f.m; ++j) t -= f.r[static_cast<size_t>(k) * cols + j] * y[j];
      if (f.r[static_cast<size_t>(k) * cols + k] == 0.0) return false;
      y[k] = t / f.r[static_cast<size_t>(k) * cols + k];
    }
    for (int j = 0; j < f.m; ++j) (*step)[g.column[(g.S + node) * 6 + f.node_cols[j]]] = -y[j];
  }
  for (double v : *step)
    if (!std::isfinite(v)) return false;
  return true;
}

// ---- the minimiser: om_ceres.h's Solve (trust_region_minimizer.cc) over many blocks ----------------------------------------
struct Result {
  int termination = 0, iterations = 0, successful = 0, unsuccessful = 0;
  double initial_cost = 0, final_cost = 0, seconds = 0;
  std::vector<int> steps;  // 1 successful, 0 unsuccessful, 2 invalid
  int rises = 0;  // successful steps after which the cost is higher than before
  double quality_margin = 1e300;    // min over steps of |quality - min_relative_decrease| / min_relative_decrease
  double tolerance_margin = 1e300;  // min over the tolerance tests of |value - threshold| / threshold
};

struct State {
  const Graph* g;
  std::vector<double> scale;
  Linearisation lin;
  std::vector<double> gradient;  // unscaled, per column
  double gradient_max_norm = 0, x_norm = 0;
};
double ReducedNorm(const Graph& g, const std::vector<double>& x) {
  double s = 0;
  for (int p = 0; p < g.P(); ++p) {
    if (g.mask[p] & 7)
      for (int k = 0; k < 3; ++k) s += x[7 * p + k] * x[7 * p + k];
    if (g.mask[p] & 56)
      for (int k = 3; k < 7; ++k) s += x[7 * p + k] * x[7 * p + k];
  }
  return std::sqrt(s);
}
void SlotsFromColumns(const Graph& g, const std::vector<double>& v, std::vector<double>* slots) {
  slots->assign(static_cast<size_t>(g.P()) * 6, 0.);
  for (size_t i = 0; i < slots->size(); ++i)
    if (g.column[i] >= 0) (*slots)[i] = v[g.column[i]];
}
void PlusAll(const Graph& g, const std::vector<double>& x, const std::vector<double>& delta_columns, std::vector<double>* out) {
  std::vector<double> slots;
  SlotsFromColumns(g, delta_columns, &slots);
  out->resize(x.size());
  for (int p = 0; p < g.P(); ++p) PosePlus(&x[7 * p], &slots[6 * p], g.mask[p], g.Kind(p), &(*out)[7 * p]);
}
bool EvaluateGradientAndJacobian(const Graph& g, const std::vector<double>& x, bool first, State* s) {
  if (!Linearise(g, x, &s->lin)) return false;
  s->gradient.assign(g.num_eff, 0.);
  std::vector<double> squared(g.num_eff, 0.);
  for (const RowBlock& k : s->lin.blocks)
    for (int which = 0; which < k.num; ++which)
      for (int slot = 0; slot < 6; ++slot) {
        const int col = g.column[k.pose[which] * 6 + slot];
        if (col < 0) continue;
        const double* j = k.j[which];
        for (int row = 0; row < 6; ++row) s->gradient[col] += j[row * 6 + slot] * k.r[row], squared[col] += j[row * 6 + slot] * j[row * 6 + slot];
      }
  if (first) {
    s->scale.assign(g.num_eff, 1.);
    for (int c = 0; c < g.num_eff; ++c) s->scale[c] = 1.0 / (1.0 + std::sqrt(squared[c]));
  }
  std::vector<double> negative(g.num_eff), projected;
  for (int c = 0; c < g.num_eff; ++c) negative[c] = -s->gradient[c];
  PlusAll(g, x, negative, &projected);
  s->gradient_max_norm = 0;
  for (int p = 0; p < g.P(); ++p)
    for (int k = 0; k < 7; ++k)
      if ((k < 3 ? g.mask[p] & 7 : g.mask[p] & 56) != 0)
        s->gradient_max_norm = std::max(s->gradient_max_norm, std::fabs(x[7 * p + k] - projected[7 * p + k]));
  s->x_norm = ReducedNorm(g, x);
  return true;
}
// One trust-region step on the scaled columns; `strategy` keeps the radius.  false: the linear solver failed.
bool ComputeStep(const Graph& g, const State& s, int solver, const Options& o, LevenbergMarquardtStrategy* strategy,
                 std::vector<double>* step, double* model_cost_change) {
  step->assign(g.num_eff, 0.);
  bool solved;
  if (solver == 0) {
    DenseMatrix jac;
    std::vector<double> r;
    Dense(g, s.lin, s.scale, &jac, &r);
    solved = strategy->ComputeStep(jac, r.data(), step->data());
  } else if (solver == 2) {
    solved = SparseQrStep(g, s.lin, s.scale, strategy->Radius(), o.min_lm_diagonal, o.max_lm_diagonal, step);
  } else {
    solved = EliminatedStep(g, s.lin, s.scale, strategy->Radius(), o.min_lm_diagonal, o.max_lm_diagonal, step);
  }
  if (!solved) return false;
  std::vector<double> slots, scales;
  SlotsFromColumns(g, *step, &slots);
  SlotsFromColumns(g, s.scale, &scales);
  double dot = 0;
  for (const RowBlock& k : s.lin.blocks) {
    for (int row = 0; row < 6; ++row) {
      double m = 0;
      for (int slot = 0; slot < 6; ++slot) {
        double t = k.j[0][row * 6 + slot] * scales[k.pose[0] * 6 + slot] * slots[k.pose[0] * 6 + slot];
        for (int which = 1; which < k.num; ++which) t += k.j[which][row * 6 + slot] * scales[k.pose[which] * 6 + slot] * slots[k.pose[which] * 6 + slot];
        m += t;
      }
      dot += m * (k.r[row] + m / 2.0);
    }
  }
  *model_cost_change = -dot;
  return true;
}
void Margin(double value, double threshold, double* margin) {
  if (threshold > 0) *margin = std::min(*margin, std::fabs(value - threshold) / threshold);
}

void Solve(const Options& options, int solver, Graph* g, Result* out) {
  const auto started = std::chrono::steady_clock::now();
  std::vector<double> x = g->x, candidate_x, best_x = g->x, delta(g->num_eff), step;
  std::vector<double> iteration_costs;
  State s;
  s.g = g;
  LevenbergMarquardtStrategy strategy(options);
  double x_cost = 0, candidate_cost = 0, minimum_cost = 0, fixed_cost = 0;
  int iteration = 0, num_consecutive_invalid_steps = 0;
  auto finish = [&](int type) {
    out->termination = type;
    g->x = best_x;
    out->final_cost = out->initial_cost;
    for (double c : iteration_costs) out->final_cost = std::min(out->final_cost, c);
    out->initial_cost += fixed_cost;
    out->final_cost += fixed_cost;
    out->iterations = static_cast<int>(iteration_costs.size());
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - started).count();
  };
  if (!EvaluateGradientAndJacobian(*g, x, true, &s)) return finish(2);
  x_cost = s.lin.cost;
  fixed_cost = s.lin.fixed_cost;
  out->initial_cost = x_cost;
  minimum_cost = x_cost;
  iteration_costs.push_back(x_cost);
  Margin(s.gradient_max_norm, options.gradient_tolerance, &out->tolerance_margin);
  if (s.gradient_max_norm <= options.gradient_tolerance) return finish(0);
  TrustRegionStepEvaluator step_evaluator(x_cost, options.use_nonmonotonic_steps ? options.max_consecutive_nonmonotonic_steps : 0);
  bool last_step_successful = false;
  for (;;) {
    if (last_step_successful) {
      ++out->successful;
      if (x_cost < minimum_cost) minimum_cost = x_cost, best_x = x;
    } else if (iteration > 0) {
      ++out->unsuccessful;
    }
    if (iteration >= options.max_num_iterations) return finish(1);
    if (last_step_successful) {
      Margin(s.gradient_max_norm, options.gradient_tolerance, &out->tolerance_margin);
      if (s.gradient_max_norm <= options.gradient_tolerance) return finish(0);
    }
    if (strategy.Radius() <= options.min_trust_region_radius) return finish(0);
    ++iteration;
    last_step_successful = false;
    double model_cost_change = 0;
    const bool solved = ComputeStep(*g, s, solver, options, &strategy, &step, &model_cost_change);
    if (!solved || !(model_cost_change > 0.0)) {
      if (++num_consecutive_invalid_steps >= options.max_num_consecutive_invalid_steps) return finish(2);
      strategy.StepIsInvalid();
      iteration_costs.push_back(x_cost);
      out->steps.push_back(2);
      continue;
    }
    num_consecutive_invalid_steps = 0;
    for (int c = 0; c < g->num_eff; ++c) delta[c] = step[c] * s.scale[c];
    for (int p = g->submaps; p < g->S; ++p)
      if (g->column[p * 6 + 3] >= 0) {
        const double yaw_step = std::fabs(delta[g->column[p * 6 + 3]]);
        g->clamp_margin = std::min(g->clamp_margin, std::fabs(yaw_step - 0.5) / 0.5);
        g->clamped_steps += yaw_step > 0.5;
      }
    PlusAll(*g, x, delta, &candidate_x);
    if (!Cost(*g, candidate_x, &candidate_cost)) candidate_cost = std::numeric_limits<double>::max();
    double step_norm = 0;
    for (int p = 0; p < g->P(); ++p)
      for (int k = 0; k < 7; ++k)
        if ((k < 3 ? g->mask[p] & 7 : g->mask[p] & 56) != 0) step_norm += (x[7 * p + k] - candidate_x[7 * p + k]) * (x[7 * p + k] - candidate_x[7 * p + k]);
    step_norm = std::sqrt(step_norm);
    const double step_size_tolerance = options.parameter_tolerance * (s.x_norm + options.parameter_tolerance);
    Margin(step_norm, step_size_tolerance, &out->tolerance_margin);
    if (step_norm <= step_size_tolerance) return finish(0);
    const double cost_change = x_cost - candidate_cost;
    Margin(std::fabs(cost_change), options.function_tolerance * x_cost, &out->tolerance_margin);
    if (std::fabs(cost_change) <= options.function_tolerance * x_cost) return finish(0);
    const double relative_decrease = step_evaluator.StepQuality(candidate_cost, model_cost_change);
    Margin(relative_decrease, options.min_relative_decrease, &out->quality_margin);
    if (relative_decrease > options.min_relative_decrease) {
      x = candidate_x;
      if (candidate_cost > x_cost) ++out->rises;
      if (!EvaluateGradientAndJacobian(*g, x, false, &s)) return finish(2);
      x_cost = s.lin.cost;
      last_step_successful = true;
      strategy.StepAccepted(relative_decrease);
      step_evaluator.StepAccepted(candidate_cost, model_cost_change);
      iteration_costs.push_back(x_cost);
      out->steps.push_back(1);
    } else {
      strategy.StepRejected(relative_decrease);
      iteration_costs.push_back(candidate_cost);
      out->steps.push_back(0);
    }
  }
}

// ---- optimization_problem_3d_test.cc:106-191 (ReducesNoise) ----------------------------------------------------------------
struct Rigid {
  double t[3];
  Quat<double> q;
};
Quat<double> Normalized(const Quat<double>& q) {
  const double n = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  return Quat<double>{q.w / n, q.x / n, q.y / n, q.z / n};
}
Rigid Compose(const Rigid& a, const Rigid& b) {  // Rigid3d operator*
  Rigid r;
  Rotate(a.q, b.t, r.t);
  for (int k = 0; k < 3; ++k) r.t[k] += a.t[k];
  r.q = Normalized(Mul(a.q, b.q));
  return r;
}
Rigid Inverse(const Rigid& a) {
  Rigid r;
  r.q = Quat<double>{a.q.w, -a.q.x, -a.q.y, -a.q.z};
  Rotate(r.q, a.t, r.t);
  for (int k = 0; k < 3; ++k) r.t[k] = -r.t[k];
  return r;
}
Quat<double> AngleAxisVectorToRotationQuaternion(const double v[3]) {  // transform.h:85-99
  double scale = 0.5, w = 1.;
  const double squared = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  if (squared > 1e-8) {
    const double norm = std::sqrt(squared);
    scale = std::sin(norm / 2.) / norm;
    w = std::cos(norm / 2.);
  }
  return Quat<double>{w, scale * v[0], scale * v[1], scale * v[2]};
}
struct NoiseTest {
  std::mt19937 rng{45387};
  Rigid RandomTransform(double translation_size, double rotation_size) {
    std::uniform_real_distribution<double> translation_distribution(-translation_size, translation_size);
    const double x = translation_distribution(rng), y = translation_distribution(rng), z = translation_distribution(rng);
    std::uniform_real_distribution<double> rotation_distribution(-rotation_size, rotation_size);
    const double rx = rotation_distribution(rng), ry = rotation_distribution(rng), rz = rotation_distribution(rng);
    const double v[3] = {rx, ry, rz};
    return Rigid{{x, y, z}, AngleAxisVectorToRotationQuaternion(v)};
  }
  Rigid RandomYawOnlyTransform(double translation_size, double rotation_size) {
    std::uniform_real_distribution<double> translation_distribution(-translation_size, translation_size);
    const double x = translation_distribution(rng), y = translation_distribution(rng), z = translation_distribution(rng);
    std::uniform_real_distribution<double> rotation_distribution(-rotation_size, rotation_size);
    const double v[3] = {0., 0., rotation_distribution(rng)};
    return Rigid{{x, y, z}, AngleAxisVectorToRotationQuaternion(v)};
  }
};
Rigid AddNoise(const Rigid& transform, const Rigid& noise) {
  Rigid r;
  for (int k = 0; k < 3; ++k) r.t[k] = transform.t[k] + noise.t[k];
  r.q = Mul(noise.q, transform.q);
  return r;
}
void Put(const Rigid& r, double* out) {
  out[0] = r.t[0], out[1] = r.t[1], out[2] = r.t[2], out[3] = r.q.w, out[4] = r.q.x, out[5] = r.q.y, out[6] = r.q.z;
}

void WriteGraph(FILE* f, const Graph& g, const int32_t header_rest[4], double radius) {
  const int32_t head[5] = {g.S, g.N, static_cast<int32_t>(g.constraints.size()), g.gravity, g.fix_z};
  fwrite(head, 4, 5, f);
  fwrite(header_rest, 4, 4, f);
  fwrite(&radius, 8, 1, f);
  fwrite(g.x.data(), 8, g.x.size(), f);
  fwrite(g.constant.data(), 4, g.constant.size(), f);
  fwrite(g.constraints.data(), sizeof(Constraint), g.constraints.size(), f);
}

int ReducesNoise(const char* path) {
  constexpr int kNumNodes = 100;
  NoiseTest t;
  const double kPi = 3.14159265358979323846;
  const Rigid submap0{{0, 0, 0}, Quat<double>{1, 0, 0, 0}};
  const Rigid submap2{{0, 0, 0}, Quat<double>{std::cos(kPi / 2), 0, 0, std::sin(kPi / 2)}};  // Rigid3d::Rotation(AngleAxisd(M_PI, UnitZ))
  std::vector<Rigid> truth(kNumNodes), noise(kNumNodes);
  for (int j = 0; j != kNumNodes; ++j) {
    truth[j] = t.RandomTransform(10., 3.);
    noise[j] = t.RandomYawOnlyTransform(0.2, 0.3);
  }
  Graph g;
  g.S = 3;
  g.N = kNumNodes;
  g.gravity = 0;
  g.x.assign(7 * (3 + kNumNodes), 0.);
  g.constant.assign(3 + kNumNodes, 0);
  Put(submap0, &g.x[0]);
  Put(submap0, &g.x[7]);
  Put(submap2, &g.x[14]);
  for (int j = 0; j != kNumNodes; ++j) Put(AddNoise(truth[j], noise[j]), &g.x[7 * (3 + j)]);
  for (int j = 0; j != kNumNodes; ++j) {
    Constraint c;
    c.node = j;
    c.submap = 0;
    Put(AddNoise(truth[j], noise[j]), c.zbar);
    c.translation_weight = c.rotation_weight = 1.;
    g.constraints.push_back(c);
    c.submap = 1;
    Put(AddNoise(truth[j], t.RandomYawOnlyTransform(0.2, 0.3)), c.zbar);
    g.constraints.push_back(c);
    c.submap = 2;
    Put(Compose(Compose(Inverse(submap2), truth[j]), t.RandomTransform(1e3, 3.)), c.zbar);
    c.translation_weight = c.rotation_weight = 1e-9;
    g.constraints.push_back(c);
  }
  FILE* f = fopen(path, "wb");
  if (f == nullptr) return 2;
  const int32_t rest[4] = {0, 200, 0, 0};  // the test's options: monotonic, 200 iterations
  WriteGraph(f, g, rest, 1e4);
  std::vector<double> gt(7 * kNumNodes);
  for (int j = 0; j != kNumNodes; ++j) Put(truth[j], &gt[7 * j]);
  fwrite(gt.data(), 8, gt.size(), f);  // behind the graph: the ground truth poses
  fclose(f);
  return 0;
}

}  // namespace

// in: int32 S N C gravity fix_z nonmonotonic max_iterations mode solver F CF L O; double radius, huber_scale; poses
// (submaps, fixed frames, nodes); int32 constant[S + N]; constraints; fixed-frame constraints (.submap = the frame); int32
// inter_submap[C]; landmark poses; int32 landmark_constant[L]; observations (dliom_pose_graph_landmark_observation).
// mode 0 solve, 1 evaluate, 2 step.  out: the poses (7 a pose) and the slots (6 a pose) in the order submaps, fixed frames,
// nodes, landmarks and the residuals (6 a residual block) in the order constraints, fixed-frame constraints, observations.
//   solve: int32 termination, iterations, successful, unsuccessful, columns, steps, rises, clamped_steps; double
//     initial_cost, final_cost, quality_margin, tolerance_margin, seconds; int32 step[steps]; the poses; double
//     loss_margin, clamp_margin, slerp_margin
//   evaluate: int32 failed, columns; double cost; the residuals; the gradient's slots
//   step: int32 failed, columns; double model_cost_change; the step's slots; int32 blocks, and a remaining residual block
//     its int32 index, 6 residuals and its 6 x 6 Jacobian blocks (two, an observation's three); the scale's slots
int main(int argc, char** argv) {
  if (argc == 3 && std::strcmp(argv[1], "--reduces-noise") == 0) return ReducesNoise(argv[2]);
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (f == nullptr) return 2;
  int32_t head[13];
  double reals[2];
  Graph g;
  if (fread(head, 4, 13, f) != 13 || fread(reals, 8, 2, f) != 2) return 2;
  const double radius = reals[0];
  const int F = head[9], CF = head[10], C = head[2];
  g.submaps = head[0], g.S = head[0] + F, g.N = head[1], g.gravity = head[3], g.fix_z = head[4];
  g.huber_scale = reals[1];
  g.L = head[11];
  const int O = head[12];
  g.x.resize(7 * static_cast<size_t>(g.S + g.N + g.L));
  const size_t before_landmarks = 7 * static_cast<size_t>(g.S + g.N);
  std::vector<int32_t> landmark_constant(g.L);
  g.observations.resize(O);
  std::vector<int32_t> constant(g.submaps + g.N), inter_submap(C);
  g.constraints.resize(C + CF);
  if (fread(g.x.data(), 8, before_landmarks, f) != before_landmarks || fread(constant.data(), 4, constant.size(), f) != constant.size() ||
      fread(g.constraints.data(), sizeof(Constraint), g.constraints.size(), f) != g.constraints.size() ||
      fread(inter_submap.data(), 4, inter_submap.size(), f) != inter_submap.size() ||
      fread(g.x.data() + before_landmarks, 8, 7 * static_cast<size_t>(g.L), f) != 7 * static_cast<size_t>(g.L) ||
      fread(landmark_constant.data(), 4, landmark_constant.size(), f) != landmark_constant.size() ||
      fread(g.observations.data(), sizeof(Observation), g.observations.size(), f) != g.observations.size())
    return 2;
  fclose(f);
  g.constant.assign(g.S + g.N + g.L, 0);  // a fixed frame is never constant
  for (int l = 0; l < g.L; ++l) g.constant[g.S + g.N + l] = landmark_constant[l];
  for (int p = 0; p < g.submaps; ++p) g.constant[p] = constant[p];
  for (int p = 0; p < g.N; ++p) g.constant[g.S + p] = constant[g.submaps + p];
  g.lossy.assign(C + CF, 0);
  for (int c = 0; c < C; ++c) g.lossy[c] = inter_submap[c] != 0;
  for (int c = C; c < C + CF; ++c) g.constraints[c].submap += g.submaps;
  g.Derive();
  Options options;
  options.use_nonmonotonic_steps = head[5] != 0;
  options.max_num_iterations = head[6];
  const int mode = head[7], solver = head[8];
  FILE* o = fopen(argv[2], "wb");
  if (o == nullptr) return 2;
  auto put_d = [o](const double* v, size_t n) { fwrite(v, 8, n, o); };
  if (mode == 0) {
    Result r;
    Solve(options, solver, &g, &r);
    const int32_t ints[8] = {r.termination, r.iterations, r.successful, r.unsuccessful, g.num_eff, static_cast<int32_t>(r.steps.size()), r.rises, g.clamped_steps};
    fwrite(ints, 4, 8, o);
    const double d[5] = {r.initial_cost, r.final_cost, r.quality_margin, r.tolerance_margin, r.seconds};
    put_d(d, 5);
    std::vector<int32_t> steps(r.steps.begin(), r.steps.end());
    fwrite(steps.data(), 4, steps.size(), o);
    put_d(g.x.data(), g.x.size());
    const double margins[3] = {g.loss_margin, g.clamp_margin, g.slerp_margin};
    put_d(margins, 3);
  } else {
    State s;
    s.g = &g;
    const bool ok = EvaluateGradientAndJacobian(g, g.x, true, &s);
    std::vector<double> slots;
    if (mode == 1) {
      const int32_t ints[2] = {ok ? 0 : 1, g.num_eff};
      fwrite(ints, 4, 2, o);
      const double cost = s.lin.cost + s.lin.fixed_cost;
      put_d(&cost, 1);
      put_d(s.lin.all_residuals.data(), s.lin.all_residuals.size());
      SlotsFromColumns(g, s.gradient, &slots);
      put_d(slots.data(), slots.size());
    } else {
      options.initial_trust_region_radius = radius;
      LevenbergMarquardtStrategy strategy(options);
      std::vector<double> step;
      double model_cost_change = 0;
      // solver 3: the linearisation alone (no step)
      const bool solved = ok && solver != 3 && ComputeStep(g, s, solver, options, &strategy, &step, &model_cost_change);
      const int32_t ints[2] = {solved || (ok && solver == 3) ? 0 : 1, g.num_eff};
      fwrite(ints, 4, 2, o);
      put_d(&model_cost_change, 1);
      if (solved)
        for (int c = 0; c < g.num_eff; ++c) step[c] *= s.scale[c];
      else
        step.assign(g.num_eff, 0.);
      SlotsFromColumns(g, step, &slots);
      put_d(slots.data(), slots.size());
      // the sparse Jacobian on the unscaled columns: per remaining constraint its index, rows and two 6 x 6 blocks
      const int32_t blocks = static_cast<int32_t>(s.lin.blocks.size());
      fwrite(&blocks, 4, 1, o);
      for (const RowBlock& k : s.lin.blocks) {
        fwrite(&k.c, 4, 1, o);
        put_d(k.r, 6);
        for (int which = 0; which < k.num; ++which) put_d(k.j[which], 36);
      }
      SlotsFromColumns(g, s.scale, &slots);
      put_d(slots.data(), slots.size());
    }
  }
  fclose(o);
  return 0;
}
