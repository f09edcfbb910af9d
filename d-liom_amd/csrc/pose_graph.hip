// OptimizationProblem3D::Solve on the device (mapping/internal/optimization/optimization_problem_3d.cc:259-589 as this
// fork runs it: SpaCostFunction3D only, see include/dliom.h "pose graph optimisation"), with the fixed-frame pose
// constraints (:491-548) and upstream's HuberLoss on the inter-submap constraints (dliom_pose_graph_terms).
//
// Every constraint couples one kept pose -- a submap or a fixed frame -- with one node pose, so with the nodes eliminated
// (their Hessian is block-diagonal 6x6) a dense system over the kept blocks' columns is left.  One trust-region iteration
// is a chain of kernel launches -- stage boundaries are launches, nothing waits on another workgroup -- and ONE polled
// read-back:
//   linearise        per constraint: residual and tangent-space Jacobians by forward duals, corrected for the loss
//                    (pg_linearise_kernel);
//                    per pose: diagonal block, gradient, column scaling (pg_pose_kernel, pg_pose_values_kernel)
//   eliminate        per node: V = (H_nn + D^2)^-1 and the constraints' W V (pg_node_kernel); per block pair
//                    S_ab = [a == b](H_ss + D^2) - sum W V W^T over its sorted list (pg_pairs_kernel); right-hand side
//   factor           blocked right-looking Cholesky of S in FP64: panel on one workgroup, triangular solve and trailing
//                    update (v_mfma_f64_16x16x4_f64) chip-wide; up to kSmallDimension the whole factorisation and the
//                    solve are one workgroup's (pg_small_kernel); then the two triangular solves
//   back-substitute  per pose: the step and Plus into the candidate; per constraint: J y and the candidate's cost;
//                    pg_reduce_kernel sums everything in a fixed order into the page-locked block
// The trust-region loop itself (Ceres 1.13 trust_region_minimizer.cc, levenberg_marquardt_strategy.cc,
// trust_region_step_evaluator.cc -- third-party behaviour, restated for this configuration) runs on the host.
// No floating-point atomics: every accumulation is a segmented sum in the order pose_graph_structure.h fixes.
//
// Landmark observations (LandmarkCostFunction3D, dliom_pose_graph_landmarks) couple two nodes and a landmark.  Those
// nodes ("promoted") and the landmarks join the kept blocks; a residual block between kept blocks only -- a constraint of
// a promoted node, an observation -- never enters the node elimination: it adds J_a^T J_b to S_ab directly
// (pg_pairs_kernel, after the pair's elimination terms) and its J^T r reaches the right-hand side through the pose's
// gradient.  An observation is linearised per (observation, block) with six dual parts (pg_observation_linearise_kernel).
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "host_math.h"
#include "internal.h"
#include "pose_graph_structure.h"

namespace dliom {
namespace {

namespace pg = pose_graph;

constexpr int kPanel = 32;            // panel width of the factorisation; the system is padded to a multiple of it
constexpr int kSmallDimension = 256;  // padded dimensions up to this: one workgroup factorises and solves
constexpr int kSmallThreads = 1024;
constexpr int kSums = 8;              // doubles of an iteration's read-back
enum { kSumCost = 0, kSumFixedCost, kSumGradientMax, kSumXSquared, kSumModel, kSumCandidateCost, kSumStepSquared, kSumFlag };

// ---- forward duals (the arithmetic of ceres::Jet: a / b multiplies by 1 / b.a) ----------------------------------------
template <int N>
struct Dual {
  double a;
  double v[N > 0 ? N : 1];
};
template <int N>
__device__ inline Dual<N> constant(double a) {
  Dual<N> r;
  r.a = a;
  for (int i = 0; i < N; ++i) r.v[i] = 0.;
  return r;
}
template <int N>
__device__ inline Dual<N> operator+(const Dual<N>& f, const Dual<N>& g) {
  Dual<N> r;
  r.a = f.a + g.a;
  for (int i = 0; i < N; ++i) r.v[i] = f.v[i] + g.v[i];
  return r;
}
template <int N>
__device__ inline Dual<N> operator-(const Dual<N>& f, const Dual<N>& g) {
  Dual<N> r;
  r.a = f.a - g.a;
  for (int i = 0; i < N; ++i) r.v[i] = f.v[i] - g.v[i];
  return r;
}
template <int N>
__device__ inline Dual<N> operator-(const Dual<N>& f) {
  Dual<N> r;
  r.a = -f.a;
  for (int i = 0; i < N; ++i) r.v[i] = -f.v[i];
  return r;
}
template <int N>
__device__ inline Dual<N> operator*(const Dual<N>& f, const Dual<N>& g) {
  Dual<N> r;
  r.a = f.a * g.a;
  for (int i = 0; i < N; ++i) r.v[i] = f.a * g.v[i] + f.v[i] * g.a;
  return r;
}
template <int N>
__device__ inline Dual<N> operator*(const Dual<N>& f, double s) {
  Dual<N> r;
  r.a = f.a * s;
  for (int i = 0; i < N; ++i) r.v[i] = f.v[i] * s;
  return r;
}
template <int N>
__device__ inline Dual<N> operator/(const Dual<N>& f, const Dual<N>& g) {
  const double inverse = 1.0 / g.a;
  const double ratio = f.a * inverse;
  Dual<N> r;
  r.a = ratio;
  for (int i = 0; i < N; ++i) r.v[i] = (f.v[i] - ratio * g.v[i]) * inverse;
  return r;
}
template <int N>
__device__ inline Dual<N> dual_sqrt(const Dual<N>& f) {
  Dual<N> r;
  r.a = sqrt(f.a);
  const double scale = 1.0 / (2.0 * r.a);  // at 0: inf, and 0 * inf = NaN, which the cutoff branch below drops, as in Ceres
  for (int i = 0; i < N; ++i) r.v[i] = f.v[i] * scale;
  return r;
}
template <int N>
__device__ inline Dual<N> dual_atan2(const Dual<N>& g, const Dual<N>& f) {
  Dual<N> r;
  r.a = atan2(g.a, f.a);
  const double scale = 1.0 / (f.a * f.a + g.a * g.a);
  for (int i = 0; i < N; ++i) r.v[i] = scale * (f.a * g.v[i] - g.a * f.v[i]);
  return r;
}
template <int N>
__device__ inline Dual<N> dual_sin(const Dual<N>& f) {
  Dual<N> r;
  r.a = sin(f.a);
  const double c = cos(f.a);
  for (int i = 0; i < N; ++i) r.v[i] = c * f.v[i];
  return r;
}
template <int N>
__device__ inline Dual<N> dual_acos(const Dual<N>& f) {
  Dual<N> r;
  r.a = acos(f.a);
  const double scale = -1.0 / sqrt(1.0 - f.a * f.a);
  for (int i = 0; i < N; ++i) r.v[i] = scale * f.v[i];
  return r;
}

// a * b of Eigen::Quaternion (w x y z)
template <int N>
__device__ inline void quaternion_product(const Dual<N> a[4], const Dual<N> b[4], Dual<N> out[4]) {
  out[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  out[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  out[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
  out[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}

// SpaCostFunction3D (spa_cost_function_3d.h:46-56): ScaleError(ComputeUnscaledError(...)) of cost_helpers_impl.h:57-101
// with transform.h:59-81.  i: the submap (start), j: the node (end).
template <int N>
__device__ inline void spa_residual(const Dual<N> qi[4], const Dual<N> ti[3], const Dual<N> qj[4], const Dual<N> tj[3],
                                    const double* zbar, double translation_weight, double rotation_weight, Dual<N> e[6]) {
  using D = Dual<N>;
  const D delta[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]};
  // R_i^-1 * delta as Eigen rotates a vector: uv = 2 vec x v; v + w uv + vec x uv
  const D w = qi[0];
  const D vec[3] = {-qi[1], -qi[2], -qi[3]};
  D uv[3] = {vec[1] * delta[2] - vec[2] * delta[1], vec[2] * delta[0] - vec[0] * delta[2], vec[0] * delta[1] - vec[1] * delta[0]};
  for (int k = 0; k < 3; ++k) uv[k] = uv[k] + uv[k];
  const D h[3] = {delta[0] + w * uv[0] + (vec[1] * uv[2] - vec[2] * uv[1]), delta[1] + w * uv[1] + (vec[2] * uv[0] - vec[0] * uv[2]),
                  delta[2] + w * uv[2] + (vec[0] * uv[1] - vec[1] * uv[0])};
  const D qj_inverse[4] = {qj[0], -qj[1], -qj[2], -qj[3]};
  D h_rotation_inverse[4], product[4];
  quaternion_product(qj_inverse, qi, h_rotation_inverse);
  const D z[4] = {constant<N>(zbar[3]), constant<N>(zbar[4]), constant<N>(zbar[5]), constant<N>(zbar[6])};
  quaternion_product(h_rotation_inverse, z, product);
  // RotationQuaternionToAngleAxisVector
  const D squared = product[1] * product[1] + product[2] * product[2] + product[3] * product[3] + product[0] * product[0];
  if (squared.a > 0.) {
    const D norm = dual_sqrt(squared);
    for (int k = 0; k < 4; ++k) product[k] = product[k] / norm;
  }
  if (product[0].a < 0.)
    for (int k = 0; k < 4; ++k) product[k] = product[k] * -1.;
  const D vec_norm = dual_sqrt(product[1] * product[1] + product[2] * product[2] + product[3] * product[3]);
  const D angle = dual_atan2(vec_norm, product[0]) * 2.;
  const D scale = angle.a < 1e-7 ? constant<N>(2.) : angle / dual_sin(angle * (1. / 2.));
  for (int k = 0; k < 3; ++k) {
    e[k] = (constant<N>(zbar[k]) - h[k]) * translation_weight;
    e[3 + k] = (scale * product[1 + k]) * rotation_weight;
  }
}

// InterpolateNodes3D (cost_helpers_impl.h:103-153): SlerpQuaternions as written there -- the dot product in its order, the
// linear scales from |cos theta| >= 1 - 1e-5 on, next_scale negated for cos theta < 0, no renormalisation -- and the
// translation prev + t (next - prev).
template <int N>
__device__ inline void interpolate_nodes(const Dual<N> prev_q[4], const Dual<N> prev_t[3], const Dual<N> next_q[4],
                                         const Dual<N> next_t[3], double t, Dual<N> q[4], Dual<N> translation[3]) {
  using D = Dual<N>;
  const D cos_theta = prev_q[0] * next_q[0] + prev_q[1] * next_q[1] + prev_q[2] * next_q[2] + prev_q[3] * next_q[3];
  const D abs_cos_theta = cos_theta.a < 0. ? -cos_theta : cos_theta;
  D prev_scale = constant<N>(1. - t), next_scale = constant<N>(t);
  if (abs_cos_theta.a < 1. - 1e-5) {
    const D theta = dual_acos(abs_cos_theta);
    const D sin_theta = dual_sin(theta);
    prev_scale = dual_sin(theta * (1. - t)) / sin_theta;
    next_scale = dual_sin(theta * t) / sin_theta;
  }
  if (cos_theta.a < 0.) next_scale = -next_scale;
  for (int k = 0; k < 4; ++k) q[k] = prev_scale * prev_q[k] + next_scale * next_q[k];
  for (int k = 0; k < 3; ++k) translation[k] = prev_t[k] + (next_t[k] - prev_t[k]) * t;
}

// ---- local parameterisations ------------------------------------------------------------------------------------------
// d Plus / d delta at 0 of the rotation block, 4 x 3 row-major: QuaternionParameterization (ceres/local_parameterization.cc)
// or, gravity-aligned, the two columns of ConstantYawQuaternionPlus (rotation_parameterization.h:41-62: x (x) [1, d0, d1, 0]
// to first order; its 1e-6 branch makes the autodiff Jacobian exactly that), or, for a fixed frame, the one column of
// YawOnlyQuaternionPlus (:27-39: [sqrt(1 - d^2), 0, 0, d] (x) x; the square root's derivative vanishes at 0)
__device__ inline void plus_jacobian(const double* q, int kind, double* j) {
  if (kind == pg::kKindYawOnly) {
    j[0] = -q[3]; j[1] = 0.; j[2] = 0.;
    j[3] = -q[2]; j[4] = 0.; j[5] = 0.;
    j[6] = q[1];  j[7] = 0.; j[8] = 0.;
    j[9] = q[0];  j[10] = 0.; j[11] = 0.;
  } else if (kind == pg::kKindConstantYaw) {
    j[0] = -q[1]; j[1] = -q[2]; j[2] = 0.;
    j[3] = q[0];  j[4] = -q[3]; j[5] = 0.;
    j[6] = q[3];  j[7] = q[0];  j[8] = 0.;
    j[9] = -q[2]; j[10] = q[1]; j[11] = 0.;
  } else {
    j[0] = -q[1]; j[1] = -q[2]; j[2] = -q[3];
    j[3] = q[0];  j[4] = q[3];  j[5] = -q[2];
    j[6] = -q[3]; j[7] = q[0];  j[8] = q[1];
    j[9] = q[2];  j[10] = -q[1]; j[11] = q[0];
  }
}
__device__ inline void hamilton(const double* z, const double* w, double* zw) {  // ceres/rotation.h QuaternionProduct
  zw[0] = z[0] * w[0] - z[1] * w[1] - z[2] * w[2] - z[3] * w[3];
  zw[1] = z[0] * w[1] + z[1] * w[0] + z[2] * w[3] - z[3] * w[2];
  zw[2] = z[0] * w[2] - z[1] * w[3] + z[2] * w[0] + z[3] * w[1];
  zw[3] = z[0] * w[3] + z[1] * w[2] - z[2] * w[1] + z[3] * w[0];
}
// Plus of a pose's blocks on the slots of `mask`; a block outside the problem keeps its bits.
__device__ inline void pose_plus(const double* x, const double* delta, int mask, int kind, double* out) {
  for (int k = 0; k < 3; ++k) out[k] = (mask >> k) & 1 ? x[k] + delta[k] : x[k];
  for (int k = 3; k < 7; ++k) out[k] = x[k];
  if ((mask & 56) == 0) return;
  double q_delta[4];
  if (kind == pg::kKindYawOnly) {
    const double clamped = delta[3] > 0.5 ? 0.5 : (delta[3] < -0.5 ? -0.5 : delta[3]);  // common::Clamp
    q_delta[0] = sqrt(1. - clamped * clamped);
    q_delta[1] = 0.;
    q_delta[2] = 0.;
    q_delta[3] = clamped;
    hamilton(q_delta, x + 3, out + 3);
  } else if (kind == pg::kKindConstantYaw) {
    const double norm = sqrt(delta[3] * delta[3] + delta[4] * delta[4]);
    const double sin_over = norm < 1e-6 ? 1. : sin(norm) / norm;
    q_delta[0] = norm < 1e-6 ? 1. : cos(norm);
    q_delta[1] = sin_over * delta[3];
    q_delta[2] = sin_over * delta[4];
    q_delta[3] = 0.;
    hamilton(x + 3, q_delta, out + 3);
  } else {
    const double norm = sqrt(delta[3] * delta[3] + delta[4] * delta[4] + delta[5] * delta[5]);
    if (norm > 0.) {
      const double sin_over = sin(norm) / norm;
      q_delta[0] = cos(norm);
      q_delta[1] = sin_over * delta[3];
      q_delta[2] = sin_over * delta[4];
      q_delta[3] = sin_over * delta[5];
      hamilton(q_delta, x + 3, out + 3);
    }
  }
}

// ---- the loss ----------------------------------------------------------------------------------------------------------
// ceres::HuberLoss(a) at s = ||r||^2 (loss_function.cc) with Corrector (corrector.cc) for rho'' <= 0, where it is a pure
// scaling of residual and Jacobian by sqrt(rho'): returns rho and sets *scaling.  Inside the quadratic region rho = s and
// the scaling is exactly 1, as under TrivialLoss.
__device__ inline double huber(double a, double s, double* scaling) {
  const double b = a * a;
  *scaling = 1.;
  if (!(s > b)) return s;
  const double r = sqrt(s);
  *scaling = sqrt(fmax(DBL_MIN, a / r));
  return 2. * a * r - b;
}

// ---- what the kernels share --------------------------------------------------------------------------------------------
struct Graph {
  // kept blocks: the submaps, then the fixed frames; constraints: the submaps', then the fixed frames'
  int num_kept, num_nodes, num_constraints, num_pairs;
  int n, np;  // reduced dimension and its padded size (the leading dimension of S)
  double huber_scale;  // 0: TrivialLoss everywhere
  // structure (one packed upload)
  const double* constraint_data;  // 9 a constraint: zbar, translation weight, rotation weight
  const int *constraint_submap, *constraint_node, *mask, *column, *fixed, *pose_start, *pose_constraints;
  const int* kind;   // per kept block: its rotation's parameterisation (pg::kKind*)
  const int* lossy;  // per constraint: non-zero = under HuberLoss(huber_scale); null when huber_scale is 0
  const int *pair_a, *pair_b, *pair_start, *pair_c, *pair_c2;
  // state
  double *x, *candidate;                  // 7 a pose: kept blocks, then nodes
  double *scale, *diagonal_block, *gradient;  // 6, 36, 6 a pose (unscaled)
  double *residual, *jacobian;            // 6, 72 a constraint ([6 x 6 submap | 6 x 6 node], unscaled, masked)
  double *cross, *cross_v, *cross_vg;     // 36, 36, 6 a constraint: E = Js^T Jn (scaled), E V, E V g_n
  double *v, *vg;                         // 36, 6 a node
  double *s, *rhs;                        // np x np row-major lower, np
  double *step, *delta;                   // 6 a pose: scaled step, and step * scale
  double *model, *cost, *candidate_cost;  // a constraint
  double *step_squared, *x_squared, *gradient_max;  // a pose
  unsigned* flag;                         // non-zero: a non-positive pivot; later stages return at once
  // Landmarks: the poses are the kept blocks, the nodes, then the landmarks; `column` then has 6 entries a pose.  The
  // observations' Jacobian blocks (three 6 x 6 an observation: prev, next, landmark), residuals, costs and models lie
  // behind the constraints' in `jacobian`, `residual`, `cost`, `model` and `candidate_cost`.
  int num_landmarks, num_observations;
  const double* observation_data;  // 10 an observation: landmark_to_tracking, the two weights, t
  const int *observation_pose;     // 3 an observation: the poses of prev, next and the landmark
  const int *observation_fixed, *node_promoted;  // node_promoted is null without landmarks
  const int *pose_observation_start, *pose_observations, *pair_direct_start, *pair_direct_a, *pair_direct_b;
};

__device__ inline int kind_of(const Graph& g, int p) { return p < g.num_kept ? g.kind[p] : pg::kKindQuaternion; }
__device__ inline int pose_count(const Graph& g) { return g.num_kept + g.num_nodes + g.num_landmarks; }
// a block of the reduced system: a submap, a fixed frame, a promoted node or a landmark
__device__ inline bool is_kept(const Graph& g, int p) {
  return p < g.num_kept || (g.node_promoted != nullptr && (p >= g.num_kept + g.num_nodes || g.node_promoted[p - g.num_kept] != 0));
}
// 1/2 rho(s) of constraint c and the corrector's scaling
__device__ inline double constraint_cost(const Graph& g, int c, double squared, double* scaling) {
  *scaling = 1.;
  if (g.huber_scale > 0. && g.lossy[c] != 0) return 0.5 * huber(g.huber_scale, squared, scaling);
  return 0.5 * squared;
}

template <int N>
__device__ inline void evaluate_constraint(const Graph& g, const double* poses, int c, Dual<N> e[6]) {
  const int a = g.constraint_submap[c], n = g.num_kept + g.constraint_node[c];
  const double* xa = poses + 7 * a;
  const double* xn = poses + 7 * n;
  Dual<N> ti[3], qi[4], tj[3], qj[4];
  for (int k = 0; k < 3; ++k) ti[k] = constant<N>(xa[k]), tj[k] = constant<N>(xn[k]);
  for (int k = 0; k < 4; ++k) qi[k] = constant<N>(xa[3 + k]), qj[k] = constant<N>(xn[3 + k]);
  if constexpr (N == 12) {
    // seeded with the tangent directions: the duals' parts are the tangent-space Jacobian's columns
    const int ma = g.mask[a], mn = g.mask[n];
    double ja[12], jn[12];
    plus_jacobian(xa + 3, g.kind[a], ja);
    plus_jacobian(xn + 3, pg::kKindQuaternion, jn);
    for (int k = 0; k < 3; ++k) {
      if ((ma >> k) & 1) ti[k].v[k] = 1.;
      if ((mn >> k) & 1) tj[k].v[6 + k] = 1.;
    }
    for (int k = 0; k < 4; ++k)
      for (int col = 0; col < 3; ++col) {
        if ((ma >> (3 + col)) & 1) qi[k].v[3 + col] = ja[k * 3 + col];
        if ((mn >> (3 + col)) & 1) qj[k].v[9 + col] = jn[k * 3 + col];
      }
  }
  const double* data = g.constraint_data + 9 * static_cast<int64_t>(c);
  spa_residual<N>(qi, ti, qj, tj, data, data[7], data[8], e);
}

__global__ void __launch_bounds__(64) pg_linearise_kernel(Graph g) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g.num_constraints) return;
  Dual<12> e[6];
  evaluate_constraint<12>(g, g.x, c, e);
  double squared = 0., scaling;
  for (int k = 0; k < 6; ++k) squared += e[k].a * e[k].a;
  g.cost[c] = constraint_cost(g, c, squared, &scaling);
  // the corrected residual and Jacobian (a scaling of exactly 1 leaves the bits alone)
  for (int k = 0; k < 6; ++k) {
    g.residual[6 * static_cast<int64_t>(c) + k] = e[k].a * scaling;
    double* row = g.jacobian + 72 * static_cast<int64_t>(c);
    for (int i = 0; i < 6; ++i) {
      row[k * 6 + i] = e[k].v[i] * scaling;
      row[36 + k * 6 + i] = e[k].v[6 + i] * scaling;
    }
  }
}

// LandmarkCostFunction3D (landmark_cost_function_3d.h:55-75): SpaCostFunction3D's error between the interpolated node pose
// (start) and the landmark (end).  N == 6: seeded with the tangent directions of block `seeded` (0 prev, 1 next, 2 the
// landmark), so that the duals' parts are that block's tangent-space Jacobian; the scalar parts do not depend on it.
template <int N>
__device__ inline void evaluate_observation(const Graph& g, const double* poses, int o, int seeded, Dual<N> e[6]) {
  Dual<N> t[3][3], q[3][4];
  for (int block = 0; block < 3; ++block) {
    const int p = g.observation_pose[3 * o + block];
    const double* x = poses + 7 * static_cast<int64_t>(p);
    for (int k = 0; k < 3; ++k) t[block][k] = constant<N>(x[k]);
    for (int k = 0; k < 4; ++k) q[block][k] = constant<N>(x[3 + k]);
    if constexpr (N == 6) {
      if (block != seeded) continue;
      const int mask = g.mask[p];
      double j[12];
      plus_jacobian(x + 3, pg::kKindQuaternion, j);
      for (int k = 0; k < 3; ++k)
        if ((mask >> k) & 1) t[block][k].v[k] = 1.;
      for (int k = 0; k < 4; ++k)
        for (int col = 0; col < 3; ++col)
          if ((mask >> (3 + col)) & 1) q[block][k].v[3 + col] = j[k * 3 + col];
    }
  }
  const double* data = g.observation_data + 10 * static_cast<int64_t>(o);
  Dual<N> interpolated_q[4], interpolated_t[3];
  interpolate_nodes<N>(q[0], t[0], q[1], t[1], data[9], interpolated_q, interpolated_t);
  spa_residual<N>(interpolated_q, interpolated_t, q[2], t[2], data, data[7], data[8], e);
}

// One thread an (observation, block): the block's 6 x 6 Jacobian; the prev block's thread also writes the residual and the
// cost (no loss on an observation).
__global__ void __launch_bounds__(64) pg_observation_linearise_kernel(Graph g) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * g.num_observations) return;
  const int o = t / 3, block = t % 3;
  Dual<6> e[6];
  evaluate_observation<6>(g, g.x, o, block, e);
  double* jac = g.jacobian + 72 * static_cast<int64_t>(g.num_constraints) + 36 * static_cast<int64_t>(t);
  for (int k = 0; k < 6; ++k)
    for (int i = 0; i < 6; ++i) jac[k * 6 + i] = e[k].v[i];
  if (block != 0) return;
  double squared = 0.;
  for (int k = 0; k < 6; ++k) {
    squared += e[k].a * e[k].a;
    g.residual[6 * (static_cast<int64_t>(g.num_constraints) + o) + k] = e[k].a;
  }
  g.cost[g.num_constraints + o] = 0.5 * squared;
}

// One wavefront a pose: lanes 0..35 the diagonal block J^T J, lanes 36..41 the gradient J^T r, over the pose's
// constraints in their fixed order.  set_scale: the iteration-0 column scaling 1 / (1 + ||J_col||).
__global__ void __launch_bounds__(256) pg_pose_kernel(Graph g, int set_scale) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (p >= pose_count(g) || lane >= 42) return;
  const int side = p < g.num_kept ? 0 : 36;
  const int i = lane < 36 ? lane / 6 : lane - 36, j = lane < 36 ? lane % 6 : 0;
  double sum = 0.;
  for (int at = g.pose_start[p]; at < g.pose_start[p + 1]; ++at) {
    const int64_t c = g.pose_constraints[at];
    const double* jac = g.jacobian + 72 * c + side;
    if (lane < 36) {
      for (int k = 0; k < 6; ++k) sum += jac[k * 6 + i] * jac[k * 6 + j];
    } else {
      for (int k = 0; k < 6; ++k) sum += jac[k * 6 + i] * g.residual[6 * c + k];
    }
  }
  if (g.num_observations > 0) {  // the observations follow the constraints in the residual blocks' order
    for (int at = g.pose_observation_start[p]; at < g.pose_observation_start[p + 1]; ++at) {
      const int64_t entry = g.pose_observations[at];
      const double* jac = g.jacobian + 72 * static_cast<int64_t>(g.num_constraints) + 36 * entry;
      const double* residual = g.residual + 6 * (g.num_constraints + entry / 3);
      if (lane < 36) {
        for (int k = 0; k < 6; ++k) sum += jac[k * 6 + i] * jac[k * 6 + j];
      } else {
        for (int k = 0; k < 6; ++k) sum += jac[k * 6 + i] * residual[k];
      }
    }
  }
  if (lane < 36) {
    g.diagonal_block[36 * static_cast<int64_t>(p) + lane] = sum;
    if (set_scale && i == j) g.scale[6 * static_cast<int64_t>(p) + i] = 1.0 / (1.0 + sqrt(sum));
  } else {
    g.gradient[6 * static_cast<int64_t>(p) + i] = sum;
  }
}

// Per pose: max |Plus(x, -gradient) - x| and ||x||^2 over the blocks in the problem.
__global__ void pg_pose_values_kernel(Graph g) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pose_count(g)) return;
  const int mask = g.mask[p];
  const double* x = g.x + 7 * static_cast<int64_t>(p);
  double negative[6], projected[7];
  for (int k = 0; k < 6; ++k) negative[k] = -g.gradient[6 * static_cast<int64_t>(p) + k];
  pose_plus(x, negative, mask, kind_of(g, p), projected);
  double most = 0., squared = 0.;
  if (mask & 7)
    for (int k = 0; k < 3; ++k) most = fmax(most, fabs(x[k] - projected[k])), squared += x[k] * x[k];
  if (mask & 56)
    for (int k = 3; k < 7; ++k) most = fmax(most, fabs(x[k] - projected[k])), squared += x[k] * x[k];
  g.gradient_max[p] = most;
  g.x_squared[p] = squared;
}

// levenberg_marquardt_strategy.cc: D^2 = clamp(diag(J^T J), 1e-6, 1e32) / radius on the scaled columns
__device__ inline double lm_diagonal(double scaled_diagonal, double radius) {
  return fmin(fmax(scaled_diagonal, 1e-6), 1e32) / radius;
}

// Per node: V = (H_nn + D_n^2)^-1 by a 6 x 6 Cholesky (slots outside the problem: identity rows), V g_n, and for each of
// its constraints E = Js^T Jn on the scaled columns, E V and E V g_n.
__global__ void __launch_bounds__(64) pg_node_kernel(Graph g, double radius) {
  const int node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= g.num_nodes) return;
  const int p = g.num_kept + node;
  if (g.node_promoted != nullptr && g.node_promoted[node] != 0) {
    // a kept block: nothing of it is eliminated, and its constraints' elimination terms read as zero
    for (int at = g.pose_start[p]; at < g.pose_start[p + 1]; ++at) {
      const int64_t c = g.pose_constraints[at];
      for (int k = 0; k < 36; ++k) g.cross[36 * c + k] = 0., g.cross_v[36 * c + k] = 0.;
      for (int k = 0; k < 6; ++k) g.cross_vg[6 * c + k] = 0.;
    }
    return;
  }
  const int mask = g.mask[p];
  double v[36], vg[6], sn[6];
  for (int k = 0; k < 36; ++k) v[k] = 0.;
  for (int k = 0; k < 6; ++k) vg[k] = 0., sn[k] = g.scale[6 * static_cast<int64_t>(p) + k];
  if (mask != 0) {
    double l[36];
    const double* h = g.diagonal_block + 36 * static_cast<int64_t>(p);
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) {
        const bool in = ((mask >> i) & 1) && ((mask >> j) & 1);
        double value = in ? sn[i] * sn[j] * h[i * 6 + j] : (i == j ? 1. : 0.);
        if (in && i == j) value += lm_diagonal(value, radius);
        l[i * 6 + j] = value;
      }
    bool ok = true;
    for (int j = 0; j < 6; ++j) {
      double d = l[j * 6 + j];
      for (int k = 0; k < j; ++k) d -= l[j * 6 + k] * l[j * 6 + k];
      if (!(d > 0.)) {
        ok = false;
        d = 1.;
      }
      d = sqrt(d);
      l[j * 6 + j] = d;
      for (int i = j + 1; i < 6; ++i) {
        double t = l[i * 6 + j];
        for (int k = 0; k < j; ++k) t -= l[i * 6 + k] * l[j * 6 + k];
        l[i * 6 + j] = t / d;
      }
    }
    if (!ok) *g.flag = 1u;
    // V = L^-T L^-1, column by column
    for (int col = 0; col < 6; ++col) {
      double z[6];
      for (int i = 0; i < 6; ++i) {
        double t = i == col ? 1. : 0.;
        for (int k = 0; k < i; ++k) t -= l[i * 6 + k] * z[k];
        z[i] = t / l[i * 6 + i];
      }
      for (int i = 5; i >= 0; --i) {
        double t = z[i];
        for (int k = i + 1; k < 6; ++k) t -= l[k * 6 + i] * z[k];
        z[i] = t / l[i * 6 + i];
      }
      for (int i = 0; i < 6; ++i) v[i * 6 + col] = ((mask >> i) & 1) && ((mask >> col) & 1) ? z[i] : 0.;
    }
    for (int i = 0; i < 6; ++i) {
      double t = 0.;
      for (int k = 0; k < 6; ++k) t += v[i * 6 + k] * (sn[k] * g.gradient[6 * static_cast<int64_t>(p) + k]);
      vg[i] = t;
    }
  }
  for (int k = 0; k < 36; ++k) g.v[36 * static_cast<int64_t>(node) + k] = v[k];
  for (int k = 0; k < 6; ++k) g.vg[6 * static_cast<int64_t>(node) + k] = vg[k];
  for (int at = g.pose_start[p]; at < g.pose_start[p + 1]; ++at) {
    const int64_t c = g.pose_constraints[at];
    const int a = g.constraint_submap[c];
    const double* jac = g.jacobian + 72 * c;
    double e[36];
    for (int i = 0; i < 6; ++i) {
      const double sa = g.scale[6 * static_cast<int64_t>(a) + i];
      for (int k = 0; k < 6; ++k) {
        double t = 0.;
        for (int m = 0; m < 6; ++m) t += jac[m * 6 + i] * jac[36 + m * 6 + k];
        e[i * 6 + k] = sa * sn[k] * t;
      }
    }
    for (int i = 0; i < 6; ++i) {
      double t = 0.;
      for (int k = 0; k < 6; ++k) {
        double f = 0.;
        for (int m = 0; m < 6; ++m) f += e[i * 6 + m] * v[m * 6 + k];
        g.cross_v[36 * c + i * 6 + k] = f;
        g.cross[36 * c + i * 6 + k] = e[i * 6 + k];
        t += e[i * 6 + k] * vg[k];
      }
      g.cross_vg[6 * c + i] = t;
    }
  }
}

// One wavefront a block pair (a >= b): lane (i, j) of 36 runs over the pair's sorted list.
__global__ void __launch_bounds__(256) pg_pairs_kernel(Graph g, double radius) {
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pair >= g.num_pairs || lane >= 36) return;
  const int a = g.pair_a[pair], b = g.pair_b[pair];
  const int i = lane / 6, j = lane % 6;
  const int row = g.column[a * 6 + i], col = g.column[b * 6 + j];
  if (row < 0 || col < 0 || col > row) return;
  double sum = 0.;
  for (int at = g.pair_start[pair]; at < g.pair_start[pair + 1]; ++at) {
    const double* f = g.cross_v + 36 * static_cast<int64_t>(g.pair_c[at]) + i * 6;
    const double* e = g.cross + 36 * static_cast<int64_t>(g.pair_c2[at]) + j * 6;
    for (int k = 0; k < 6; ++k) sum += f[k] * e[k];
  }
  double value = 0.;
  if (a == b) {
    const double* scale = g.scale + 6 * static_cast<int64_t>(a);
    value = scale[i] * scale[j] * g.diagonal_block[36 * static_cast<int64_t>(a) + lane];
    if (i == j) value += lm_diagonal(value, radius);
  }
  value -= sum;
  if (g.pair_direct_start != nullptr) {
    double direct = 0.;
    for (int at = g.pair_direct_start[pair]; at < g.pair_direct_start[pair + 1]; ++at) {
      const double* ja = g.jacobian + 36 * static_cast<int64_t>(g.pair_direct_a[at]) + i;
      const double* jb = g.jacobian + 36 * static_cast<int64_t>(g.pair_direct_b[at]) + j;
      for (int k = 0; k < 6; ++k) direct += ja[k * 6] * jb[k * 6];
    }
    value += g.scale[6 * static_cast<int64_t>(a) + i] * g.scale[6 * static_cast<int64_t>(b) + j] * direct;
  }
  g.s[static_cast<int64_t>(row) * g.np + col] = value;
}

// Zeroes the lower triangle of S (its diagonal tiles whole) in kPanel x kPanel tiles, grid (tiles, tiles): block pairs that
// are in no list stay zero, and nothing ever reads above the diagonal tiles.
__global__ void __launch_bounds__(256) pg_zero_lower_kernel(Graph g) {
  if (blockIdx.x > blockIdx.y) return;
  for (int e = threadIdx.x; e < kPanel * kPanel; e += blockDim.x)
    g.s[static_cast<int64_t>(blockIdx.y * kPanel + e / kPanel) * g.np + blockIdx.x * kPanel + e % kPanel] = 0.;
}

// Right-hand side -(g_s - sum E V g_n) on the scaled columns, the padding's unit diagonal.
__global__ void pg_rhs_kernel(Graph g) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < g.np - g.n) g.s[static_cast<int64_t>(g.n + t) * g.np + g.n + t] = 1.;
  if (t >= (g.node_promoted != nullptr ? pose_count(g) : g.num_kept) * 6) return;
  const int a = t / 6, i = t % 6;
  const int row = g.column[t];
  if (row < 0) return;
  double sum = 0.;
  for (int at = g.pose_start[a]; at < g.pose_start[a + 1]; ++at) sum += g.cross_vg[6 * static_cast<int64_t>(g.pose_constraints[at]) + i];
  g.rhs[row] = -(g.scale[t] * g.gradient[t] - sum);
}

// ---- the factorisation ---------------------------------------------------------------------------------------------------
// The diagonal block at k0 in LDS (kPanel x (kPanel + 1)), by every thread of the workgroup.
__device__ inline void panel_block(double* s, int ld, int k0, double* tile, unsigned* flag) {
  const int tid = threadIdx.x, threads = blockDim.x;
  for (int e = tid; e < kPanel * kPanel; e += threads) {
    const int i = e / kPanel, j = e % kPanel;
    tile[i * (kPanel + 1) + j] = j <= i ? s[static_cast<int64_t>(k0 + i) * ld + k0 + j] : 0.;
  }
  __syncthreads();
  for (int j = 0; j < kPanel; ++j) {
    const double d = tile[j * (kPanel + 1) + j];
    __syncthreads();
    if (!(d > 0.)) {  // the same for every thread: they leave together
      if (tid == 0) *flag = 1u;
      return;
    }
    const double root = sqrt(d);
    if (tid == 0) tile[j * (kPanel + 1) + j] = root;
    if (tid > j && tid < kPanel) tile[tid * (kPanel + 1) + j] /= root;
    __syncthreads();
    for (int e = tid; e < kPanel * kPanel; e += threads) {
      const int i = e / kPanel, k = e % kPanel;
      if (k > j && k <= i) tile[i * (kPanel + 1) + k] -= tile[i * (kPanel + 1) + j] * tile[k * (kPanel + 1) + j];
    }
    __syncthreads();
  }
  for (int e = tid; e < kPanel * kPanel; e += threads) {
    const int i = e / kPanel, j = e % kPanel;
    if (j <= i) s[static_cast<int64_t>(k0 + i) * ld + k0 + j] = tile[i * (kPanel + 1) + j];
  }
}
// Row `row` (below the panel) of L21 = A21 L11^-T; L11 is `tile`.
__device__ inline void trsm_row(double* s, int ld, int k0, int row, const double* tile) {
  double* a = s + static_cast<int64_t>(row) * ld + k0;
  double x[kPanel];
  for (int j = 0; j < kPanel; ++j) x[j] = a[j];
#pragma unroll
  for (int j = 0; j < kPanel; ++j) {
    double t = x[j];
#pragma unroll
    for (int k = 0; k < j; ++k) t -= x[k] * tile[j * (kPanel + 1) + k];
    x[j] = t / tile[j * (kPanel + 1) + j];
  }
  for (int j = 0; j < kPanel; ++j) a[j] = x[j];
}
// The 16 x 16 tile at (row0, col0) of the trailing matrix minus L21 L21^T, by one wavefront: eight
// v_mfma_f64_16x16x4_f64 (A / B: lane & 15 the row / column, lane >> 4 the k; C / D: column lane & 15, row
// (lane >> 4) + 4 * register).
__device__ inline void update_tile(double* s, int ld, int k0, int row0, int col0, int lane) {
  typedef double double4_t __attribute__((ext_vector_type(4)));
  const int m = lane & 15, k = lane >> 4;
  const double* a = s + static_cast<int64_t>(row0 + m) * ld + k0 + k;
  const double* b = s + static_cast<int64_t>(col0 + m) * ld + k0 + k;
  double* c = s + static_cast<int64_t>(row0 + k) * ld + col0 + m;
  double4_t acc;
  for (int r = 0; r < 4; ++r) acc[r] = c[static_cast<int64_t>(4 * r) * ld];
#pragma unroll
  for (int kk = 0; kk < kPanel / 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[4 * kk], b[4 * kk], acc, 0, 0, 0);
  for (int r = 0; r < 4; ++r) c[static_cast<int64_t>(4 * r) * ld] = acc[r];
}
// Forward and backward substitution with the factor, in blocks of kPanel, by every thread of the workgroup.
__device__ inline void triangular_solves(const double* s, int ld, int np, double* rhs, double* tile, double* x) {
  const int tid = threadIdx.x, threads = blockDim.x;
  for (int k0 = 0; k0 < np; k0 += kPanel) {
    for (int e = tid; e < kPanel * kPanel; e += threads) tile[(e / kPanel) * (kPanel + 1) + e % kPanel] = s[static_cast<int64_t>(k0 + e / kPanel) * ld + k0 + e % kPanel];
    if (tid < kPanel) x[tid] = rhs[k0 + tid];
    __syncthreads();
    for (int j = 0; j < kPanel; ++j) {
      if (tid == j) x[j] = x[j] / tile[j * (kPanel + 1) + j];
      __syncthreads();
      if (tid > j && tid < kPanel) x[tid] -= tile[tid * (kPanel + 1) + j] * x[j];
      __syncthreads();
    }
    if (tid < kPanel) rhs[k0 + tid] = x[tid];
    for (int row = k0 + kPanel + tid; row < np; row += threads) {
      const double* l = s + static_cast<int64_t>(row) * ld + k0;
      double t = rhs[row];
      for (int j = 0; j < kPanel; ++j) t -= l[j] * x[j];
      rhs[row] = t;
    }
    __syncthreads();
  }
  for (int k0 = np - kPanel; k0 >= 0; k0 -= kPanel) {
    for (int e = tid; e < kPanel * kPanel; e += threads) tile[(e / kPanel) * (kPanel + 1) + e % kPanel] = s[static_cast<int64_t>(k0 + e / kPanel) * ld + k0 + e % kPanel];
    if (tid < kPanel) x[tid] = rhs[k0 + tid];
    __syncthreads();
    for (int j = kPanel - 1; j >= 0; --j) {
      if (tid == j) x[j] = x[j] / tile[j * (kPanel + 1) + j];
      __syncthreads();
      if (tid < j) x[tid] -= tile[j * (kPanel + 1) + tid] * x[j];
      __syncthreads();
    }
    if (tid < kPanel) rhs[k0 + tid] = x[tid];
    for (int row = tid; row < k0; row += threads) {
      double t = rhs[row];
      for (int j = 0; j < kPanel; ++j) t -= s[static_cast<int64_t>(k0 + j) * ld + row] * x[j];
      rhs[row] = t;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) pg_panel_kernel(Graph g, int k0) {
  __shared__ double tile[kPanel * (kPanel + 1)];
  if (*g.flag != 0u) return;
  panel_block(g.s, g.np, k0, tile, g.flag);
}
__global__ void __launch_bounds__(64) pg_trsm_kernel(Graph g, int k0) {
  __shared__ double tile[kPanel * (kPanel + 1)];
  if (*g.flag != 0u) return;
  for (int e = threadIdx.x; e < kPanel * kPanel; e += blockDim.x)
    tile[(e / kPanel) * (kPanel + 1) + e % kPanel] = g.s[static_cast<int64_t>(k0 + e / kPanel) * g.np + k0 + e % kPanel];
  __syncthreads();
  const int row = k0 + kPanel + blockIdx.x * blockDim.x + threadIdx.x;
  if (row < g.np) trsm_row(g.s, g.np, k0, row, tile);
}
// grid: (tiles, ceil(tiles / 4)); 4 wavefronts a workgroup, one lower tile each
__global__ void __launch_bounds__(256) pg_update_kernel(Graph g, int k0) {
  if (*g.flag != 0u) return;
  const int tj = blockIdx.x, ti = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int first = k0 + kPanel;
  if (tj > ti || first + 16 * ti >= g.np) return;
  update_tile(g.s, g.np, k0, first + 16 * ti, first + 16 * tj, threadIdx.x & 63);
}
__global__ void __launch_bounds__(kSmallThreads) pg_solve_kernel(Graph g) {
  __shared__ double tile[kPanel * (kPanel + 1)];
  __shared__ double x[kPanel];
  if (*g.flag != 0u) return;
  triangular_solves(g.s, g.np, g.np, g.rhs, tile, x);
}
// Small systems: factorisation and solves in one workgroup (early in a run the graph is a few submaps, and the launch
// count is what a solve costs).
__global__ void __launch_bounds__(kSmallThreads) pg_small_kernel(Graph g) {
  __shared__ double tile[kPanel * (kPanel + 1)];
  __shared__ double x[kPanel];
  __shared__ unsigned failed;
  if (*g.flag != 0u) return;
  const int tid = threadIdx.x;
  for (int k0 = 0; k0 < g.np; k0 += kPanel) {
    panel_block(g.s, g.np, k0, tile, g.flag);
    __syncthreads();
    if (tid == 0) failed = *g.flag;
    __syncthreads();
    if (failed != 0u) return;
    for (int row = k0 + kPanel + tid; row < g.np; row += blockDim.x) trsm_row(g.s, g.np, k0, row, tile);
    __syncthreads();
    const int tiles = (g.np - k0 - kPanel) / 16;
    for (int t = tid >> 6; t < tiles * tiles; t += blockDim.x >> 6) {
      const int ti = t / tiles, tj = t % tiles;
      if (tj <= ti) update_tile(g.s, g.np, k0, k0 + kPanel + 16 * ti, k0 + kPanel + 16 * tj, tid & 63);
    }
    __syncthreads();
  }
  triangular_solves(g.s, g.np, g.np, g.rhs, tile, x);
}

// ---- back-substitution -------------------------------------------------------------------------------------------------
// Per pose: the scaled step (a submap's from the solve, a node's -V (g_n + sum E^T y_s)), delta = step * scale, Plus into
// the candidate, ||x - candidate||^2 over the blocks in the problem.
__global__ void pg_step_kernel(Graph g) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pose_count(g) || *g.flag != 0u) return;
  const int mask = g.mask[p];
  const double* scale = g.scale + 6 * static_cast<int64_t>(p);
  double y[6];
  if (is_kept(g, p)) {
    for (int k = 0; k < 6; ++k) y[k] = g.column[p * 6 + k] >= 0 ? g.rhs[g.column[p * 6 + k]] : 0.;
  } else {
    double w[6];
    for (int k = 0; k < 6; ++k) w[k] = scale[k] * g.gradient[6 * static_cast<int64_t>(p) + k];
    for (int at = g.pose_start[p]; at < g.pose_start[p + 1]; ++at) {
      const int64_t c = g.pose_constraints[at];
      const int a = g.constraint_submap[c];
      const double* e = g.cross + 36 * c;
      for (int i = 0; i < 6; ++i) {
        const int col = g.column[a * 6 + i];
        if (col < 0) continue;
        const double ys = g.rhs[col];
        for (int k = 0; k < 6; ++k) w[k] += e[i * 6 + k] * ys;
      }
    }
    const double* v = g.v + 36 * static_cast<int64_t>(p - g.num_kept);
    for (int i = 0; i < 6; ++i) {
      double t = 0.;
      for (int k = 0; k < 6; ++k) t += v[i * 6 + k] * w[k];
      y[i] = -t;
    }
  }
  double delta[6], out[7];
  for (int k = 0; k < 6; ++k) {
    if (!((mask >> k) & 1)) y[k] = 0.;
    delta[k] = y[k] * scale[k];
    g.step[6 * static_cast<int64_t>(p) + k] = y[k];
    g.delta[6 * static_cast<int64_t>(p) + k] = delta[k];
  }
  const double* x = g.x + 7 * static_cast<int64_t>(p);
  pose_plus(x, delta, mask, kind_of(g, p), out);
  double squared = 0.;
  for (int k = 0; k < 7; ++k) {
    g.candidate[7 * static_cast<int64_t>(p) + k] = out[k];
    if ((k < 3 ? mask & 7 : mask & 56) != 0) squared += (x[k] - out[k]) * (x[k] - out[k]);
  }
  g.step_squared[p] = squared;
}
// Per constraint: (J y) . (r + J y / 2), and the candidate's cost (the cost-only variant: no duals' parts).
__global__ void __launch_bounds__(256) pg_candidate_kernel(Graph g) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g.num_constraints || *g.flag != 0u) return;
  const double* da = g.delta + 6 * static_cast<int64_t>(g.constraint_submap[c]);
  const double* dn = g.delta + 6 * static_cast<int64_t>(g.num_kept + g.constraint_node[c]);
  const double* jac = g.jacobian + 72 * static_cast<int64_t>(c);
  double model = 0.;
  for (int k = 0; k < 6; ++k) {
    double jy = 0.;
    for (int i = 0; i < 6; ++i) jy += jac[k * 6 + i] * da[i];
    for (int i = 0; i < 6; ++i) jy += jac[36 + k * 6 + i] * dn[i];
    model += jy * (g.residual[6 * static_cast<int64_t>(c) + k] + jy / 2.0);
  }
  g.model[c] = model;
  Dual<0> e[6];
  evaluate_constraint<0>(g, g.candidate, c, e);
  double squared = 0., scaling;
  for (int k = 0; k < 6; ++k) squared += e[k].a * e[k].a;
  g.candidate_cost[c] = constraint_cost(g, c, squared, &scaling);
}

// Per observation: the same over its three blocks.
__global__ void __launch_bounds__(256) pg_observation_candidate_kernel(Graph g) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= g.num_observations || *g.flag != 0u) return;
  const double* jac = g.jacobian + 72 * static_cast<int64_t>(g.num_constraints) + 108 * static_cast<int64_t>(o);
  const double* residual = g.residual + 6 * (static_cast<int64_t>(g.num_constraints) + o);
  double model = 0.;
  for (int k = 0; k < 6; ++k) {
    double jy = 0.;
    for (int block = 0; block < 3; ++block) {
      const double* d = g.delta + 6 * static_cast<int64_t>(g.observation_pose[3 * o + block]);
      for (int i = 0; i < 6; ++i) jy += jac[36 * block + k * 6 + i] * d[i];
    }
    model += jy * (residual[k] + jy / 2.0);
  }
  g.model[g.num_constraints + o] = model;
  Dual<0> e[6];
  evaluate_observation<0>(g, g.candidate, o, 0, e);
  double squared = 0.;
  for (int k = 0; k < 6; ++k) squared += e[k].a * e[k].a;
  g.candidate_cost[g.num_constraints + o] = 0.5 * squared;
}

// The sums of an iteration in a fixed order (thread t takes elements t, t + 1024, ...; then a tree), into the
// page-locked block, and the completion word behind them.
__device__ inline double block_sum(double mine, double* scratch, bool maximum) {
  const int tid = threadIdx.x;
  __syncthreads();
  scratch[tid] = mine;
  __syncthreads();
  for (int half = kSmallThreads / 2; half > 0; half >>= 1) {
    if (tid < half) scratch[tid] = maximum ? fmax(scratch[tid], scratch[tid + half]) : scratch[tid] + scratch[tid + half];
    __syncthreads();
  }
  return scratch[0];
}
__global__ void __launch_bounds__(kSmallThreads) pg_reduce_kernel(Graph g, int with_step, double* out, unsigned* done_word, unsigned done_seq) {
  __shared__ double scratch[kSmallThreads];
  const int tid = threadIdx.x;
  const int poses = pose_count(g);
  const bool step = with_step != 0 && *g.flag == 0u;
  double cost = 0., fixed = 0., most = 0., x_squared = 0., model = 0., candidate = 0., step_squared = 0.;
  for (int c = tid; c < g.num_constraints + g.num_observations; c += kSmallThreads) {
    if (c < g.num_constraints ? g.fixed[c] : g.observation_fixed[c - g.num_constraints]) {
      fixed += g.cost[c];
    } else {
      cost += g.cost[c];
      if (step) model += g.model[c], candidate += g.candidate_cost[c];
    }
  }
  for (int p = tid; p < poses; p += kSmallThreads) {
    most = fmax(most, g.gradient_max[p]);
    x_squared += g.x_squared[p];
    if (step) step_squared += g.step_squared[p];
  }
  double sums[kSums];
  sums[kSumCost] = block_sum(cost, scratch, false);
  sums[kSumFixedCost] = block_sum(fixed, scratch, false);
  sums[kSumGradientMax] = block_sum(most, scratch, true);
  sums[kSumXSquared] = block_sum(x_squared, scratch, false);
  sums[kSumModel] = block_sum(model, scratch, false);
  sums[kSumCandidateCost] = block_sum(candidate, scratch, false);
  sums[kSumStepSquared] = block_sum(step_squared, scratch, false);
  sums[kSumFlag] = *g.flag != 0u ? 1. : 0.;
  if (tid == 0) {
    for (int k = 0; k < kSums; ++k) out[k] = sums[k];
    __threadfence_system();
    if (done_word != nullptr) *reinterpret_cast<volatile unsigned*>(done_word) = done_seq;
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct Solver {
  dliom_ctx* ctx = nullptr;
  pg::Structure structure;
  Graph g = {};
  void* device = nullptr;
  double* best = nullptr;  // 7 a pose: the iterate of the lowest cost so far
  double stage_ms[4] = {0., 0., 0., 0.};
  std::chrono::steady_clock::time_point stage_begin;
  int read_backs = 0;

  ~Solver() {
    if (device != nullptr) (void)hipFree(device);
  }
  int begin_stage() {
    if (!ctx->profiling) return DLIOM_OK;
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    stage_begin = std::chrono::steady_clock::now();
    return DLIOM_OK;
  }
  int end_stage(int stage) {
    if (!ctx->profiling) return DLIOM_OK;
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    stage_ms[stage] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - stage_begin).count();
    return DLIOM_OK;
  }
};

bool all_finite(const double* v, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// Checks the arguments, builds the structure, allocates and uploads: nothing is launched before this returns DLIOM_OK.
int prepare(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps, const double* submap_poses7,
            const unsigned char* submap_constant, int gravity_aligned_submap, int num_nodes, const double* node_poses7,
            const unsigned char* node_constant, int64_t num_constraints, const dliom_pose_graph_constraint* constraints,
            const dliom_pose_graph_terms* terms, const dliom_pose_graph_landmarks* landmarks, Solver* solver) {
  static const dliom_pose_graph_terms kNoTerms = {0, nullptr, 0, nullptr, 0., nullptr};
  static const dliom_pose_graph_landmarks kNoLandmarks = {0, nullptr, nullptr, 0, nullptr};
  if (terms == nullptr) terms = &kNoTerms;
  if (landmarks == nullptr) landmarks = &kNoLandmarks;
  const int num_landmarks = landmarks->num_landmarks;
  const int64_t num_observations = landmarks->num_observations;
  const dliom_pose_graph_landmark_observation* observations = landmarks->observations;
  if (num_landmarks < 0 || num_observations < 0 || (num_landmarks > 0 && landmarks->landmark_poses7 == nullptr) ||
      (num_observations > 0 && observations == nullptr))
    return DLIOM_ERR_INVALID_ARGUMENT;
  const bool with_landmarks = num_landmarks > 0 || num_observations > 0;
  const int num_frames = terms->num_fixed_frames;
  const int64_t num_frame_constraints = terms->num_fixed_frame_constraints;
  const dliom_pose_graph_constraint* frame_constraints = terms->fixed_frame_constraints;
  if (num_frames < 0 || num_frame_constraints < 0 || (num_frames > 0 && terms->fixed_frame_poses7 == nullptr) ||
      (num_frame_constraints > 0 && frame_constraints == nullptr) || !(terms->huber_scale >= 0.) || !std::isfinite(terms->huber_scale))
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (ctx == nullptr || options == nullptr || num_submaps < 0 || num_nodes < 0 || num_constraints < 0 ||
      (num_submaps > 0 && submap_poses7 == nullptr) || (num_nodes > 0 && node_poses7 == nullptr) ||
      (num_constraints > 0 && constraints == nullptr) || gravity_aligned_submap < -1 || gravity_aligned_submap >= num_submaps)
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (static_cast<int64_t>(num_submaps) + num_frames + num_nodes + num_landmarks > INT32_MAX / 72) return DLIOM_ERR_TOO_LARGE;
  solver->ctx = ctx;
  pg::Structure& s = solver->structure;
  constexpr int64_t stride = sizeof(dliom_pose_graph_constraint) / sizeof(int32_t);
  static_assert(sizeof(dliom_pose_graph_constraint) % sizeof(int32_t) == 0, "the constraints are read with an int32 stride");
  const int32_t* first = reinterpret_cast<const int32_t*>(constraints);
  const int32_t* frame_first = reinterpret_cast<const int32_t*>(frame_constraints);
  constexpr int64_t observation_stride = sizeof(dliom_pose_graph_landmark_observation) / sizeof(int32_t);
  static_assert(sizeof(dliom_pose_graph_landmark_observation) % sizeof(int32_t) == 0, "the observations are read with an int32 stride");
  const int32_t* observation_first = reinterpret_cast<const int32_t*>(observations);
  pg::Indices in;
  in.num_submaps = num_submaps, in.submap_constant = submap_constant, in.gravity_aligned_submap = gravity_aligned_submap;
  in.num_fixed_frames = num_frames;
  in.num_nodes = num_nodes, in.node_constant = node_constant;
  in.num_constraints = num_constraints, in.constraint_submap = first, in.constraint_node = first + 1, in.constraint_stride = stride;
  in.num_frame_constraints = num_frame_constraints, in.frame_constraint_frame = frame_first, in.frame_constraint_node = frame_first + 1;
  in.frame_constraint_stride = stride;
  in.num_landmarks = num_landmarks, in.landmark_constant = landmarks->landmark_constant;
  in.num_observations = num_observations, in.observation_landmark = observation_first, in.observation_prev = observation_first + 1;
  in.observation_next = observation_first + 2, in.observation_stride = observation_stride;
  in.fix_z = options->fix_z_in_3d != 0;
  in.max_reduced_dimension = DLIOM_POSE_GRAPH_MAX_REDUCED_DIMENSION;
  const int status = pg::build_structure(in, &s);
  if (status == pg::kStructureBadIndex) return DLIOM_ERR_INVALID_ARGUMENT;
  if (status == pg::kStructureTooLarge) return DLIOM_ERR_TOO_LARGE;
  if (!all_finite(submap_poses7, 7 * static_cast<int64_t>(num_submaps)) || !all_finite(node_poses7, 7 * static_cast<int64_t>(num_nodes)))
    return DLIOM_ERR_SOLVER;
  if (!all_finite(terms->fixed_frame_poses7, 7 * static_cast<int64_t>(num_frames))) return DLIOM_ERR_SOLVER;
  if (!all_finite(landmarks->landmark_poses7, 7 * static_cast<int64_t>(num_landmarks))) return DLIOM_ERR_SOLVER;
  for (int64_t o = 0; o < num_observations; ++o)
    if (!std::isfinite(observations[o].interpolation_parameter) || !all_finite(observations[o].landmark_to_tracking7, 7) ||
        !std::isfinite(observations[o].translation_weight) || !std::isfinite(observations[o].rotation_weight))
      return DLIOM_ERR_SOLVER;
  // residual block c: the constraints, then the fixed frames'
  const int64_t C = num_constraints + num_frame_constraints;
  auto block = [&](int64_t c) -> const dliom_pose_graph_constraint& {
    return c < num_constraints ? constraints[c] : frame_constraints[c - num_constraints];
  };
  for (int64_t c = 0; c < C; ++c)
    if (!all_finite(block(c).zbar, 7) || !std::isfinite(block(c).translation_weight) || !std::isfinite(block(c).rotation_weight))
      return DLIOM_ERR_SOLVER;
  // fixed-frame constraints never carry a loss (optimization_problem_3d.cc:541-546)
  const bool with_loss = terms->huber_scale > 0. && terms->inter_submap != nullptr;

  Graph& g = solver->g;
  const int64_t kept = static_cast<int64_t>(num_submaps) + num_frames, poses = kept + num_nodes + num_landmarks;
  const int64_t O = num_observations;
  g.num_kept = static_cast<int>(kept);
  g.num_landmarks = num_landmarks;
  g.num_observations = static_cast<int>(O);
  g.huber_scale = with_loss ? terms->huber_scale : 0.;
  g.num_nodes = num_nodes;
  g.num_constraints = static_cast<int>(C);
  g.num_pairs = static_cast<int>(s.pair_a.size());
  g.n = s.reduced_dimension;
  g.np = std::max(kPanel, (g.n + kPanel - 1) / kPanel * kPanel);
  // one host buffer, one copy: [constraint data | poses | int arrays] (a vector of doubles; the ints ride in its tail)
  // Without landmarks and observations the device sees the columns of the submaps and the fixed frames only, and none
  // of the observations' and the direct terms' lists: node_promoted and pair_direct_start stay null, and the kernels
  // branch on that.
  const size_t num_columns = 6 * static_cast<size_t>(with_landmarks ? poses : kept);
  size_t num_ints = (with_loss ? 3 : 2) * static_cast<size_t>(C) + s.kind.size() + s.mask.size() + num_columns + s.fixed.size() + s.pose_start.size() +
                          s.pose_constraints.size() + s.pair_a.size() + s.pair_b.size() + s.pair_start.size() + s.pair_c.size() +
                          s.pair_c2.size() + 1 + 3 * static_cast<size_t>(O);
  if (with_landmarks)
    num_ints += s.observation_fixed.size() + s.node_promoted.size() + s.pose_observation_start.size() + s.pose_observations.size() +
                s.pair_direct_start.size() + s.pair_direct_a.size() + s.pair_direct_b.size();
  const size_t upload_doubles = static_cast<size_t>(9 * C + 7 * poses + 10 * O);
  std::vector<double> host(upload_doubles + (num_ints + 1) / 2);
  for (int64_t c = 0; c < C; ++c) {
    std::memcpy(&host[9 * c], block(c).zbar, 7 * sizeof(double));
    host[9 * c + 7] = block(c).translation_weight;
    host[9 * c + 8] = block(c).rotation_weight;
  }
  if (num_submaps > 0) std::memcpy(&host[9 * C], submap_poses7, sizeof(double) * 7 * num_submaps);
  if (num_frames > 0) std::memcpy(&host[9 * C + 7 * static_cast<int64_t>(num_submaps)], terms->fixed_frame_poses7, sizeof(double) * 7 * num_frames);
  if (num_nodes > 0) std::memcpy(&host[9 * C + 7 * kept], node_poses7, sizeof(double) * 7 * num_nodes);
  if (num_landmarks > 0) std::memcpy(&host[9 * C + 7 * (kept + num_nodes)], landmarks->landmark_poses7, sizeof(double) * 7 * num_landmarks);
  for (int64_t o = 0; o < O; ++o) {
    double* data = &host[9 * C + 7 * poses + 10 * o];
    std::memcpy(data, observations[o].landmark_to_tracking7, 7 * sizeof(double));
    data[7] = observations[o].translation_weight;
    data[8] = observations[o].rotation_weight;
    data[9] = observations[o].interpolation_parameter;
  }
  int32_t* host_ints = reinterpret_cast<int32_t*>(host.data() + upload_doubles);
  size_t ints_used = 0;
  auto append = [&](const std::vector<int32_t>& v, size_t at_most = SIZE_MAX) {
    const size_t at = ints_used, count = std::min(v.size(), at_most);
    if (count > 0) std::memcpy(host_ints + at, v.data(), count * sizeof(int32_t));
    ints_used += count;
    return at;
  };
  const size_t at_submap = ints_used;
  for (int64_t c = 0; c < C; ++c) host_ints[ints_used++] = c < num_constraints ? block(c).submap : num_submaps + block(c).submap;
  const size_t at_node = ints_used;
  for (int64_t c = 0; c < C; ++c) host_ints[ints_used++] = block(c).node;
  const size_t at_lossy = ints_used;
  if (with_loss)
    for (int64_t c = 0; c < C; ++c) host_ints[ints_used++] = c < num_constraints && terms->inter_submap[c] != 0 ? 1 : 0;
  const size_t at_kind = append(s.kind);
  const size_t at_mask = append(s.mask), at_column = append(s.column, num_columns), at_fixed = append(s.fixed), at_start = append(s.pose_start),
               at_list = append(s.pose_constraints), at_a = append(s.pair_a), at_b = append(s.pair_b),
               at_pair_start = append(s.pair_start), at_c = append(s.pair_c), at_c2 = append(s.pair_c2);
  host_ints[ints_used++] = 0;
  const size_t at_observation_pose = ints_used;
  for (int64_t o = 0; o < O; ++o) {
    host_ints[ints_used++] = static_cast<int32_t>(kept) + observations[o].prev_node;
    host_ints[ints_used++] = static_cast<int32_t>(kept) + observations[o].next_node;
    host_ints[ints_used++] = static_cast<int32_t>(kept) + num_nodes + observations[o].landmark;
  }
  const size_t landmark_ints = with_landmarks ? SIZE_MAX : 0;
  const size_t at_observation_fixed = append(s.observation_fixed, landmark_ints), at_promoted = append(s.node_promoted, landmark_ints),
               at_observation_start = append(s.pose_observation_start, landmark_ints),
               at_observation_list = append(s.pose_observations, landmark_ints),
               at_direct_start = append(s.pair_direct_start, landmark_ints), at_direct_a = append(s.pair_direct_a, landmark_ints),
               at_direct_b = append(s.pair_direct_b, landmark_ints);

  // the device block: doubles, then the ints
  int64_t doubles = 0;
  auto take = [&doubles](int64_t count) {
    const int64_t at = doubles;
    doubles += (count + 31) / 32 * 32;
    return at;
  };
  const int64_t np = g.np;
  const int64_t o_upload = take(static_cast<int64_t>(host.size())), o_candidate = take(7 * poses), o_scale = take(6 * poses),
                o_block = take(36 * poses), o_gradient = take(6 * poses), o_residual = take(6 * (C + O)), o_jacobian = take(72 * C + 108 * O),
                o_cross = take(36 * C), o_cross_v = take(36 * C), o_cross_vg = take(6 * C), o_v = take(36 * static_cast<int64_t>(num_nodes)),
                o_vg = take(6 * static_cast<int64_t>(num_nodes)), o_rhs = take(np), o_step = take(6 * poses), o_delta = take(6 * poses),
                o_model = take(C + O), o_cost = take(C + O), o_candidate_cost = take(C + O), o_step_squared = take(poses),
                o_x_squared = take(poses), o_gradient_max = take(poses), o_flag = take(32), o_best = take(7 * poses), o_s = take(np * np);
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_HIP_TRY(hipMalloc(&solver->device, static_cast<size_t>(doubles) * sizeof(double)));
  double* d = static_cast<double*>(solver->device);
  const int32_t* ints = reinterpret_cast<const int32_t*>(d + o_upload + upload_doubles);
  DLIOM_HIP_TRY(hipMemcpyAsync(d + o_upload, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  DLIOM_HIP_TRY(hipMemsetAsync(d + o_flag, 0, 32 * sizeof(double), ctx->stream));
  DLIOM_HIP_TRY(hipMemsetAsync(d + o_scale, 0, static_cast<size_t>(o_residual - o_scale) * sizeof(double), ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // the host buffer goes out of scope
  ++ctx->host_syncs;
  g.constraint_data = d + o_upload;
  g.x = d + o_upload + 9 * C;
  g.candidate = d + o_candidate;
  g.scale = d + o_scale;
  g.diagonal_block = d + o_block;
  g.gradient = d + o_gradient;
  g.residual = d + o_residual;
  g.jacobian = d + o_jacobian;
  g.cross = d + o_cross;
  g.cross_v = d + o_cross_v;
  g.cross_vg = d + o_cross_vg;
  g.v = d + o_v;
  g.vg = d + o_vg;
  g.rhs = d + o_rhs;
  g.step = d + o_step;
  g.delta = d + o_delta;
  g.model = d + o_model;
  g.cost = d + o_cost;
  g.candidate_cost = d + o_candidate_cost;
  g.step_squared = d + o_step_squared;
  g.x_squared = d + o_x_squared;
  g.gradient_max = d + o_gradient_max;
  g.flag = reinterpret_cast<unsigned*>(d + o_flag);
  g.s = d + o_s;
  g.constraint_submap = ints + at_submap;
  g.constraint_node = ints + at_node;
  g.kind = ints + at_kind;
  g.lossy = with_loss ? ints + at_lossy : nullptr;
  g.mask = ints + at_mask;
  g.column = ints + at_column;
  g.fixed = ints + at_fixed;
  g.pose_start = ints + at_start;
  g.pose_constraints = ints + at_list;
  g.pair_a = ints + at_a;
  g.pair_b = ints + at_b;
  g.pair_start = ints + at_pair_start;
  g.pair_c = ints + at_c;
  g.pair_c2 = ints + at_c2;
  g.observation_data = d + o_upload + 9 * C + 7 * poses;
  g.observation_pose = ints + at_observation_pose;
  g.observation_fixed = ints + at_observation_fixed;
  g.node_promoted = with_landmarks ? ints + at_promoted : nullptr;
  g.pose_observation_start = ints + at_observation_start;
  g.pose_observations = ints + at_observation_list;
  g.pair_direct_start = with_landmarks ? ints + at_direct_start : nullptr;
  g.pair_direct_a = ints + at_direct_a;
  g.pair_direct_b = ints + at_direct_b;
  solver->best = d + o_best;
  return DLIOM_OK;
}

int enqueue_linearise(Solver* solver, bool set_scale) {
  const Graph& g = solver->g;
  hipStream_t stream = solver->ctx->stream;
  const int poses = g.num_kept + g.num_nodes + g.num_landmarks;
  DLIOM_TRY(solver->begin_stage());
  if (g.num_constraints > 0) hipLaunchKernelGGL(pg_linearise_kernel, dim3(blocks_of(g.num_constraints, 64)), dim3(64), 0, stream, g);
  if (g.num_observations > 0)
    hipLaunchKernelGGL(pg_observation_linearise_kernel, dim3(blocks_of(3 * g.num_observations, 64)), dim3(64), 0, stream, g);
  if (poses > 0) {
    hipLaunchKernelGGL(pg_pose_kernel, dim3(blocks_of(poses, 4)), dim3(256), 0, stream, g, set_scale ? 1 : 0);
    hipLaunchKernelGGL(pg_pose_values_kernel, dim3(blocks_of(poses, 256)), dim3(256), 0, stream, g);
  }
  DLIOM_HIP_TRY(hipGetLastError());
  return solver->end_stage(0);
}

int enqueue_step(Solver* solver, double radius) {
  const Graph& g = solver->g;
  hipStream_t stream = solver->ctx->stream;
  const int poses = g.num_kept + g.num_nodes + g.num_landmarks;
  DLIOM_TRY(solver->begin_stage());
  DLIOM_HIP_TRY(hipMemsetAsync(g.flag, 0, sizeof(unsigned), stream));
  DLIOM_HIP_TRY(hipMemsetAsync(g.rhs, 0, static_cast<size_t>(g.np) * sizeof(double), stream));
  hipLaunchKernelGGL(pg_zero_lower_kernel, dim3(g.np / kPanel, g.np / kPanel), dim3(256), 0, stream, g);
  if (g.num_nodes > 0) hipLaunchKernelGGL(pg_node_kernel, dim3(blocks_of(g.num_nodes, 64)), dim3(64), 0, stream, g, radius);
  if (g.num_pairs > 0) hipLaunchKernelGGL(pg_pairs_kernel, dim3(blocks_of(g.num_pairs, 4)), dim3(256), 0, stream, g, radius);
  hipLaunchKernelGGL(pg_rhs_kernel, dim3(blocks_of(std::max((g.node_promoted != nullptr ? poses : g.num_kept) * 6, g.np), 256)), dim3(256), 0, stream, g);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_TRY(solver->end_stage(1));
  DLIOM_TRY(solver->begin_stage());
  if (g.np <= kSmallDimension) {
    hipLaunchKernelGGL(pg_small_kernel, dim3(1), dim3(kSmallThreads), 0, stream, g);
  } else {
    for (int k0 = 0; k0 < g.np; k0 += kPanel) {
      hipLaunchKernelGGL(pg_panel_kernel, dim3(1), dim3(256), 0, stream, g, k0);
      const int rows = g.np - k0 - kPanel;
      if (rows <= 0) break;
      hipLaunchKernelGGL(pg_trsm_kernel, dim3(blocks_of(rows, 64)), dim3(64), 0, stream, g, k0);
      const int tiles = rows / 16;
      hipLaunchKernelGGL(pg_update_kernel, dim3(tiles, blocks_of(tiles, 4)), dim3(256), 0, stream, g, k0);
    }
    hipLaunchKernelGGL(pg_solve_kernel, dim3(1), dim3(kSmallThreads), 0, stream, g);
  }
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_TRY(solver->end_stage(2));
  DLIOM_TRY(solver->begin_stage());
  if (poses > 0) hipLaunchKernelGGL(pg_step_kernel, dim3(blocks_of(poses, 256)), dim3(256), 0, stream, g);
  if (g.num_constraints > 0) hipLaunchKernelGGL(pg_candidate_kernel, dim3(blocks_of(g.num_constraints, 256)), dim3(256), 0, stream, g);
  if (g.num_observations > 0)
    hipLaunchKernelGGL(pg_observation_candidate_kernel, dim3(blocks_of(g.num_observations, 256)), dim3(256), 0, stream, g);
  DLIOM_HIP_TRY(hipGetLastError());
  return solver->end_stage(3);
}

// The iteration's one read-back.
int read_sums(Solver* solver, bool with_step, double sums[kSums]) {
  dliom_ctx* ctx = solver->ctx;
  double* host = pinned_at<double>(ctx, kPinPoseGraphSums);
  static_assert(kSums * sizeof(double) <= kPinPoseGraphSums.bytes, "the sums fit their region");
  unsigned* done = ctx->done_word;
  const unsigned seq = done != nullptr ? next_done_seq(ctx) : 0u;
  hipLaunchKernelGGL(pg_reduce_kernel, dim3(1), dim3(kSmallThreads), 0, ctx->stream, solver->g, with_step ? 1 : 0, host, done, seq);
  DLIOM_HIP_TRY(hipGetLastError());
  if (done != nullptr) {
    DLIOM_TRY(wait_done(ctx, ctx->stream, done, seq, 2000));
  } else {
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    ++ctx->host_syncs;
  }
  ++solver->read_backs;
  for (int k = 0; k < kSums; ++k) sums[k] = host[k];
  return DLIOM_OK;
}

// `width` doubles a pose from the device's order (submaps, fixed frames, nodes, landmarks) into the caller's four arrays;
// enqueued.
int copy_poses_out(Solver* solver, const double* device, int width, int num_submaps, int num_nodes, double* submaps, double* nodes,
                   double* frames, double* landmarks) {
  hipStream_t stream = solver->ctx->stream;
  const size_t S = static_cast<size_t>(num_submaps), K = static_cast<size_t>(solver->g.num_kept), bytes = sizeof(double) * width;
  if (S > 0) DLIOM_HIP_TRY(hipMemcpyAsync(submaps, device, bytes * S, hipMemcpyDeviceToHost, stream));
  if (K > S) DLIOM_HIP_TRY(hipMemcpyAsync(frames, device + width * S, bytes * (K - S), hipMemcpyDeviceToHost, stream));
  if (num_nodes > 0) DLIOM_HIP_TRY(hipMemcpyAsync(nodes, device + width * K, bytes * num_nodes, hipMemcpyDeviceToHost, stream));
  if (solver->g.num_landmarks > 0)
    DLIOM_HIP_TRY(hipMemcpyAsync(landmarks, device + width * (K + num_nodes), bytes * solver->g.num_landmarks, hipMemcpyDeviceToHost, stream));
  return DLIOM_OK;
}

}  // namespace
}  // namespace dliom

using namespace dliom;

extern "C" {

int dliom_pose_graph_evaluate_landmarks(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps,
                                        const double* submap_poses7, const unsigned char* submap_constant, int gravity_aligned_submap,
                                        int num_nodes, const double* node_poses7, const unsigned char* node_constant,
                                        int64_t num_constraints, const dliom_pose_graph_constraint* constraints,
                                        const dliom_pose_graph_terms* terms, const dliom_pose_graph_landmarks* landmarks, double* cost,
                                        double* residuals, double* gradient) {
  Solver solver;
  DLIOM_TRY(prepare(ctx, options, num_submaps, submap_poses7, submap_constant, gravity_aligned_submap, num_nodes, node_poses7,
                    node_constant, num_constraints, constraints, terms, landmarks, &solver));
  DLIOM_TRY(enqueue_linearise(&solver, true));
  double sums[kSums];
  DLIOM_TRY(read_sums(&solver, false, sums));
  if (cost != nullptr) *cost = sums[kSumCost] + sums[kSumFixedCost];
  const size_t blocks = static_cast<size_t>(solver.g.num_constraints) + solver.g.num_observations;
  if (residuals != nullptr && blocks > 0)
    DLIOM_HIP_TRY(hipMemcpyAsync(residuals, solver.g.residual, sizeof(double) * 6 * blocks, hipMemcpyDeviceToHost, ctx->stream));
  const size_t before_frames = static_cast<size_t>(num_submaps) + num_nodes, before_landmarks = static_cast<size_t>(solver.g.num_kept) + num_nodes;
  if (gradient != nullptr) DLIOM_TRY(copy_poses_out(&solver, solver.g.gradient, 6, num_submaps, num_nodes, gradient, gradient + 6 * static_cast<size_t>(num_submaps),
                                                    gradient + 6 * before_frames, gradient + 6 * before_landmarks));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  return DLIOM_OK;
}
int dliom_pose_graph_evaluate_terms(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps,
                                    const double* submap_poses7, const unsigned char* submap_constant, int gravity_aligned_submap,
                                    int num_nodes, const double* node_poses7, const unsigned char* node_constant,
                                    int64_t num_constraints, const dliom_pose_graph_constraint* constraints,
                                    const dliom_pose_graph_terms* terms, double* cost, double* residuals, double* gradient) {
  return dliom_pose_graph_evaluate_landmarks(ctx, options, num_submaps, submap_poses7, submap_constant, gravity_aligned_submap,
                                             num_nodes, node_poses7, node_constant, num_constraints, constraints, terms, nullptr, cost,
                                             residuals, gradient);
}
int dliom_pose_graph_evaluate(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps,
                              const double* submap_poses7, const unsigned char* submap_constant, int gravity_aligned_submap,
                              int num_nodes, const double* node_poses7, const unsigned char* node_constant,
                              int64_t num_constraints, const dliom_pose_graph_constraint* constraints, double* cost,
                              double* residuals, double* gradient) {
  return dliom_pose_graph_evaluate_terms(ctx, options, num_submaps, submap_poses7, submap_constant, gravity_aligned_submap, num_nodes,
                                         node_poses7, node_constant, num_constraints, constraints, nullptr, cost, residuals, gradient);
}

int dliom_pose_graph_step_landmarks(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps,
                                    const double* submap_poses7, const unsigned char* submap_constant, int gravity_aligned_submap,
                                    int num_nodes, const double* node_poses7, const unsigned char* node_constant,
                                    int64_t num_constraints, const dliom_pose_graph_constraint* constraints,
                                    const dliom_pose_graph_terms* terms, const dliom_pose_graph_landmarks* landmarks, double radius,
                                    double* delta, double* model_cost_change, int* reduced_dimension) {
  if (!(radius > 0.)) return DLIOM_ERR_INVALID_ARGUMENT;
  Solver solver;
  DLIOM_TRY(prepare(ctx, options, num_submaps, submap_poses7, submap_constant, gravity_aligned_submap, num_nodes, node_poses7,
                    node_constant, num_constraints, constraints, terms, landmarks, &solver));
  if (reduced_dimension != nullptr) *reduced_dimension = solver.g.n;
  DLIOM_TRY(enqueue_linearise(&solver, true));
  DLIOM_TRY(enqueue_step(&solver, radius));
  double sums[kSums];
  DLIOM_TRY(read_sums(&solver, true, sums));
  if (sums[kSumFlag] != 0.) return DLIOM_ERR_SOLVER;
  if (model_cost_change != nullptr) *model_cost_change = -sums[kSumModel];
  const size_t before_frames = static_cast<size_t>(num_submaps) + num_nodes, before_landmarks = static_cast<size_t>(solver.g.num_kept) + num_nodes;
  if (delta != nullptr) DLIOM_TRY(copy_poses_out(&solver, solver.g.delta, 6, num_submaps, num_nodes, delta, delta + 6 * static_cast<size_t>(num_submaps),
                                                 delta + 6 * before_frames, delta + 6 * before_landmarks));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  return DLIOM_OK;
}
int dliom_pose_graph_step_terms(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps,
                                const double* submap_poses7, const unsigned char* submap_constant, int gravity_aligned_submap,
                                int num_nodes, const double* node_poses7, const unsigned char* node_constant,
                                int64_t num_constraints, const dliom_pose_graph_constraint* constraints,
                                const dliom_pose_graph_terms* terms, double radius, double* delta, double* model_cost_change,
                                int* reduced_dimension) {
  return dliom_pose_graph_step_landmarks(ctx, options, num_submaps, submap_poses7, submap_constant, gravity_aligned_submap, num_nodes,
                                         node_poses7, node_constant, num_constraints, constraints, terms, nullptr, radius, delta,
                                         model_cost_change, reduced_dimension);
}
int dliom_pose_graph_step(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps,
                          const double* submap_poses7, const unsigned char* submap_constant, int gravity_aligned_submap,
                          int num_nodes, const double* node_poses7, const unsigned char* node_constant,
                          int64_t num_constraints, const dliom_pose_graph_constraint* constraints, double radius,
                          double* delta, double* model_cost_change, int* reduced_dimension) {
  return dliom_pose_graph_step_terms(ctx, options, num_submaps, submap_poses7, submap_constant, gravity_aligned_submap, num_nodes,
                                     node_poses7, node_constant, num_constraints, constraints, nullptr, radius, delta,
                                     model_cost_change, reduced_dimension);
}

// trust_region_minimizer.cc of Ceres 1.13 (Init / IterationZero / the loop), with levenberg_marquardt_strategy.cc's
// radius rules and trust_region_step_evaluator.cc, for this configuration: third-party behaviour, restated.
int dliom_pose_graph_solve_landmarks(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps, double* submap_poses7,
                                     const unsigned char* submap_constant, int gravity_aligned_submap, int num_nodes,
                                     double* node_poses7, const unsigned char* node_constant, int64_t num_constraints,
                                     const dliom_pose_graph_constraint* constraints, const dliom_pose_graph_terms* terms,
                                     const dliom_pose_graph_landmarks* landmarks, dliom_pose_graph_summary* summary) {
  if (summary == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  const auto started = std::chrono::steady_clock::now();
  Solver solver;
  DLIOM_TRY(prepare(ctx, options, num_submaps, submap_poses7, submap_constant, gravity_aligned_submap, num_nodes, node_poses7,
                    node_constant, num_constraints, constraints, terms, landmarks, &solver));
  std::memset(summary, 0, sizeof(*summary));
  summary->reduced_dimension = solver.g.n;
  Graph& g = solver.g;
  const size_t pose_bytes = sizeof(double) * 7 * (static_cast<size_t>(g.num_kept) + num_nodes + g.num_landmarks);
  double* best = solver.best;

  // the 1.13 defaults that common/ceres_solver_options.cc:35-42 leaves alone
  constexpr double kMinRelativeDecrease = 1e-3, kFunctionTolerance = 1e-6, kGradientTolerance = 1e-10, kParameterTolerance = 1e-8;
  constexpr double kMaxRadius = 1e16, kMinRadius = 1e-32;
  constexpr int kMaxInvalidSteps = 5;
  const int max_nonmonotonic = options->use_nonmonotonic_steps ? 5 : 0;
  double radius = 1e4, decrease_factor = 2.0;
  // TrustRegionStepEvaluator
  double minimum_cost_e = 0., current_cost = 0., reference_cost = 0., candidate_cost_e = 0.;
  double accumulated_reference = 0., accumulated_candidate = 0.;
  int consecutive_nonmonotonic = 0;

  double x_cost = 0., x_norm = 0., fixed_cost = 0., minimum_cost = 0., gradient_max = 0.;
  std::vector<double> iteration_costs;
  int iteration = 0, invalid_in_a_row = 0, termination = -1;
  bool last_step_successful = false, linearised = false;
  auto record = [summary](int kind) {
    if (summary->num_recorded_steps < DLIOM_POSE_GRAPH_MAX_RECORDED_STEPS) summary->steps[summary->num_recorded_steps++] = static_cast<unsigned char>(kind);
  };

  DLIOM_HIP_TRY(hipMemcpyAsync(best, g.x, pose_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  for (;;) {
    // FinalizeIterationAndCheckIfMinimizerCanContinue of the previous iteration; the gradient test of an iteration whose
    // linearisation has not been read back yet follows below, with that read-back
    if (iteration > 0) {
      if (last_step_successful) {
        ++summary->num_successful_steps;
        if (x_cost < minimum_cost) {
          minimum_cost = x_cost;
          DLIOM_HIP_TRY(hipMemcpyAsync(best, g.x, pose_bytes, hipMemcpyDeviceToDevice, ctx->stream));
        }
      } else {
        ++summary->num_unsuccessful_steps;
      }
      if (iteration >= options->max_num_iterations) {
        termination = 1;
        break;
      }
      if (linearised && last_step_successful && gradient_max <= kGradientTolerance) {
        termination = 0;
        break;
      }
      if (radius <= kMinRadius) {
        termination = 0;
        break;
      }
    }
    // this iteration's launches: the linearisation if x has moved, the step, the candidate; one read-back
    if (!linearised) {
      DLIOM_TRY(enqueue_linearise(&solver, iteration == 0));
      ++summary->num_residual_evaluations;
      ++summary->num_jacobian_evaluations;
    }
    DLIOM_TRY(enqueue_step(&solver, radius));
    double sums[kSums];
    DLIOM_TRY(read_sums(&solver, true, sums));
    if (!linearised) {
      linearised = true;
      x_cost = sums[kSumCost];
      fixed_cost = sums[kSumFixedCost];
      x_norm = std::sqrt(sums[kSumXSquared]);
      gradient_max = sums[kSumGradientMax];
      if (iteration == 0) {
        if (!std::isfinite(x_cost)) {  // "Initial residual and Jacobian evaluation failed."
          termination = 2;
          break;
        }
        summary->initial_cost = x_cost;
        minimum_cost = x_cost;
        iteration_costs.push_back(x_cost);
        minimum_cost_e = current_cost = reference_cost = candidate_cost_e = x_cost;
        if (gradient_max <= kGradientTolerance) {
          termination = 0;
          break;
        }
        if (options->max_num_iterations <= 0) {
          termination = 1;
          break;
        }
      } else if (gradient_max <= kGradientTolerance) {  // the previous, successful iteration's gradient test
        termination = 0;
        break;
      }
    }
    ++iteration;
    last_step_successful = false;
    // ComputeTrustRegionStep
    const bool solved = sums[kSumFlag] == 0.;
    if (!solved) ++summary->linear_solver_failures;
    const double model_cost_change = -sums[kSumModel];
    if (!solved || !(model_cost_change > 0.0)) {  // HandleInvalidStep
      if (++invalid_in_a_row >= kMaxInvalidSteps) {
        termination = 2;
        break;
      }
      radius *= 0.5;
      iteration_costs.push_back(x_cost);
      record(2);
      continue;
    }
    invalid_in_a_row = 0;
    ++summary->num_residual_evaluations;
    double candidate_cost = sums[kSumCandidateCost];
    if (!std::isfinite(candidate_cost)) candidate_cost = DBL_MAX;  // a failed evaluation: the step is rejected below
    const double step_norm = std::sqrt(sums[kSumStepSquared]);
    if (step_norm <= kParameterTolerance * (x_norm + kParameterTolerance)) {
      termination = 0;
      break;
    }
    if (std::fabs(x_cost - candidate_cost) <= kFunctionTolerance * x_cost) {
      termination = 0;
      break;
    }
    const double relative_decrease =
        std::max((current_cost - candidate_cost) / model_cost_change,
                 (reference_cost - candidate_cost) / (accumulated_reference + model_cost_change));
    if (relative_decrease > kMinRelativeDecrease) {  // HandleSuccessfulStep
      std::swap(g.x, g.candidate);
      linearised = false;
      x_cost = candidate_cost;  // the linearisation at the new x gives the same bits (same code, same order)
      last_step_successful = true;
      radius = std::min(kMaxRadius, radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * relative_decrease - 1.0, 3)));
      decrease_factor = 2.0;
      // TrustRegionStepEvaluator::StepAccepted
      current_cost = candidate_cost;
      accumulated_candidate += model_cost_change;
      accumulated_reference += model_cost_change;
      if (current_cost < minimum_cost_e) {
        minimum_cost_e = current_cost;
        consecutive_nonmonotonic = 0;
        candidate_cost_e = current_cost;
        accumulated_candidate = 0.0;
      } else {
        ++consecutive_nonmonotonic;
        if (current_cost > candidate_cost_e) {
          candidate_cost_e = current_cost;
          accumulated_candidate = 0.0;
        }
      }
      if (consecutive_nonmonotonic == max_nonmonotonic) {
        reference_cost = candidate_cost_e;
        accumulated_reference = accumulated_candidate;
      }
      iteration_costs.push_back(x_cost);
      record(1);
    } else {  // HandleUnsuccessfulStep
      radius /= decrease_factor;
      decrease_factor *= 2.0;
      iteration_costs.push_back(candidate_cost);
      record(0);
    }
  }
  summary->termination_type = termination;
  summary->num_iterations = static_cast<int>(iteration_costs.size());
  // solver.cc SetSummaryFinalCost: the minimum over the iterations, plus the fixed cost
  double final_cost = summary->initial_cost;
  for (double c : iteration_costs) final_cost = std::min(final_cost, c);
  summary->initial_cost += fixed_cost;
  summary->final_cost = final_cost + fixed_cost;
  int status = DLIOM_OK;
  if (termination == 2) {
    status = DLIOM_ERR_SOLVER;
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  } else {
    DLIOM_TRY(copy_poses_out(&solver, best, 7, num_submaps, num_nodes, submap_poses7, node_poses7,
                             terms != nullptr ? terms->fixed_frame_poses7 : nullptr,
                             landmarks != nullptr ? landmarks->landmark_poses7 : nullptr));
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  ++ctx->host_syncs;
  if (ctx->profiling) {
    summary->linearise_ms = solver.stage_ms[0];
    summary->eliminate_ms = solver.stage_ms[1];
    summary->factor_ms = solver.stage_ms[2];
    summary->back_substitute_ms = solver.stage_ms[3];
    const double total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - started).count();
    summary->host_ms = total - (solver.stage_ms[0] + solver.stage_ms[1] + solver.stage_ms[2] + solver.stage_ms[3]);
  }
  return status;
}
int dliom_pose_graph_solve_terms(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps, double* submap_poses7,
                                 const unsigned char* submap_constant, int gravity_aligned_submap, int num_nodes,
                                 double* node_poses7, const unsigned char* node_constant, int64_t num_constraints,
                                 const dliom_pose_graph_constraint* constraints, const dliom_pose_graph_terms* terms,
                                 dliom_pose_graph_summary* summary) {
  return dliom_pose_graph_solve_landmarks(ctx, options, num_submaps, submap_poses7, submap_constant, gravity_aligned_submap, num_nodes,
                                          node_poses7, node_constant, num_constraints, constraints, terms, nullptr, summary);
}
// GetInitialLandmarkPose (optimization_problem_3d.cc:106-122): Rigid3d::FromArrays(InterpolateNodes3D(...)) *
// landmark_to_tracking, on the host in double.
int dliom_pose_graph_initial_landmark_pose(const double* prev_pose7, const double* next_pose7, double t,
                                           const double* landmark_to_tracking7, double* out7) {
  if (prev_pose7 == nullptr || next_pose7 == nullptr || landmark_to_tracking7 == nullptr || out7 == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  const double* start = prev_pose7 + 3;
  const double* end = next_pose7 + 3;
  const double cos_theta = start[0] * end[0] + start[1] * end[1] + start[2] * end[2] + start[3] * end[3];
  const double abs_cos_theta = std::fabs(cos_theta);
  double prev_scale = 1. - t, next_scale = t;
  if (abs_cos_theta < 1. - 1e-5) {
    const double theta = std::acos(abs_cos_theta);
    const double sin_theta = std::sin(theta);
    prev_scale = std::sin((1. - t) * theta) / sin_theta;
    next_scale = std::sin(t * theta) / sin_theta;
  }
  if (cos_theta < 0.) next_scale = -next_scale;
  PoseD interpolated, observed;
  for (int k = 0; k < 4; ++k) interpolated.q[k] = prev_scale * start[k] + next_scale * end[k], observed.q[k] = landmark_to_tracking7[3 + k];
  for (int k = 0; k < 3; ++k) interpolated.t[k] = prev_pose7[k] + t * (next_pose7[k] - prev_pose7[k]), observed.t[k] = landmark_to_tracking7[k];
  const PoseD pose = pose_mul(interpolated, observed);
  for (int k = 0; k < 3; ++k) out7[k] = pose.t[k];
  for (int k = 0; k < 4; ++k) out7[3 + k] = pose.q[k];
  return DLIOM_OK;
}
int dliom_pose_graph_solve(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps, double* submap_poses7,
                           const unsigned char* submap_constant, int gravity_aligned_submap, int num_nodes,
                           double* node_poses7, const unsigned char* node_constant, int64_t num_constraints,
                           const dliom_pose_graph_constraint* constraints, dliom_pose_graph_summary* summary) {
  return dliom_pose_graph_solve_terms(ctx, options, num_submaps, submap_poses7, submap_constant, gravity_aligned_submap, num_nodes,
                                      node_poses7, node_constant, num_constraints, constraints, nullptr, summary);
}

}  // extern "C"
