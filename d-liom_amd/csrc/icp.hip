// Scan alignment by ICP (dliom.h "scan alignment by ICP"): pcl::IterativeClosestPoint as
// gen_ground_truth_by_ndt_match.cc:190-205 runs it, on the exact nearest-neighbour index of nn_index.hip.  The definition
// is stated once, in the header; the kernels and the host solve below follow it operation for operation.
//
// An iteration is: search (nn_index.hip), tree reduction, solve and decision, transform.
//   tree_reduce_kernel (tree_reduce.h)  the header's fixed tree over 2048 consecutive source indices a workgroup, sixteen
//                      quantities a leaf (IcpLeaves::leaf), whatever the launch geometry
//   icp_finish_kernel  one workgroup: the tree over the workgroups' partial sums (tree_finish), then the sums, the count
//                      and the search counters into the page-locked block (kPinIcpSums) and the completion word that
//                      wait_done() polls
//   the solve          on the host, in double (nothing in the compiler's documents says that double division and sqrt
//                      are correctly rounded on the device): one polled read-back an iteration, counted in the result
//   nn_transform_kernel (nn_index.hip)  p <- (float)(R p + t)
// The host decides after every iteration, so nothing is enqueued behind a decision and no kernel waits on another.
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "device_common.h"
#include "icp_internal.h"

namespace dliom {
namespace {

constexpr int kThreads = kTreeThreads;
static_assert(sizeof(IcpReadback) <= kPinIcpSums.bytes, "the read-back fits its region");

__global__ __launch_bounds__(kThreads) void icp_finish_kernel(double* partials, const int* __restrict__ counts, int P, int P2,
                                                              int* counters, const unsigned* max_sq, IcpReadback* out,
                                                              unsigned* done_word, unsigned done_seq) {
  icp_finish_body(partials, counts, P, P2, counters, max_sq, out);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence_system();
    *reinterpret_cast<volatile unsigned*>(done_word) = done_seq;
  }
}

__global__ __launch_bounds__(kThreads) void icp_max_norm_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                const float* __restrict__ z, int n, unsigned* max_sq) {
  const int i = static_cast<int>(blockIdx.x) * kThreads + threadIdx.x;
  note_kept(i < n ? norm_word(x[i], y[i], z[i]) : 0u, max_sq);
}

}  // namespace

// ---- the solve (dliom.h, Solve): IEEE double + - * / sqrt, a fixed count.  (These, the checks and icp_iterate are
// icp_internal.h's: icp_batch.hip runs the same ones per pair.)
void icp_solve(const double S[kIcpSums], long long n, double R[9], double t[3]) {
  const double dn = static_cast<double>(n);
  double cp[3], cq[3], H[3][3];
  for (int a = 0; a < 3; ++a) {
    cp[a] = S[a] / dn;
    cq[a] = S[3 + a] / dn;
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) H[a][b] = S[6 + 3 * a + b] - (S[a] * S[3 + b]) / dn;
  double A[4][4], V[4][4];
  A[0][0] = (H[0][0] + H[1][1]) + H[2][2];
  A[0][1] = H[1][2] - H[2][1];
  A[0][2] = H[2][0] - H[0][2];
  A[0][3] = H[0][1] - H[1][0];
  A[1][1] = (H[0][0] - H[1][1]) - H[2][2];
  A[1][2] = H[0][1] + H[1][0];
  A[1][3] = H[2][0] + H[0][2];
  A[2][2] = (H[1][1] - H[0][0]) - H[2][2];
  A[2][3] = H[1][2] + H[2][1];
  A[3][3] = (H[2][2] - H[0][0]) - H[1][1];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      if (c < r) A[r][c] = A[c][r];
      V[r][c] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < DLIOM_ICP_JACOBI_SWEEPS; ++sweep)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(tt * tt + 1.0);
        const double s = tt * c;
        A[p][p] = A[p][p] - tt * apq;
        A[q][q] = A[q][q] + tt * apq;
        A[p][q] = A[q][p] = 0.0;
        for (int r = 0; r < 4; ++r) {
          if (r != p && r != q) {
            const double arp = A[r][p], arq = A[r][q];
            A[r][p] = A[p][r] = c * arp - s * arq;
            A[r][q] = A[q][r] = s * arp + c * arq;
          }
          const double vrp = V[r][p], vrq = V[r][q];
          V[r][p] = c * vrp - s * vrq;
          V[r][q] = s * vrp + c * vrq;
        }
      }
  int best = 0;
  for (int c = 1; c < 4; ++c)
    if (A[c][c] > A[best][best]) best = c;
  double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
  const double norm = std::sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / norm;
  x = x / norm;
  y = y / norm;
  z = z / norm;
  R[0] = 1.0 - 2.0 * (y * y + z * z);
  R[1] = 2.0 * (x * y - z * w);
  R[2] = 2.0 * (x * z + y * w);
  R[3] = 2.0 * (x * y + z * w);
  R[4] = 1.0 - 2.0 * (x * x + z * z);
  R[5] = 2.0 * (y * z - x * w);
  R[6] = 2.0 * (x * z - y * w);
  R[7] = 2.0 * (y * z + x * w);
  R[8] = 1.0 - 2.0 * (x * x + y * y);
  for (int a = 0; a < 3; ++a) t[a] = cq[a] - ((R[3 * a] * cp[0] + R[3 * a + 1] * cp[1]) + R[3 * a + 2] * cp[2]);
}

// T <- [R t; 0 0 0 1] T
void icp_compose(const double R[9], const double t[3], double T[16]) {
  double out[16];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 4; ++b) {
      out[4 * a + b] = (R[3 * a] * T[b] + R[3 * a + 1] * T[4 + b]) + R[3 * a + 2] * T[8 + b];
      if (b == 3) out[4 * a + b] = out[4 * a + b] + t[a];
    }
  out[12] = out[13] = out[14] = 0.0;
  out[15] = 1.0;
  std::memcpy(T, out, sizeof(out));
}

Rigid12 rigid_of(const double R[9], const double t[3]) {
  Rigid12 m;
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) m.m[4 * a + b] = R[3 * a + b];
    m.m[4 * a + 3] = t[a];
  }
  return m;
}

bool icp_options_ok(const dliom_icp_options* o) {
  if (o == nullptr) return false;
  const double finite_ones[4] = {o->transformation_epsilon, o->euclidean_fitness_epsilon, o->rotation_epsilon, o->relative_mse_epsilon};
  for (double v : finite_ones)
    if (!std::isfinite(v) || v < 0.0) return false;
  if (std::isnan(o->max_correspondence_distance) || o->max_correspondence_distance < 0.0) return false;
  return o->maximum_iterations >= 0 && o->min_correspondences >= 3 && o->reserved == 0 &&
         (o->search == DLIOM_NN_AUTO || o->search == DLIOM_NN_BRUTE_FORCE);
}

// dliom.h: finite, last row 0 0 0 1, |R^T R - I| <= 1e-6 in every entry, det R > 0
bool icp_guess_ok(const double* g) {
  if (g == nullptr) return false;
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(g[k])) return false;
  if (g[12] != 0.0 || g[13] != 0.0 || g[14] != 0.0 || g[15] != 1.0) return false;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double dot = g[a] * g[b] + g[4 + a] * g[4 + b] + g[8 + a] * g[8 + b];
      if (!(std::fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-6)) return false;
    }
  const double det = g[0] * (g[5] * g[10] - g[6] * g[9]) - g[1] * (g[4] * g[10] - g[6] * g[8]) + g[2] * (g[4] * g[9] - g[5] * g[8]);
  return det > 0.0;
}

// dliom.h, Iteration and Convergence: iteration k of an alignment from the sums of its search.  false: fewer than
// min_correspondences (the loop ends, T and the points stay).  Else T and the result are brought up to date, (R, t) is
// what the points are to be moved by, and *ends says whether a criterion of Convergence held.
bool icp_iterate(const dliom_icp_options* options, const double sums[kIcpSums], long long n, int k, double* previous_mse,
                 dliom_icp_result* res, double R[9], double t[3], bool* ends) {
  res->correspondences = static_cast<int>(n);
  if (n < options->min_correspondences) {
    res->converged = 0;
    res->reason = DLIOM_ICP_NO_CORRESPONDENCES;
    return false;
  }
  icp_solve(sums, n, R, t);
  icp_compose(R, t, res->transform);
  const double mse = sums[15] / static_cast<double>(n);
  res->mse = mse;
  res->iterations = k;
  const double cosine = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double translation_sq = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
  const double change = std::fabs(mse - *previous_mse);
  int reason = DLIOM_ICP_NOT_CONVERGED;
  if (k >= options->maximum_iterations)
    reason = DLIOM_ICP_ITERATIONS;
  else if (cosine >= 1.0 - options->rotation_epsilon && translation_sq <= options->transformation_epsilon)
    reason = DLIOM_ICP_TRANSFORM;
  else if (change < options->euclidean_fitness_epsilon)
    reason = DLIOM_ICP_ABS_MSE;
  else if (change / *previous_mse < options->relative_mse_epsilon)
    reason = DLIOM_ICP_REL_MSE;
  *previous_mse = mse;
  *ends = reason != DLIOM_ICP_NOT_CONVERGED;
  if (*ends) {
    res->converged = 1;
    res->reason = reason;
  }
  return true;
}

size_t icp_work_bytes(int64_t n) {
  int P = 1, P2 = 1;
  tree_geometry(static_cast<int>(n), &P, &P2);
  const size_t per = align256(4 * static_cast<size_t>(std::max<int64_t>(n, 1)));
  return 8 * per + align256(static_cast<size_t>(P2) * kIcpSums * sizeof(double)) + align256(4 * static_cast<size_t>(P2));
}

namespace {

// The device arrays of one alignment or step, carved from the index's scratch
struct IcpWork {
  dliom_nn_index* index = nullptr;
  dliom_ctx* ctx = nullptr;
  int n = 0, P = 0, P2 = 1;
  int* counters = nullptr;
  unsigned* max_sq = nullptr;
  float *px = nullptr, *py = nullptr, *pz = nullptr;
  NnSearch search;
  double* partials = nullptr;
  int* counts = nullptr;
  bool timed = false;
  std::vector<hipEvent_t> events;  // five an iteration while timed: search | reduce | (host) | transform
  double solve_ms = 0.0;
  ~IcpWork() {
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
  }
  int mark() {
    if (!timed) return DLIOM_OK;
    hipEvent_t e = nullptr;
    DLIOM_HIP_TRY(hipEventCreate(&e));
    events.push_back(e);
    DLIOM_HIP_TRY(hipEventRecord(e, ctx->stream));
    return DLIOM_OK;
  }
};

int icp_carve(dliom_nn_index* index, int n, IcpWork* w) {
  w->index = index;
  w->ctx = nn_ctx(index);
  w->n = n;
  tree_geometry(n, &w->P, &w->P2);
  const size_t per = align256(4 * static_cast<size_t>(std::max(n, 1)));
  const size_t partial_bytes = align256(static_cast<size_t>(w->P2) * kIcpSums * sizeof(double));
  DevBuf* scratch = nn_scratch(index);
  DLIOM_TRY(scratch->reserve(256 + icp_work_bytes(n)));
  char* const base = scratch->as<char>();
  w->counters = reinterpret_cast<int*>(base);
  w->max_sq = reinterpret_cast<unsigned*>(base + 64);
  w->px = reinterpret_cast<float*>(base + 256);
  w->py = reinterpret_cast<float*>(base + 256 + per);
  w->pz = reinterpret_cast<float*>(base + 256 + 2 * per);
  w->search.px = w->px;
  w->search.py = w->py;
  w->search.pz = w->pz;
  w->search.n = n;
  w->search.j = reinterpret_cast<int*>(base + 256 + 3 * per);
  w->search.d2 = reinterpret_cast<float*>(base + 256 + 4 * per);
  w->search.list = reinterpret_cast<int*>(base + 256 + 5 * per);
  w->search.key = reinterpret_cast<unsigned long long*>(base + 256 + 6 * per);
  w->search.counters = w->counters;
  w->partials = reinterpret_cast<double*>(base + 256 + 8 * per);
  w->counts = reinterpret_cast<int*>(base + 256 + 8 * per + partial_bytes);
  const FillJob fill{base, 256, 0u};  // the counters and the norm word
  return fill_multi(w->ctx, &fill, 1);
}

// search, reduce, the polled read-back: the correspondences of the points in w->search and their sums
int icp_search_and_sum(IcpWork* w, double max_d2, int search, IcpReadback* out) {
  dliom_ctx* ctx = w->ctx;
  DLIOM_TRY(w->mark());
  DLIOM_TRY(nn_search_enqueue(w->index, w->search, max_d2, search));
  DLIOM_TRY(w->mark());
  const NnGridView g = nn_view(w->index);
  const IcpLeaves L{w->search.px, w->search.py, w->search.pz, w->search.j, w->search.d2, g.by_index, w->n};
  hipLaunchKernelGGL((tree_reduce_kernel<kIcpSums, IcpLeaves>), dim3(static_cast<unsigned>(w->P)), dim3(kThreads), 0, ctx->stream, L, w->partials, w->counts);
  DLIOM_HIP_TRY(hipGetLastError());
  IcpReadback* const host = pinned_at<IcpReadback>(ctx, kPinIcpSums);
  const unsigned seq = next_done_seq(ctx);
  const auto enqueued_at = std::chrono::steady_clock::now();
  hipLaunchKernelGGL(icp_finish_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, w->partials, w->counts, w->P, w->P2, w->counters,
                     w->max_sq, host, ctx->done_word, seq);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_TRY(w->mark());
  int* const poll_us = nn_poll_us(w->index);
  DLIOM_TRY(wait_done(ctx, ctx->stream, ctx->done_word, seq, *poll_us));
  const auto took = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - enqueued_at).count();
  *poll_us = static_cast<int>(std::min<long long>(std::max<long long>(2 * took, 150), 100000));
  *out = *host;
  return DLIOM_OK;
}

}  // namespace

// nn_index.h: the fitness score of n points in HBM (ndt.hip's final points): one search without a bound, one read-back
int icp_fitness_of(dliom_nn_index* index, const float* x, const float* y, const float* z, int n, double* score, long long* count) {
  IcpWork w;
  DLIOM_TRY(icp_carve(index, n, &w));
  if (n > 0) {
    DLIOM_HIP_TRY(hipMemcpyAsync(w.px, x, 4 * static_cast<size_t>(n), hipMemcpyDeviceToDevice, w.ctx->stream));
    DLIOM_HIP_TRY(hipMemcpyAsync(w.py, y, 4 * static_cast<size_t>(n), hipMemcpyDeviceToDevice, w.ctx->stream));
    DLIOM_HIP_TRY(hipMemcpyAsync(w.pz, z, 4 * static_cast<size_t>(n), hipMemcpyDeviceToDevice, w.ctx->stream));
  }
  IcpReadback rb;
  DLIOM_TRY(icp_search_and_sum(&w, std::numeric_limits<double>::infinity(), DLIOM_NN_AUTO, &rb));
  *count = rb.n;
  *score = rb.n > 0 ? rb.sums[15] / static_cast<double>(rb.n) : std::numeric_limits<double>::quiet_NaN();
  return DLIOM_OK;
}

}  // namespace dliom

extern "C" {

int dliom_icp_default_options(dliom_icp_options* options) {
  if (options == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *options = dliom_icp_options{30.0, 1e-6, 1e-6, 1e-5, 1e-5, 100, 3, DLIOM_NN_AUTO, 0};
  return DLIOM_OK;
}

int dliom_icp_align(dliom_nn_index* index, const dliom_cloud* source, const double* guess16, const dliom_icp_options* options,
                    dliom_icp_result* result, dliom_cloud** aligned) {
  using namespace dliom;
  if (aligned != nullptr) *aligned = nullptr;
  if (index == nullptr || source == nullptr || result == nullptr || !icp_options_ok(options) || !icp_guess_ok(guess16))
    return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_ctx* ctx = nn_ctx(index);
  if (source->ctx != ctx || source->n < 0 || source->n > DLIOM_NN_MAX_POINTS || ctx->done_word == nullptr)
    return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const int n = static_cast<int>(source->n);
  dliom_icp_result res = {};
  std::memcpy(res.transform, guess16, sizeof(res.transform));
  res.mse = std::numeric_limits<double>::infinity();
  res.fitness_score = std::numeric_limits<double>::quiet_NaN();
  IcpWork w;
  w.timed = ctx->profiling;
  DLIOM_TRY(icp_carve(index, n, &w));
  Rigid12 start;
  std::memcpy(start.m, guess16, sizeof(start.m));
  DLIOM_TRY(nn_transform_enqueue(ctx, source->d_x, source->d_y, source->d_z, n, start, w.px, w.py, w.pz));
  const double D = options->max_correspondence_distance;
  const double max_d2 = D * D;
  double previous_mse = std::numeric_limits<double>::infinity();
  IcpReadback rb;
  for (int k = 1;; ++k) {
    DLIOM_TRY(icp_search_and_sum(&w, max_d2, options->search, &rb));
    ++res.read_backs;
    const auto solve_from = std::chrono::steady_clock::now();
    double R[9], t[3];
    bool ends = false;
    if (!icp_iterate(options, rb.sums, rb.n, k, &previous_mse, &res, R, t, &ends)) {
      if (w.timed) {  // keeps the events in fives
        DLIOM_TRY(w.mark());
        DLIOM_TRY(w.mark());
      }
      break;
    }
    w.solve_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - solve_from).count();
    DLIOM_TRY(w.mark());
    DLIOM_TRY(nn_transform_enqueue(ctx, w.px, w.py, w.pz, n, rigid_of(R, t), w.px, w.py, w.pz));
    DLIOM_TRY(w.mark());
    if (ends) break;
  }
  // the fitness score: one more search without a bound (and the aligned cloud's norm bound in the same read-back)
  const size_t loop_events = w.events.size();
  if (aligned != nullptr && n > 0) {
    hipLaunchKernelGGL(icp_max_norm_kernel, dim3(blocks_of(n, kThreads)), dim3(kThreads), 0, ctx->stream, w.px, w.py, w.pz, n, w.max_sq);
    DLIOM_HIP_TRY(hipGetLastError());
  }
  w.timed = false;
  DLIOM_TRY(icp_search_and_sum(&w, std::numeric_limits<double>::infinity(), options->search, &rb));
  ++res.read_backs;
  res.fitness_count = rb.n;
  if (rb.n > 0) res.fitness_score = rb.sums[15] / static_cast<double>(rb.n);
  res.settled_by_grid = rb.counters[kNnByGrid];
  res.settled_by_brute_force = rb.counters[kNnByBruteForce];
  if (loop_events > 0) {
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t e = 0; e + 4 < loop_events; e += 5) {
      float ms[3] = {0.f, 0.f, 0.f};
      DLIOM_HIP_TRY(hipEventElapsedTime(&ms[0], w.events[e], w.events[e + 1]));
      DLIOM_HIP_TRY(hipEventElapsedTime(&ms[1], w.events[e + 1], w.events[e + 2]));
      DLIOM_HIP_TRY(hipEventElapsedTime(&ms[2], w.events[e + 3], w.events[e + 4]));
      res.search_ms += ms[0];
      res.reduce_ms += ms[1];
      res.transform_ms += ms[2];
    }
    res.solve_ms = w.solve_ms;
  }
  if (aligned != nullptr) {
    float *x, *y, *z;
    dliom_cloud* cloud = nullptr;
    DLIOM_TRY(alloc_device_cloud(ctx, n, &cloud, &x, &y, &z));
    float max_sq;
    std::memcpy(&max_sq, &rb.max_sq, 4);
    int st = finish_device_cloud_from(ctx, cloud, std::sqrt(max_sq), w.px, w.py, w.pz);
    if (st == DLIOM_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = DLIOM_ERR_HIP;  // the scratch is free again
    ++ctx->host_syncs;
    if (st != DLIOM_OK) {
      dliom_cloud_destroy(cloud);
      return st;
    }
    *aligned = cloud;
  }
  *result = res;
  return DLIOM_OK;
}

int dliom_icp_step(dliom_nn_index* index, const dliom_cloud* points, const dliom_icp_options* options, int32_t* j_out,
                   float* d2_out, double* sums16, int64_t* correspondences, double* rotation9, double* translation3) {
  using namespace dliom;
  if (index == nullptr || points == nullptr || !icp_options_ok(options) || sums16 == nullptr || correspondences == nullptr ||
      rotation9 == nullptr || translation3 == nullptr)
    return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_ctx* ctx = nn_ctx(index);
  if (points->ctx != ctx || points->n < 0 || points->n > DLIOM_NN_MAX_POINTS || ctx->done_word == nullptr ||
      (points->n > 0 && (j_out == nullptr || d2_out == nullptr)))
    return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const int n = static_cast<int>(points->n);
  IcpWork w;
  DLIOM_TRY(icp_carve(index, n, &w));
  w.search.px = points->d_x;
  w.search.py = points->d_y;
  w.search.pz = points->d_z;
  IcpReadback rb;
  const double D = options->max_correspondence_distance;
  DLIOM_TRY(icp_search_and_sum(&w, D * D, options->search, &rb));
  if (n > 0) {
    DLIOM_HIP_TRY(hipMemcpyAsync(j_out, w.search.j, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipMemcpyAsync(d2_out, w.search.d2, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    ++ctx->host_syncs;
  }
  std::memcpy(sums16, rb.sums, sizeof(rb.sums));
  *correspondences = rb.n;
  const double identity[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  std::memcpy(rotation9, identity, sizeof(identity));
  translation3[0] = translation3[1] = translation3[2] = 0.0;
  if (rb.n >= options->min_correspondences) icp_solve(rb.sums, rb.n, rotation9, translation3);
  return DLIOM_OK;
}

}  // extern "C"
