// Scan alignment by NDT (dliom.h "scan alignment by NDT"): pcl::NormalDistributionsTransform as
// LocalTrajectoryBuilder3D::MatchByNDT and gen_ground_truth_by_ndt_match.cc's `--method ndt` run it.  The definition is
// stated once, in the header; the kernels and the host steps below follow it operation for operation.
//
// The target (dliom_ndt_target_create):
//   ndt_key_kernel      a lane a target point: its 63-bit cell key (z high, x low), or the skip key
//   hipcub radix sort   stable, by key: a cell's points come out in ascending point index
//   ndt_head_kernel     segment heads; their inclusive sum numbers the cells; ndt_bounds_kernel writes each cell's first
//                       position and key
//   ndt_cell_sums_kernel  a workgroup a cell: n and the nine sums in the header's fixed tree -- 256 leaves at a time
//                       through LDS, longer cells in aligned chunks of 256 whose partial sums meet in a binary counter
//                       (the same tree, whatever the cell's length)
//   the per-cell step   on the host, in double (division and sqrt, as ICP's solve): mean, covariance, Jacobi, icov; the
//                       valid cells' keys, means and icov go back up once, sorted by key
// An evaluation (the hot path):
//   ndt_eval_kernel<G, H>  a lane a source point: transform, nine binary searches (a row of three x-neighbours is
//                       contiguous in key order), the 7 / 21 / 28 values in registers in the header's order, then one
//                       store a value into the leaf arrays in HBM (224 B a point at most)
//   tree_reduce_kernel (tree_reduce.h) and ndt_finish_kernel  ICP's fixed tree over the source index; the sums and the
//                       pair count into the page-locked block (kPinNdtSums) and the completion word: one polled read-back
// The pseudo-inverse, the step length and every decision run on the host between evaluations: NdtAlignment, a state machine
// that takes an evaluation's sums and gives the next evaluation to run.  dliom_ndt_align drives one of it and blocks on
// every evaluation; ndt_batch.hip drives one per pair, a round at a time.  The kernels' bodies are ndt_internal.h's.
// A stream of scans (dliom_ndt_scan_matcher, MatchByNDT as InitilizeByNDT calls it): each scan through the approximate
// voxel grid (approx_voxel.hip) once, aligned to the cells its predecessor left, then its own cells built and kept.
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "ndt_internal.h"

struct dliom_ndt_scan_matcher {
  dliom_ctx* ctx;
  dliom_ndt_options options;
  float leaf;
  dliom_ndt_target* target;  // the previous scan's cells (null before the first scan)
};

namespace dliom {
namespace {

constexpr int kThreads = kNdtThreads;
constexpr int kHalf = kNdtHalf;

// ---- the target (ndt_internal.h: the bodies, which a chunk of ndt_target_batch.hip runs too) ---------------------------------
__global__ __launch_bounds__(kThreads) void ndt_key_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ z, int n, float inv,
                                                           unsigned long long* __restrict__ keys, int* __restrict__ index) {
  const int i = static_cast<int>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  keys[i] = ndt_key_body(x, y, z, i, inv);
  index[i] = i;
}

__global__ __launch_bounds__(kThreads) void ndt_head_kernel(const unsigned long long* __restrict__ keys, int n,
                                                            unsigned* __restrict__ head, unsigned* __restrict__ kept) {
  const int i = static_cast<int>(blockIdx.x) * kThreads + threadIdx.x;
  if (i < n) ndt_head_body(keys, i, head, kept);
}

__global__ __launch_bounds__(kThreads) void ndt_bounds_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ head,
                                                              const unsigned* __restrict__ inclusive, int n, int cells, int kept,
                                                              int* __restrict__ cell_first, unsigned long long* __restrict__ cell_key) {
  ndt_bounds_body(keys, head, inclusive, 0u, static_cast<int>(blockIdx.x) * kThreads + threadIdx.x, n, cells, kept, cell_first, cell_key);
}

// sums: cells x 9
__global__ __launch_bounds__(kThreads) void ndt_cell_sums_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                 const float* __restrict__ z, const int* __restrict__ sorted_index,
                                                                 const int* __restrict__ cell_first, double* __restrict__ sums) {
  const int c = static_cast<int>(blockIdx.x);
  const int first = cell_first[c];
  ndt_cell_sums_body(x, y, z, sorted_index, first, cell_first[c + 1] - first, sums + static_cast<size_t>(c) * 9);
}

// ---- the evaluation (ndt_internal.h: the table, the pose's rows, the body, the leaves and the read-back) --------------------
template <bool G, bool H>
__global__ __launch_bounds__(kThreads) void ndt_eval_kernel(NdtTable T, NdtPose P, const float* __restrict__ sx, const float* __restrict__ sy,
                                                            const float* __restrict__ sz, int n, double* __restrict__ leaves,
                                                            int* __restrict__ pairs) {
  ndt_eval_body<G, H>(T, P, sx, sy, sz, n, leaves, pairs, static_cast<int>(blockIdx.x));
}

template <int S>
__global__ __launch_bounds__(kTreeThreads) void ndt_finish_kernel(double* partials, const int* __restrict__ counts, int P, int P2,
                                                                  NdtReadback* out, unsigned* done_word, unsigned done_seq) {
  ndt_finish_body<S>(partials, counts, P, P2, out);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence_system();
    *reinterpret_cast<volatile unsigned*>(done_word) = done_seq;
  }
}

__global__ __launch_bounds__(kThreads) void ndt_max_norm_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                const float* __restrict__ z, int n, unsigned* max_sq) {
  const int i = static_cast<int>(blockIdx.x) * kThreads + threadIdx.x;
  note_kept(i < n ? norm_word(x[i], y[i], z[i]) : 0u, max_sq);
}

// ---- host steps ----------------------------------------------------------------------------------------------------------
// Cyclic Jacobi with ICP's rotation rule on a symmetric N x N; the eigenvalues are left on A's diagonal
template <int N>
void jacobi(double A[N][N], double V[N][N], int sweeps) {
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < N; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < sweeps; ++sweep)
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(tt * tt + 1.0);
        const double s = tt * c;
        A[p][p] = A[p][p] - tt * apq;
        A[q][q] = A[q][q] + tt * apq;
        A[p][q] = A[q][p] = 0.0;
        for (int r = 0; r < N; ++r) {
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
}

// dliom.h, target cells: mean, covariance, eigen-decomposition, icov, validity
void ndt_finish_cell(const double S[9], int min_points, dliom_ndt_cell* cell) {
  const double dn = static_cast<double>(cell->n);
  for (int a = 0; a < 3; ++a) cell->mean[a] = S[a] / dn;
  for (double& v : cell->icov) v = 0.0;
  cell->valid = 0;
  if (cell->n < min_points) return;
  const int at[3][3] = {{3, 4, 5}, {4, 6, 7}, {5, 7, 8}};
  double C[3][3], V[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b)
      C[a][b] = C[b][a] = ((S[at[a][b]] - 2.0 * (S[a] * cell->mean[b])) / dn + cell->mean[a] * cell->mean[b]) * ((dn - 1.0) / dn);
  jacobi<3>(C, V, DLIOM_NDT_JACOBI_SWEEPS);
  int order[3] = {0, 1, 2};
  for (int a = 1; a < 3; ++a)  // stable insertion sort
    for (int b = a; b > 0 && C[order[b]][order[b]] < C[order[b - 1]][order[b - 1]]; --b) std::swap(order[b], order[b - 1]);
  double l[3] = {C[order[0]][order[0]], C[order[1]][order[1]], C[order[2]][order[2]]};
  if (!(l[0] >= 0.0 && l[1] >= 0.0 && l[2] > 0.0)) return;
  const double least = 0.01 * l[2];
  if (l[0] < least) l[0] = least;
  if (l[1] < least) l[1] = least;
  double icov[6];
  int k = 0;
  bool finite = true;
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) {
      icov[k] = ((V[a][order[0]] * V[b][order[0]]) / l[0] + (V[a][order[1]] * V[b][order[1]]) / l[1]) +
                (V[a][order[2]] * V[b][order[2]]) / l[2];
      finite = finite && std::isfinite(icov[k]);
      ++k;
    }
  if (!finite) return;
  std::memcpy(cell->icov, icov, sizeof(icov));
  cell->valid = 1;
}

}  // namespace

void ndt_pose(const double p[6], NdtPose* P) {
  const double sa = std::sin(p[3]), ca = std::cos(p[3]), sb = std::sin(p[4]), cb = std::cos(p[4]), sc = std::sin(p[5]),
               cc = std::cos(p[5]);
  std::memset(P, 0, sizeof(*P));
  const double R[9] = {cb * cc, -(cb * sc), sb, ca * sc + sa * sb * cc, ca * cc - sa * sb * sc, -(sa * cb),
                       sa * sc - ca * sb * cc, sa * cc + ca * sb * sc, ca * cb};
  std::memcpy(P->R, R, sizeof(R));
  for (int a = 0; a < 3; ++a) P->t[a] = p[a];
  auto set = [](double row[3], double k0, double k1, double k2) {
    row[0] = k0;
    row[1] = k1;
    row[2] = k2;
  };
  set(P->J[0][1], -(sa * sc) + ca * sb * cc, -(sa * cc) - ca * sb * sc, -(ca * cb));
  set(P->J[0][2], ca * sc + sa * sb * cc, ca * cc - sa * sb * sc, -(sa * cb));
  set(P->J[1][0], -(sb * cc), sb * sc, cb);
  set(P->J[1][1], sa * cb * cc, -(sa * cb * sc), sa * sb);
  set(P->J[1][2], -(ca * cb * cc), ca * cb * sc, -(ca * sb));
  set(P->J[2][0], -(cb * sc), -(cb * cc), 0.0);
  set(P->J[2][1], ca * cc - sa * sb * sc, -(ca * sc) - sa * sb * cc, 0.0);
  set(P->J[2][2], sa * cc + ca * sb * sc, -(sa * sc) + ca * sb * cc, 0.0);
  set(P->H[0][1], -(ca * sc) - sa * sb * cc, -(ca * cc) + sa * sb * sc, sa * cb);
  set(P->H[0][2], -(sa * sc) + ca * sb * cc, -(sa * cc) - ca * sb * sc, -(ca * cb));
  set(P->H[1][1], ca * cb * cc, -(ca * cb * sc), ca * sb);
  set(P->H[1][2], sa * cb * cc, -(sa * cb * sc), sa * sb);
  set(P->H[2][1], -(sa * cc) - ca * sb * sc, sa * sc - ca * sb * cc, 0.0);
  set(P->H[2][2], ca * cc - sa * sb * sc, -(ca * sc) - sa * sb * cc, 0.0);
  set(P->H[3][0], -(cb * cc), cb * sc, -sb);
  set(P->H[3][1], -(sa * sb * cc), sa * sb * sc, sa * cb);
  set(P->H[3][2], ca * sb * cc, -(ca * sb * sc), -(ca * cb));
  set(P->H[4][0], sb * sc, sb * cc, 0.0);
  set(P->H[4][1], -(sa * cb * sc), -(sa * cb * cc), 0.0);
  set(P->H[4][2], ca * cb * sc, ca * cb * cc, 0.0);
  set(P->H[5][0], -(cb * cc), cb * sc, 0.0);
  set(P->H[5][1], -(ca * sc) - sa * sb * cc, -(ca * cc) + sa * sb * sc, 0.0);
  set(P->H[5][2], -(sa * sc) + ca * sb * cc, -(sa * cc) - ca * sb * sc, 0.0);
}

NdtConstants ndt_constants(const dliom_ndt_options& o) {
  const double c1 = 10.0 * (1.0 - o.outlier_ratio);
  const double c2 = o.outlier_ratio / ((o.resolution * o.resolution) * o.resolution);
  const double d3 = -std::log(c2);
  const double d1 = -std::log(c1 + c2) - d3;
  const double d2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / d1);
  return NdtConstants{d1, d2};
}

bool ndt_options_ok(const dliom_ndt_options* o) {
  if (o == nullptr) return false;
  if (!std::isfinite(o->resolution) || o->resolution <= 0.0 || !std::isfinite(o->step_size) || o->step_size <= 0.0) return false;
  if (!(o->outlier_ratio > 0.0 && o->outlier_ratio < 1.0)) return false;
  if (!std::isfinite(o->transformation_epsilon) || o->transformation_epsilon < 0.0) return false;
  return o->maximum_iterations >= 0 && o->min_points_per_voxel >= 3 && o->reserved == 0 &&
         (o->step_mode == DLIOM_NDT_STEP_CLAMPED || o->step_mode == DLIOM_NDT_STEP_MORE_THUENTE);
}

// dliom.h (ICP): finite, last row 0 0 0 1, |R^T R - I| <= 1e-6 in every entry, det R > 0
bool ndt_guess_ok(const double* g) {
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

NdtTable ndt_table_of(const dliom_ndt_target* t, const NdtConstants& k) {
  const float res = static_cast<float>(t->resolution);
  return NdtTable{t->table.as<unsigned long long>(),
                  reinterpret_cast<const double*>(t->table.as<char>() + t->cell_data_at),
                  static_cast<int>(t->n_valid),
                  1.0f / res,
                  res * res,
                  k.d1,
                  k.d2};
}

void ndt_finish_cells(dliom_ndt_target* t, int cells, const int* first, const unsigned long long* key, const double* sums,
                      NdtValidCells* valid) {
  t->cells.resize(cells);
  for (int c = 0; c < cells; ++c) {
    dliom_ndt_cell& cell = t->cells[c];
    cell.index[0] = static_cast<int>(key[c] & 0x1fffffu) - kHalf;
    cell.index[1] = static_cast<int>((key[c] >> 21) & 0x1fffffu) - kHalf;
    cell.index[2] = static_cast<int>((key[c] >> 42) & 0x1fffffu) - kHalf;
    cell.n = first[c + 1] - first[c];
    ndt_finish_cell(&sums[static_cast<size_t>(c) * 9], t->min_points, &cell);
    if (cell.valid != 0) {
      valid->keys.push_back(key[c]);
      valid->data.insert(valid->data.end(), cell.mean, cell.mean + 3);
      valid->data.insert(valid->data.end(), cell.icov, cell.icov + 6);
    }
  }
}

int ndt_table_upload_enqueue(dliom_ndt_target* t, const NdtValidCells& valid) {
  t->n_valid = static_cast<int64_t>(valid.keys.size());
  t->cell_data_at = align256(8 * std::max<size_t>(valid.keys.size(), 1));
  DLIOM_TRY(t->table.reserve(t->cell_data_at + 72 * std::max<size_t>(valid.keys.size(), 1)));
  if (valid.keys.empty()) return DLIOM_OK;
  hipStream_t stream = t->ctx->stream;
  if (hipMemcpyAsync(t->table.p, valid.keys.data(), 8 * valid.keys.size(), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(t->table.as<char>() + t->cell_data_at, valid.data.data(), 8 * valid.data.size(), hipMemcpyHostToDevice, stream) !=
          hipSuccess)
    return DLIOM_ERR_HIP;
  return DLIOM_OK;
}

void ndt_unpack(const NdtReadback& rb, int what, NdtSums* out) {
  int at = 0;
  if (what != DLIOM_NDT_EVAL_HESSIAN) {
    out->score = rb.sums[0];
    for (int a = 0; a < 6; ++a) out->g[a] = rb.sums[1 + a];
    at = 7;
  }
  if (what != DLIOM_NDT_EVAL_GRADIENT)
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) out->H[a][b] = out->H[b][a] = rb.sums[at++];
  out->pairs = rb.pairs;
}

// delta = -pinv(H) g (dliom.h, Alignment 1)
void ndt_newton_step(const NdtSums& s, double delta[6]) {
  double A[6][6], V[6][6];
  std::memcpy(A, s.H, sizeof(A));
  jacobi<6>(A, V, DLIOM_NDT_PINV_SWEEPS);
  double largest = 0.0;
  for (int k = 0; k < 6; ++k)
    if (std::fabs(A[k][k]) > largest) largest = std::fabs(A[k][k]);
  const double floor_ = 6.0 * 0x1p-52 * largest;
  double z[6];
  for (int k = 0; k < 6; ++k) {
    double y = 0.0;
    for (int r = 0; r < 6; ++r) y = y + V[r][k] * s.g[r];
    z[k] = std::fabs(A[k][k]) > floor_ ? y / A[k][k] : 0.0;
  }
  for (int r = 0; r < 6; ++r) {
    double v = 0.0;
    for (int k = 0; k < 6; ++k) v = v + V[r][k] * z[k];
    delta[r] = -v;
  }
}

namespace {

// One evaluation's work on the stream and its read-back.  Events (while timed): before | after the evaluation kernel |
// after the reduction.
struct NdtRun {
  dliom_ndt_target* target;
  const dliom_cloud* source;
  NdtConstants k;
  bool timed = false;
  std::vector<hipEvent_t> events;
  int64_t read_backs = 0;
  ~NdtRun() {
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
  }
  int mark() {
    if (!timed) return DLIOM_OK;
    hipEvent_t e = nullptr;
    DLIOM_HIP_TRY(hipEventCreate(&e));
    events.push_back(e);
    DLIOM_HIP_TRY(hipEventRecord(e, target->ctx->stream));
    return DLIOM_OK;
  }
  template <bool G, bool H>
  int run(const NdtPose& P, NdtReadback* out);
  // *out keeps what this kind of evaluation does not compute
  int evaluate(const double p[6], int what, NdtSums* out) {
    NdtPose P;
    ndt_pose(p, &P);
    NdtReadback rb;
    if (what == DLIOM_NDT_EVAL_GRADIENT)
      DLIOM_TRY((run<true, false>(P, &rb)));
    else if (what == DLIOM_NDT_EVAL_ALL)
      DLIOM_TRY((run<true, true>(P, &rb)));
    else
      DLIOM_TRY((run<false, true>(P, &rb)));
    ndt_unpack(rb, what, out);
    return DLIOM_OK;
  }
};

template <bool G, bool H>
int NdtRun::run(const NdtPose& P, NdtReadback* out) {
  constexpr int S = ndt_sums(G, H);
  dliom_ndt_target* const t = target;
  dliom_ctx* const ctx = t->ctx;
  const int n = static_cast<int>(source->n);
  int blocks = 0, P2 = 1;
  tree_geometry(n, &blocks, &P2);
  const size_t leaf_bytes = align256(static_cast<size_t>(S) * std::max(n, 1) * sizeof(double));
  const size_t pair_bytes = align256(4 * static_cast<size_t>(std::max(n, 1)));
  const size_t partial_bytes = align256(static_cast<size_t>(P2) * S * sizeof(double));
  DLIOM_TRY(t->scratch.reserve(leaf_bytes + pair_bytes + partial_bytes + align256(4 * static_cast<size_t>(P2))));
  char* const base = t->scratch.as<char>();
  double* const leaves = reinterpret_cast<double*>(base);
  int* const pairs = reinterpret_cast<int*>(base + leaf_bytes);
  double* const partials = reinterpret_cast<double*>(base + leaf_bytes + pair_bytes);
  int* const counts = reinterpret_cast<int*>(base + leaf_bytes + pair_bytes + partial_bytes);
  const NdtTable table = ndt_table_of(t, k);
  DLIOM_TRY(mark());
  if (n > 0) {
    hipLaunchKernelGGL((ndt_eval_kernel<G, H>), dim3(blocks_of(n, kThreads)), dim3(kThreads), 0, ctx->stream, table, P, source->d_x,
                       source->d_y, source->d_z, n, leaves, pairs);
    DLIOM_HIP_TRY(hipGetLastError());
  }
  DLIOM_TRY(mark());
  const NdtLeaves<S> L{leaves, pairs, n};
  hipLaunchKernelGGL((tree_reduce_kernel<S, NdtLeaves<S>>), dim3(static_cast<unsigned>(blocks)), dim3(kTreeThreads), 0, ctx->stream, L,
                     partials, counts);
  DLIOM_HIP_TRY(hipGetLastError());
  NdtReadback* const host = pinned_at<NdtReadback>(ctx, kPinNdtSums);
  const unsigned seq = next_done_seq(ctx);
  const auto enqueued_at = std::chrono::steady_clock::now();
  hipLaunchKernelGGL((ndt_finish_kernel<S>), dim3(1), dim3(kTreeThreads), 0, ctx->stream, partials, counts, blocks, P2, host,
                     ctx->done_word, seq);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_TRY(mark());
  DLIOM_TRY(wait_done(ctx, ctx->stream, ctx->done_word, seq, t->poll_us));
  const auto took = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - enqueued_at).count();
  t->poll_us = static_cast<int>(std::min<long long>(std::max<long long>(2 * took, 150), 100000));
  ++read_backs;
  *out = *host;
  return DLIOM_OK;
}

inline double min_of(double a, double b) { return b < a ? b : a; }
inline double max_of(double a, double b) { return a < b ? b : a; }

double mt_trial(double a_l, double f_l, double g_l, double a_u, double f_u, double g_u, double a_t, double f_t, double g_t) {
  if (f_t > f_l) {
    const double z = (3.0 * (f_t - f_l) / (a_t - a_l) - g_t) - g_l;
    const double w = std::sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * ((w - g_l) - z) / ((g_t - g_l) + 2.0 * w);
    const double a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t));
    return std::fabs(a_c - a_l) < std::fabs(a_q - a_l) ? a_c : 0.5 * (a_q + a_c);
  }
  if (g_t * g_l < 0.0) {
    const double z = (3.0 * (f_t - f_l) / (a_t - a_l) - g_t) - g_l;
    const double w = std::sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * ((w - g_l) - z) / ((g_t - g_l) + 2.0 * w);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    return std::fabs(a_c - a_t) >= std::fabs(a_s - a_t) ? a_c : a_s;
  }
  if (std::fabs(g_t) <= std::fabs(g_l)) {
    const double z = (3.0 * (f_t - f_l) / (a_t - a_l) - g_t) - g_l;
    const double w = std::sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * ((w - g_l) - z) / ((g_t - g_l) + 2.0 * w);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    const double next = std::fabs(a_c - a_t) < std::fabs(a_s - a_t) ? a_c : a_s;
    return a_t > a_l ? min_of(a_t + 0.66 * (a_u - a_t), next) : max_of(a_t + 0.66 * (a_u - a_t), next);
  }
  const double z = (3.0 * (f_t - f_u) / (a_t - a_u) - g_t) - g_u;
  const double w = std::sqrt(z * z - g_t * g_u);
  return a_u + (a_t - a_u) * ((w - g_u) - z) / ((g_t - g_u) + 2.0 * w);
}

// -> converged
bool mt_update(double* a_l, double* f_l, double* g_l, double* a_u, double* f_u, double* g_u, double a_t, double f_t, double g_t) {
  if (f_t > *f_l) {
    *a_u = a_t;
    *f_u = f_t;
    *g_u = g_t;
    return false;
  }
  if (g_t * (*a_l - a_t) > 0.0) {
    *a_l = a_t;
    *f_l = f_t;
    *g_l = g_t;
    return false;
  }
  if (g_t * (*a_l - a_t) < 0.0) {
    *a_u = *a_l;
    *f_u = *f_l;
    *g_u = *g_l;
    *a_l = a_t;
    *f_l = f_t;
    *g_l = g_t;
    return false;
  }
  return true;
}

double dot6(const double a[6], const double b[6]) {
  double v = 0.0;
  for (int r = 0; r < 6; ++r) v = v + a[r] * b[r];
  return v;
}

void ndt_pose_of_guess(const double* g, double p[6]) {
  p[0] = g[3];
  p[1] = g[7];
  p[2] = g[11];
  p[3] = std::atan2(-g[6], g[10]);
  p[4] = std::atan2(g[2], std::sqrt(g[0] * g[0] + g[1] * g[1]));
  p[5] = std::atan2(-g[4 * 0 + 1], g[0]);
}

bool ndt_call_ok(const dliom_ndt_target* target, const dliom_cloud* source, const dliom_ndt_options* options) {
  if (target == nullptr || source == nullptr || !ndt_options_ok(options)) return false;
  if (source->ctx != target->ctx || source->n < 0 || source->n > DLIOM_NN_MAX_POINTS || target->ctx->done_word == nullptr) return false;
  return options->resolution == target->resolution;
}

}  // namespace

// ---- dliom.h's ALIGNMENT and STEP LENGTH, between evaluations (ndt_internal.h) ----------------------------------------------
void NdtAlignment::ask(int what, NdtRequest* next) {
  if (what == DLIOM_NDT_EVAL_GRADIENT)
    ++without_hessian_;
  else
    ++with_hessian_;
  next->what = what;
}

void NdtAlignment::start(const dliom_ndt_options& options, const double guess16[16], NdtRequest* first) {
  *this = NdtAlignment();
  o_ = options;
  ndt_pose_of_guess(guess16, p_);
  std::memcpy(first->p, p_, sizeof(p_));
  ask(DLIOM_NDT_EVAL_ALL, first);
  phase_ = kGuess;
}

bool NdtAlignment::advance(const NdtSums& sums, NdtRequest* next) {
  const double mu = 1e-4;
  sums_ = sums;
  switch (phase_) {
    case kGuess:
      return begin_iteration(next);
    case kFirstTrial:  // the clamped first trial's evaluation, with the Hessian
      if (o_.step_mode == DLIOM_NDT_STEP_CLAMPED) return end_step(a_t_, next);
      a_l_ = a_u_ = f_l_ = f_u_ = 0.0;
      g_l_ = g_u_ = dphi0_ - mu * dphi0_;
      open_ = true;
      interval_converged_ = false;
      phi_t_ = -sums_.score;
      dphi_t_ = -dot6(sums_.g, dir_);
      psi_t_ = (phi_t_ - phi0_) - (mu * dphi0_) * a_t_;
      dpsi_t_ = dphi_t_ - mu * dphi0_;
      trials_ = 0;
      return more_trials(next);
    case kTrial:  // a trial's evaluation, without the Hessian
      phi_t_ = -sums_.score;
      dphi_t_ = -dot6(sums_.g, dir_);
      psi_t_ = (phi_t_ - phi0_) - (mu * dphi0_) * a_t_;
      dpsi_t_ = dphi_t_ - mu * dphi0_;
      if (open_ && psi_t_ <= 0.0 && dpsi_t_ >= 0.0) {
        open_ = false;
        f_l_ = (f_l_ + phi0_) - (mu * dphi0_) * a_l_;
        g_l_ = g_l_ + mu * dphi0_;
        f_u_ = (f_u_ + phi0_) - (mu * dphi0_) * a_u_;
        g_u_ = g_u_ + mu * dphi0_;
      }
      interval_converged_ = open_ ? mt_update(&a_l_, &f_l_, &g_l_, &a_u_, &f_u_, &g_u_, a_t_, psi_t_, dpsi_t_)
                                  : mt_update(&a_l_, &f_l_, &g_l_, &a_u_, &f_u_, &g_u_, a_t_, phi_t_, dphi_t_);
      ++trials_;
      return more_trials(next);
    case kHessianOnly:
      return end_step(a_t_, next);
    case kDone:
      break;
  }
  return false;
}

// Alignment 1 to 3, up to the step's first evaluation
bool NdtAlignment::begin_iteration(NdtRequest* next) {
  for (;;) {
    double delta[6];
    ndt_newton_step(sums_, delta);
    const double s = std::sqrt(dot6(delta, delta));
    if (s == 0.0 || s != s) {
      converged_ = s == s ? 1 : 0;
      reason_ = DLIOM_NDT_ZERO_STEP;
      iterations_ = it_;
      phase_ = kDone;
      return false;
    }
    for (int r = 0; r < 6; ++r) dir_[r] = delta[r] / s;
    const double step_max = o_.step_size, step_min = o_.transformation_epsilon / 2.0;
    phi0_ = -sums_.score;
    dphi0_ = -dot6(sums_.g, dir_);
    if (dphi0_ == 0.0) {  // a step of length 0: nothing is evaluated
      if (moved_and_done(0.0)) return false;
      continue;
    }
    if (dphi0_ > 0.0) {
      dphi0_ = -dphi0_;
      for (int r = 0; r < 6; ++r) dir_[r] = -dir_[r];
    }
    a_t_ = max_of(min_of(s, step_max), step_min);
    for (int r = 0; r < 6; ++r) x_[r] = p_[r] + dir_[r] * a_t_;
    std::memcpy(next->p, x_, sizeof(x_));
    ask(DLIOM_NDT_EVAL_ALL, next);
    phase_ = kFirstTrial;
    return true;
  }
}

// the More-Thuente loop's test and the next trial; behind the loop the Hessian-only evaluation, if any trial ran
bool NdtAlignment::more_trials(NdtRequest* next) {
  const double nu = 0.9;
  const double step_max = o_.step_size, step_min = o_.transformation_epsilon / 2.0;
  if (!interval_converged_ && trials_ < 10 && !(psi_t_ <= 0.0 && dphi_t_ <= -nu * dphi0_)) {
    a_t_ = open_ ? mt_trial(a_l_, f_l_, g_l_, a_u_, f_u_, g_u_, a_t_, psi_t_, dpsi_t_)
                 : mt_trial(a_l_, f_l_, g_l_, a_u_, f_u_, g_u_, a_t_, phi_t_, dphi_t_);
    a_t_ = max_of(min_of(a_t_, step_max), step_min);
    for (int r = 0; r < 6; ++r) x_[r] = p_[r] + dir_[r] * a_t_;
    std::memcpy(next->p, x_, sizeof(x_));
    ask(DLIOM_NDT_EVAL_GRADIENT, next);
    phase_ = kTrial;
    return true;
  }
  if (trials_ > 0) {
    std::memcpy(next->p, x_, sizeof(x_));
    ask(DLIOM_NDT_EVAL_HESSIAN, next);
    phase_ = kHessianOnly;
    return true;
  }
  return end_step(a_t_, next);
}

// Alignment 3 (the move) to 5
bool NdtAlignment::end_step(double a, NdtRequest* next) { return moved_and_done(a) ? false : begin_iteration(next); }

bool NdtAlignment::moved_and_done(double a) {
  for (int r = 0; r < 6; ++r) p_[r] = p_[r] + dir_[r] * a;
  if (it_ > o_.maximum_iterations || (it_ > 0 && std::fabs(a) < o_.transformation_epsilon)) {
    converged_ = 1;
    reason_ = it_ > o_.maximum_iterations ? DLIOM_NDT_ITERATIONS : DLIOM_NDT_EPSILON;
    iterations_ = it_ + 1;
    phase_ = kDone;
    return true;
  }
  ++it_;
  return false;
}

void NdtAlignment::finish(int64_t n, dliom_ndt_result* res, NdtPose* P) const {
  res->converged = converged_;
  res->reason = reason_;
  res->iterations = iterations_;
  std::memcpy(res->p, p_, sizeof(p_));
  ndt_pose(p_, P);
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) res->transform[4 * a + b] = P->R[3 * a + b];
    res->transform[4 * a + 3] = P->t[a];
  }
  res->transform[12] = res->transform[13] = res->transform[14] = 0.0;
  res->transform[15] = 1.0;
  res->score = sums_.score;
  res->transformation_probability = sums_.score / static_cast<double>(n);
  res->pairs = sums_.pairs;
  res->evaluations_with_hessian = with_hessian_;
  res->evaluations_without_hessian = without_hessian_;
}

}  // namespace dliom

extern "C" {

int dliom_ndt_default_options(dliom_ndt_options* options) {
  if (options == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *options = dliom_ndt_options{1.0, 0.1, 0.01, 0.55, 35, 6, DLIOM_NDT_STEP_CLAMPED, 0};
  return DLIOM_OK;
}

int dliom_ndt_target_create(dliom_ctx* ctx, const dliom_cloud* target, const dliom_ndt_options* options, dliom_ndt_target** out) {
  using namespace dliom;
  if (out != nullptr) *out = nullptr;
  if (ctx == nullptr || target == nullptr || out == nullptr || !ndt_options_ok(options) || target->ctx != ctx || target->n <= 0 ||
      target->n > DLIOM_NN_MAX_POINTS || ctx->done_word == nullptr)
    return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const auto started = std::chrono::steady_clock::now();
  const int n = static_cast<int>(target->n);
  struct Work {  // released on every way out
    DevBuf a, b;
    ~Work() {
      a.release();
      b.release();
    }
  } work;
  size_t sort_bytes = 0, scan_bytes = 0;
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, static_cast<const unsigned long long*>(nullptr),
                                                   static_cast<unsigned long long*>(nullptr), static_cast<const int*>(nullptr),
                                                   static_cast<int*>(nullptr), n, 0, 64, ctx->stream));
  DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, static_cast<const unsigned*>(nullptr), static_cast<unsigned*>(nullptr), n,
                                                 ctx->stream));
  const size_t per8 = align256(8 * static_cast<size_t>(n)), per4 = align256(4 * static_cast<size_t>(n));
  const size_t tmp_bytes = align256(std::max(sort_bytes, scan_bytes));
  DLIOM_TRY(work.a.reserve(2 * per8 + 4 * per4 + 256 + tmp_bytes));
  char* const a = work.a.as<char>();
  auto* const keys_in = reinterpret_cast<unsigned long long*>(a);
  auto* const keys = reinterpret_cast<unsigned long long*>(a + per8);
  int* const index_in = reinterpret_cast<int*>(a + 2 * per8);
  int* const sorted_index = reinterpret_cast<int*>(a + 2 * per8 + per4);
  unsigned* const head = reinterpret_cast<unsigned*>(a + 2 * per8 + 2 * per4);
  unsigned* const inclusive = reinterpret_cast<unsigned*>(a + 2 * per8 + 3 * per4);
  unsigned* const kept_word = reinterpret_cast<unsigned*>(a + 2 * per8 + 4 * per4);
  void* const tmp = a + 2 * per8 + 4 * per4 + 256;
  const FillJob fill{kept_word, 4, static_cast<unsigned>(n)};
  DLIOM_TRY(fill_multi(ctx, &fill, 1));
  const float inv = 1.0f / static_cast<float>(options->resolution);
  const dim3 grid(blocks_of(n, kThreads)), block(kThreads);
  hipLaunchKernelGGL(ndt_key_kernel, grid, block, 0, ctx->stream, target->d_x, target->d_y, target->d_z, n, inv, keys_in, index_in);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, keys_in, keys, index_in, sorted_index, n, 0, 64, ctx->stream));
  hipLaunchKernelGGL(ndt_head_kernel, grid, block, 0, ctx->stream, keys, n, head, kept_word);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(tmp, scan_bytes, head, inclusive, n, ctx->stream));
  const GatherJob jobs[2] = {{inclusive + (n - 1), 1}, {kept_word, 1}};
  unsigned* const words = pinned_at<unsigned>(ctx, kPinReadback);
  DLIOM_TRY(gather_and_wait(ctx, jobs, 2, words));
  const int cells = static_cast<int>(words[0]), kept = static_cast<int>(words[1]);
  if (cells < 0 || cells > n || kept < 0 || kept > n) return DLIOM_ERR_INTERNAL;
  auto t = std::make_unique<dliom_ndt_target>();
  t->ctx = ctx;
  t->resolution = options->resolution;
  t->min_points = options->min_points_per_voxel;
  t->n_points = n;
  t->n_kept = kept;
  t->build_read_backs = 1;
  NdtValidCells valid;
  if (cells > 0) {
    const size_t first_bytes = align256(4 * (static_cast<size_t>(cells) + 1)), key_bytes = align256(8 * static_cast<size_t>(cells));
    DLIOM_TRY(work.b.reserve(first_bytes + key_bytes + 72 * static_cast<size_t>(cells)));
    char* const b = work.b.as<char>();
    int* const cell_first = reinterpret_cast<int*>(b);
    auto* const cell_key = reinterpret_cast<unsigned long long*>(b + first_bytes);
    double* const sums = reinterpret_cast<double*>(b + first_bytes + key_bytes);
    hipLaunchKernelGGL(ndt_bounds_kernel, grid, block, 0, ctx->stream, keys, head, inclusive, n, cells, kept, cell_first, cell_key);
    DLIOM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ndt_cell_sums_kernel, dim3(static_cast<unsigned>(cells)), block, 0, ctx->stream, target->d_x, target->d_y,
                       target->d_z, sorted_index, cell_first, sums);
    DLIOM_HIP_TRY(hipGetLastError());
    std::vector<int> h_first(static_cast<size_t>(cells) + 1);
    std::vector<unsigned long long> h_key(cells);
    std::vector<double> h_sums(static_cast<size_t>(cells) * 9);
    DLIOM_HIP_TRY(hipMemcpyAsync(h_first.data(), cell_first, 4 * h_first.size(), hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipMemcpyAsync(h_key.data(), cell_key, 8 * h_key.size(), hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipMemcpyAsync(h_sums.data(), sums, 8 * h_sums.size(), hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    ++ctx->host_syncs;
    ++t->build_read_backs;
    ndt_finish_cells(t.get(), cells, h_first.data(), h_key.data(), h_sums.data(), &valid);
  }
  int status = ndt_table_upload_enqueue(t.get(), valid);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) status = DLIOM_ERR_HIP;  // the host vectors and the work buffers are free again
  ++ctx->host_syncs;
  if (status != DLIOM_OK) {
    t->table.release();
    return status;
  }
  if (ctx->profiling) t->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - started).count();
  *out = t.release();
  return DLIOM_OK;
}

void dliom_ndt_target_destroy(dliom_ndt_target* target) {
  if (target == nullptr) return;
  (void)hipSetDevice(target->ctx->device);
  (void)hipStreamSynchronize(target->ctx->stream);
  target->table.release();
  target->scratch.release();
  delete target;
}

int dliom_ndt_target_memory_stats(const dliom_ndt_target* target, dliom_ndt_target_memory* out) {
  if (target == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = dliom_ndt_target_memory{target->n_points,
                                 target->n_kept,
                                 static_cast<int64_t>(target->cells.size()),
                                 target->n_valid,
                                 static_cast<int64_t>(target->table.cap),
                                 static_cast<int64_t>(target->scratch.cap),
                                 target->build_read_backs,
                                 target->build_ms};
  return DLIOM_OK;
}

int dliom_ndt_target_cells(const dliom_ndt_target* target, dliom_ndt_cell* cells, int64_t capacity, int64_t* count) {
  if (target == nullptr || count == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *count = static_cast<int64_t>(target->cells.size());
  if (cells == nullptr) return DLIOM_OK;
  if (capacity < *count) return DLIOM_ERR_CAPACITY;
  if (*count > 0) std::memcpy(cells, target->cells.data(), sizeof(dliom_ndt_cell) * target->cells.size());
  return DLIOM_OK;
}

int dliom_ndt_evaluate(dliom_ndt_target* target, const dliom_cloud* source, const double* p6, const dliom_ndt_options* options,
                       int what, double* score, double* gradient6, double* hessian36, int64_t* pairs) {
  using namespace dliom;
  if (!ndt_call_ok(target, source, options) || p6 == nullptr || score == nullptr || gradient6 == nullptr || hessian36 == nullptr ||
      pairs == nullptr || what < DLIOM_NDT_EVAL_GRADIENT || what > DLIOM_NDT_EVAL_HESSIAN)
    return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(target->ctx->device));
  NdtRun run{target, source, ndt_constants(*options)};
  NdtSums sums;
  DLIOM_TRY(run.evaluate(p6, what, &sums));
  *score = sums.score;
  std::memcpy(gradient6, sums.g, sizeof(sums.g));
  std::memcpy(hessian36, sums.H, sizeof(sums.H));
  *pairs = sums.pairs;
  return DLIOM_OK;
}

int dliom_ndt_align(dliom_ndt_target* target, const dliom_cloud* source, const double* guess16, const dliom_ndt_options* options,
                    dliom_nn_index* fitness_index, dliom_ndt_result* result, dliom_cloud** aligned) {
  using namespace dliom;
  if (aligned != nullptr) *aligned = nullptr;
  if (!ndt_call_ok(target, source, options) || result == nullptr || !ndt_guess_ok(guess16) ||
      (fitness_index != nullptr && nn_ctx(fitness_index) != target->ctx))
    return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_ctx* const ctx = target->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const int n = static_cast<int>(source->n);
  dliom_ndt_result res = {};
  res.fitness_score = std::numeric_limits<double>::quiet_NaN();
  NdtRun run{target, source, ndt_constants(*options)};
  run.timed = ctx->profiling;
  const auto started = std::chrono::steady_clock::now();
  NdtAlignment machine;
  NdtRequest request;
  NdtSums sums;
  machine.start(*options, guess16, &request);
  do {
    DLIOM_TRY(run.evaluate(request.p, request.what, &sums));
  } while (machine.advance(sums, &request));
  const double loop_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - started).count();
  NdtPose P;
  machine.finish(n, &res, &P);
  res.read_backs = run.read_backs;
  if (!run.events.empty()) {
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t e = 0; e + 2 < run.events.size(); e += 3) {
      float ms[2] = {0.f, 0.f};
      DLIOM_HIP_TRY(hipEventElapsedTime(&ms[0], run.events[e], run.events[e + 1]));
      DLIOM_HIP_TRY(hipEventElapsedTime(&ms[1], run.events[e + 1], run.events[e + 2]));
      res.evaluate_ms += ms[0];
      res.reduce_ms += ms[1];
    }
    res.host_ms = std::max(0.0, loop_ms - res.evaluate_ms - res.reduce_ms);
  }
  // the final points: the fitness score and the aligned cloud
  if (fitness_index != nullptr || aligned != nullptr) {
    float *x, *y, *z;
    dliom_cloud* cloud = nullptr;
    DLIOM_TRY(alloc_device_cloud(ctx, n, &cloud, &x, &y, &z));
    Rigid12 m;
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) m.m[4 * a + b] = P.R[3 * a + b];
      m.m[4 * a + 3] = P.t[a];
    }
    int st = DLIOM_OK;
    unsigned* max_sq = nullptr;
    if (n > 0) st = nn_transform_enqueue(ctx, source->d_x, source->d_y, source->d_z, n, m, x, y, z);
    if (st == DLIOM_OK && fitness_index != nullptr) {
      long long count = 0;
      st = icp_fitness_of(fitness_index, x, y, z, n, &res.fitness_score, &count);
      res.fitness_count = count;
      ++res.read_backs;
    }
    if (st == DLIOM_OK && aligned != nullptr) {
      unsigned word = 0;
      if (n > 0) {
        st = target->scratch.reserve(256);
        if (st == DLIOM_OK) {
          max_sq = target->scratch.as<unsigned>();
          const FillJob fill{max_sq, 4, 0u};
          st = fill_multi(ctx, &fill, 1);
        }
        if (st == DLIOM_OK) {
          hipLaunchKernelGGL(ndt_max_norm_kernel, dim3(blocks_of(n, kThreads)), dim3(kThreads), 0, ctx->stream, x, y, z, n, max_sq);
          if (hipGetLastError() != hipSuccess) st = DLIOM_ERR_HIP;
        }
        if (st == DLIOM_OK) {
          const GatherJob job{max_sq, 1};
          unsigned* const words = pinned_at<unsigned>(ctx, kPinReadback);
          st = gather_and_wait(ctx, &job, 1, words);
          word = words[0];
          ++res.read_backs;
        }
      }
      float max_norm_sq;
      std::memcpy(&max_norm_sq, &word, 4);
      if (st == DLIOM_OK) st = finish_device_cloud(ctx, cloud, std::sqrt(max_norm_sq));
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && st == DLIOM_OK) st = DLIOM_ERR_HIP;
    ++ctx->host_syncs;
    if (st != DLIOM_OK || aligned == nullptr) {
      dliom_cloud_destroy(cloud);
      if (st != DLIOM_OK) return st;
    } else {
      *aligned = cloud;
    }
  }
  *result = res;
  return DLIOM_OK;
}

// ---- MatchByNDT over a stream of scans: the previous scan's cells stay on the device -----------------------------------------
int dliom_ndt_scan_matcher_create(dliom_ctx* ctx, const dliom_ndt_options* options, float leaf, dliom_ndt_scan_matcher** out) {
  if (out != nullptr) *out = nullptr;
  if (ctx == nullptr || out == nullptr || !dliom::ndt_options_ok(options) || !(leaf > 0.f)) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = new dliom_ndt_scan_matcher{ctx, *options, leaf, nullptr};
  return DLIOM_OK;
}

void dliom_ndt_scan_matcher_destroy(dliom_ndt_scan_matcher* matcher) {
  if (matcher == nullptr) return;
  dliom_ndt_target_destroy(matcher->target);
  delete matcher;
}

int dliom_ndt_scan_matcher_has_target(const dliom_ndt_scan_matcher* matcher, int* has_target) {
  if (matcher == nullptr || has_target == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *has_target = matcher->target != nullptr ? 1 : 0;
  return DLIOM_OK;
}

int dliom_ndt_scan_matcher_match(dliom_ndt_scan_matcher* matcher, const dliom_cloud* scan, const double* guess16,
                                 dliom_ndt_result* result) {
  if (matcher == nullptr || scan == nullptr || scan->ctx != matcher->ctx) return DLIOM_ERR_INVALID_ARGUMENT;
  const bool first = matcher->target == nullptr;
  if (!first && (guess16 == nullptr || result == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_cloud* filtered = nullptr;
  DLIOM_TRY(dliom_cloud_approximate_voxel_filter(matcher->ctx, scan, matcher->leaf, &filtered));
  dliom_ndt_result res = {};
  int st = DLIOM_OK;
  if (!first) st = dliom_ndt_align(matcher->target, filtered, guess16, &matcher->options, nullptr, &res, nullptr);
  dliom_ndt_target* cells = nullptr;
  if (st == DLIOM_OK) st = dliom_ndt_target_create(matcher->ctx, filtered, &matcher->options, &cells);
  dliom_cloud_destroy(filtered);
  if (st != DLIOM_OK) return st;  // the matcher is as it was
  dliom_ndt_target_destroy(matcher->target);
  matcher->target = cells;
  if (!first) *result = res;
  return DLIOM_OK;
}

}  // extern "C"
