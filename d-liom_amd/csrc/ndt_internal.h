// What an alignment of one pair (ndt.hip) and of many pairs in lock step (ndt_batch.hip) share: the target as the kernels
// see it, the evaluation's body, the leaves of its sums, the read-back of one evaluation and the body that writes it, and
// the host's part -- the pose's coefficient rows, the Newton step and the alignment itself as a resumable state machine
// (NdtAlignment, defined in ndt.hip).  Stated once, so that a pair gets the same bits whichever call aligns it.
#ifndef DLIOM_CSRC_NDT_INTERNAL_H_
#define DLIOM_CSRC_NDT_INTERNAL_H_

#include <cstdint>
#include <vector>

#include "device_common.h"
#include "nn_index.h"
#include "tree_reduce.h"

struct dliom_ndt_target {
  dliom_ctx* ctx = nullptr;
  double resolution = 0.0;
  int min_points = 0;
  int64_t n_points = 0, n_kept = 0, n_valid = 0;
  std::vector<dliom_ndt_cell> cells;  // every cell, in key order
  dliom::DevBuf table;                // the valid cells: keys (8 B each), then mean and icov (72 B each)
  size_t cell_data_at = 0;
  dliom::DevBuf scratch;              // an evaluation's leaves, partial sums and counts
  int poll_us = 150;
  int64_t build_read_backs = 0;
  double build_ms = 0.0;
};

namespace dliom {

constexpr int kNdtThreads = 256;
constexpr int kNdtHalf = DLIOM_NDT_MAX_CELL_INDEX;
constexpr int kNdtCellDoubles = 9;  // mean (3), icov 00 01 02 11 12 22

__host__ __device__ inline unsigned long long ndt_key(int ix, int iy, int iz) {
  return (static_cast<unsigned long long>(iz + kNdtHalf) << 42) | (static_cast<unsigned long long>(iy + kNdtHalf) << 21) |
         static_cast<unsigned long long>(ix + kNdtHalf);
}

// ---- the target's build: the bodies that dliom_ndt_target_create's kernels (ndt.hip) and a chunk of
// dliom_ndt_target_create_batch (ndt_target_batch.hip) both run.  Every pointer is the TARGET'S OWN: its coordinates, and
// its run of the sorted keys, indices, heads and scan, so that positions count from the target's first one.
constexpr unsigned long long kNdtSkipKey = ~0ull;

// point i's 63-bit cell key (z high, x low), or the skip key
__device__ __forceinline__ unsigned long long ndt_key_body(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ z, int i, float inv) {
  const float f[3] = {floorf(x[i] * inv), floorf(y[i] * inv), floorf(z[i] * inv)};
  bool ok = isfinite(x[i]) && isfinite(y[i]) && isfinite(z[i]);
  for (int a = 0; a < 3; ++a) ok = ok && f[a] >= -static_cast<float>(kNdtHalf) && f[a] < static_cast<float>(kNdtHalf);
  return ok ? ndt_key(static_cast<int>(f[0]), static_cast<int>(f[1]), static_cast<int>(f[2])) : kNdtSkipKey;
}

// head[i] = 1 where a cell starts; *kept (n on entry) = the first position that holds the skip key.  Position 0 starts a
// cell whatever lies in front of the target's run.
__device__ __forceinline__ void ndt_head_body(const unsigned long long* __restrict__ keys, int i, unsigned* __restrict__ head,
                                              unsigned* __restrict__ kept) {
  const unsigned long long k = keys[i];
  const bool first = i == 0 || keys[i - 1] != k;
  head[i] = first && k != kNdtSkipKey ? 1u : 0u;
  if (first && k == kNdtSkipKey) *kept = static_cast<unsigned>(i);
}

// cell_first: cells + 1 entries.  before: the scan's value in front of the target's run (0 for a run that starts the scan).
__device__ __forceinline__ void ndt_bounds_body(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ head,
                                                const unsigned* __restrict__ inclusive, unsigned before, int i, int n, int cells,
                                                int kept, int* __restrict__ cell_first, unsigned long long* __restrict__ cell_key) {
  if (i == 0) cell_first[cells] = kept;
  if (i >= n || head[i] == 0u) return;
  const int c = static_cast<int>(inclusive[i] - before) - 1;
  if (c < 0 || c >= cells) return;
  cell_first[c] = i;
  cell_key[c] = keys[i];
}

// Called by every lane of a kNdtThreads workgroup: the nine sums (S 0..2, Q 00 01 02 11 12 22) of the cell that holds the
// m sorted positions from `first`, in the header's fixed tree -- 256 leaves at a time through LDS, longer cells in aligned
// chunks of 256 whose partial sums meet in a binary counter (the same tree, whatever the cell's length).
__device__ __forceinline__ void ndt_cell_sums_body(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                   const int* __restrict__ sorted_index, int first, int m, double* __restrict__ sums) {
  __shared__ double lds[kNdtThreads * 9];
  __shared__ double stack[17 * 9];  // the binary counter of the chunks' partial sums: level l holds 2^l chunks
  int m2 = 1;
  while (m2 < m) m2 <<= 1;
  const int width = m2 < kNdtThreads ? m2 : kNdtThreads;  // leaves of a chunk
  const int chunks = m2 / width;
  for (int chunk = 0; chunk < chunks; ++chunk) {
    const int at = chunk * width + static_cast<int>(threadIdx.x);
    double v[9];
    if (static_cast<int>(threadIdx.x) < width && at < m) {
      const int j = sorted_index[first + at];
      const double p[3] = {x[j], y[j], z[j]};
      v[0] = p[0];
      v[1] = p[1];
      v[2] = p[2];
      v[3] = p[0] * p[0];
      v[4] = p[0] * p[1];
      v[5] = p[0] * p[2];
      v[6] = p[1] * p[1];
      v[7] = p[1] * p[2];
      v[8] = p[2] * p[2];
    } else {
      for (int k = 0; k < 9; ++k) v[k] = 0.0;
    }
    __syncthreads();  // the previous chunk's root has been taken
    for (int k = 0; k < 9; ++k) lds[threadIdx.x * 9 + k] = v[k];
    for (int w = 1; w < width; w <<= 1) {
      __syncthreads();
      const int pairs = width / (2 * w);
      for (int e = threadIdx.x; e < pairs * 9; e += kNdtThreads) {
        const int left = (e / 9) * 2 * w, k = e % 9;
        lds[left * 9 + k] = lds[left * 9 + k] + lds[(left + w) * 9 + k];
      }
    }
    __syncthreads();
    if (threadIdx.x < 9) {  // lane k carries sum k through the counter
      double carry = lds[threadIdx.x];
      int level = 0;
      while ((chunk >> level) & 1) {
        carry = stack[level * 9 + threadIdx.x] + carry;
        ++level;
      }
      stack[level * 9 + threadIdx.x] = carry;
      if (chunk == chunks - 1) sums[threadIdx.x] = carry;
    }
  }
}

struct NdtTable {
  const unsigned long long* keys;  // the valid cells, ascending
  const double* cell;              // 9 doubles each
  int cells;
  float inv, r2;
  double d1, d2;
};

// T(p) and the coefficient rows of the header's point derivatives
struct NdtPose {
  double R[9], t[3];
  double J[3][3][3];  // [angle][component][coefficient]; J[0][0] is not used (the component is +0.0)
  double H[6][3][3];  // 33 34 35 44 45 55; [0..2][0] are not used
};

__device__ __forceinline__ double ndt_exp(double u) {
  if (u < -708.0) return 0.0;
  if (u != u) return u;
  if (u > 708.0) return __longlong_as_double(0x7ff0000000000000ll);
  const double k = rint(u * 0x1.71547652b82fep+0);
  const double r = (u - k * 0x1.62e42fee00000p-1) - k * 0x1.a39ef35793c76p-33;
  constexpr double c[14] = {1.0,
                            1.0,
                            1.0 / 2.0,
                            1.0 / 6.0,
                            1.0 / 24.0,
                            1.0 / 120.0,
                            1.0 / 720.0,
                            1.0 / 5040.0,
                            1.0 / 40320.0,
                            1.0 / 362880.0,
                            1.0 / 3628800.0,
                            1.0 / 39916800.0,
                            1.0 / 479001600.0,
                            1.0 / 6227020800.0};
  double p = c[13];
#pragma unroll
  for (int n = 12; n >= 0; --n) p = p * r + c[n];
  return p * __longlong_as_double(static_cast<long long>(static_cast<int>(k) + 1023) << 52);
}

__device__ __forceinline__ double ndt_dot3(const double a[3], double x0, double x1, double x2) { return (a[0] * x0 + a[1] * x1) + a[2] * x2; }

constexpr int ndt_sums(bool G, bool H) { return (G ? 7 : 0) + (H ? 21 : 0); }

// One source point of an evaluation, a lane a point (i = block * kNdtThreads + lane): transform, nine binary searches, the
// 7 / 21 / 28 values in registers in the header's order, then one store a value.  leaves: S arrays of n; pairs: n.
// ndt_eval_kernel runs it for the one pair of its arguments, ndt_batch_eval_kernel for a pair of a table.
template <bool G, bool H>
__device__ __forceinline__ void ndt_eval_body(const NdtTable& T, const NdtPose& P, const float* __restrict__ sx,
                                              const float* __restrict__ sy, const float* __restrict__ sz, int n,
                                              double* __restrict__ leaves, int* __restrict__ pairs, int block) {
  constexpr int S = ndt_sums(G, H);
  constexpr int kH0 = G ? 7 : 0;
  constexpr int kHalf = kNdtHalf;
  const int i = block * kNdtThreads + static_cast<int>(threadIdx.x);
  if (i >= n) return;
  double acc[S];
#pragma unroll
  for (int k = 0; k < S; ++k) acc[k] = 0.0;
  int count = 0;
  const double x0 = sx[i], x1 = sy[i], x2 = sz[i];
  const float q[3] = {static_cast<float>(((P.R[0] * x0 + P.R[1] * x1) + P.R[2] * x2) + P.t[0]),
                      static_cast<float>(((P.R[3] * x0 + P.R[4] * x1) + P.R[5] * x2) + P.t[1]),
                      static_cast<float>(((P.R[6] * x0 + P.R[7] * x1) + P.R[8] * x2) + P.t[2])};
  const float f[3] = {floorf(q[0] * T.inv), floorf(q[1] * T.inv), floorf(q[2] * T.inv)};
  bool live = isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) live = live && f[a] >= -static_cast<float>(kHalf + 1) && f[a] <= static_cast<float>(kHalf);
  if (live && T.cells > 0) {
    const int ix = static_cast<int>(f[0]), iy = static_cast<int>(f[1]), iz = static_cast<int>(f[2]);
    // the point's derivative vectors
    double Jv[3][3], Hv[6][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int r = 0; r < 3; ++r) Jv[a][r] = (a == 0 && r == 0) ? 0.0 : ndt_dot3(P.J[a][r], x0, x1, x2);
    if constexpr (H) {
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int r = 0; r < 3; ++r) Hv[a][r] = (a < 3 && r == 0) ? 0.0 : ndt_dot3(P.H[a][r], x0, x1, x2);
    }
    const int xlo = max(ix - 1, -kHalf), xhi = min(ix + 1, kHalf - 1);
    for (int dz = -1; dz <= 1; ++dz) {
      const int cz = iz + dz;
      if (cz < -kHalf || cz >= kHalf) continue;
      for (int dy = -1; dy <= 1; ++dy) {
        const int cy = iy + dy;
        if (cy < -kHalf || cy >= kHalf || xlo > xhi) continue;
        const unsigned long long klo = ndt_key(xlo, cy, cz), khi = ndt_key(xhi, cy, cz);
        int lo = 0, hi = T.cells;  // the first cell with key >= klo
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (T.keys[mid] < klo)
            lo = mid + 1;
          else
            hi = mid;
        }
        for (int c = lo; c < T.cells && T.keys[c] <= khi; ++c) {
          const double* cell = T.cell + static_cast<size_t>(c) * kNdtCellDoubles;
          const double mean[3] = {cell[0], cell[1], cell[2]};
          const float dx = q[0] - static_cast<float>(mean[0]), dy2 = q[1] - static_cast<float>(mean[1]),
                      dz2 = q[2] - static_cast<float>(mean[2]);
          if (!((dx * dx + dy2 * dy2) + dz2 * dz2 <= T.r2)) continue;
          ++count;
          const double ic[3][3] = {{cell[3], cell[4], cell[5]}, {cell[4], cell[6], cell[7]}, {cell[5], cell[7], cell[8]}};
          const double xt[3] = {static_cast<double>(q[0]) - mean[0], static_cast<double>(q[1]) - mean[1],
                                static_cast<double>(q[2]) - mean[2]};
          double w[3];
#pragma unroll
          for (int r = 0; r < 3; ++r) w[r] = ndt_dot3(ic[r], xt[0], xt[1], xt[2]);
          const double qq = (xt[0] * w[0] + xt[1] * w[1]) + xt[2] * w[2];
          const double e = ndt_exp(-(T.d2 * qq) * 0.5);
          double fe = T.d2 * e;
          if (fe > 1.0 || fe < 0.0 || fe != fe) continue;
          if constexpr (G) acc[0] += -T.d1 * e;
          fe = fe * T.d1;
          double cJ[6][3], u[6];
#pragma unroll
          for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int r = 0; r < 3; ++r) cJ[a][r] = a < 3 ? ic[r][a] : ndt_dot3(ic[r], Jv[a - 3][0], Jv[a - 3][1], Jv[a - 3][2]);
            u[a] = (xt[0] * cJ[a][0] + xt[1] * cJ[a][1]) + xt[2] * cJ[a][2];
            if constexpr (G) acc[1 + a] += u[a] * fe;
          }
          if constexpr (H) {
            int slot = kH0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
              for (int b = a; b < 6; ++b) {
                double h = 0.0;
                if (a >= 3) {  // b >= a
                  const int which = a == 3 ? b - 3 : (a == 4 ? b - 1 : 5);
                  double v[3];
#pragma unroll
                  for (int r = 0; r < 3; ++r) v[r] = ndt_dot3(ic[r], Hv[which][0], Hv[which][1], Hv[which][2]);
                  h = (xt[0] * v[0] + xt[1] * v[1]) + xt[2] * v[2];
                }
                const double k = b < 3 ? cJ[a][b] : (Jv[b - 3][0] * cJ[a][0] + Jv[b - 3][1] * cJ[a][1]) + Jv[b - 3][2] * cJ[a][2];
                acc[slot] += fe * ((((-T.d2) * u[a]) * u[b] + h) + k);
                ++slot;
              }
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < S; ++k) leaves[static_cast<size_t>(k) * n + i] = acc[k];
  pairs[i] = count;
}

template <int S>
struct NdtLeaves {
  const double* v;
  const int* pairs;
  int n;
  __device__ __forceinline__ void leaf(int i, double out[S], int* count) const {
    if (i < n) {
      for (int k = 0; k < S; ++k) out[k] = v[static_cast<size_t>(k) * n + i];
      *count = pairs[i];
    } else {
      for (int k = 0; k < S; ++k) out[k] = 0.0;
      *count = 0;
    }
  }
};

struct NdtReadback {  // kPinNdtSums; what an evaluation leaves in a slot of kPinNdtBatchReadback
  double sums[28];
  long long pairs;
};
static_assert(sizeof(NdtReadback) <= kPinNdtSums.bytes && sizeof(NdtReadback) <= kPinNdtBatchSlotBytes, "the read-back fits its regions");

// Called by every lane of a kTreeThreads workgroup: the tree over the P partial sums of one evaluation (partials: room for
// P2 >= P entries), then the S sums and the pair count into *out (page-locked).  The caller makes them visible to the host.
template <int S>
__device__ __forceinline__ void ndt_finish_body(double* partials, const int* __restrict__ counts, int P, int P2, NdtReadback* out) {
  tree_finish<S>(partials, P, P2);
  if (threadIdx.x < S) out->sums[threadIdx.x] = partials[threadIdx.x];
  if (threadIdx.x == 0) {
    long long n = 0;
    for (int b = 0; b < P; ++b) n += counts[b];
    out->pairs = n;
  }
}

// ---- the host's part (ndt.hip) ---------------------------------------------------------------------------------------------
struct NdtConstants {
  double d1, d2;
};
NdtConstants ndt_constants(const dliom_ndt_options& o);
bool ndt_options_ok(const dliom_ndt_options* o);
bool ndt_guess_ok(const double* g);
void ndt_pose(const double p[6], NdtPose* P);
NdtTable ndt_table_of(const dliom_ndt_target* t, const NdtConstants& k);

// The build's host step (dliom.h, target cells), a cell at a time in double: fills t->cells from the cells' first positions
// (cells + 1 entries), keys and sums (9 a cell) as they were read back, and gathers the valid cells' keys and data.
struct NdtValidCells {
  std::vector<unsigned long long> keys;
  std::vector<double> data;  // kNdtCellDoubles a cell
};
void ndt_finish_cells(dliom_ndt_target* t, int cells, const int* first, const unsigned long long* key, const double* sums,
                      NdtValidCells* valid);
// Allocates t->table for the valid cells and enqueues their copies on the context's stream; `valid` stays as it is until
// the stream has been waited for.
int ndt_table_upload_enqueue(dliom_ndt_target* t, const NdtValidCells& valid);

// What the host keeps of an alignment's evaluations: an evaluation writes only what it computed, the rest stays
struct NdtSums {
  double score = 0.0, g[6] = {}, H[6][6] = {};
  long long pairs = 0;
};
// the read-back of an evaluation of kind `what` (DLIOM_NDT_EVAL_*) into *out
void ndt_unpack(const NdtReadback& rb, int what, NdtSums* out);
// delta = -pinv(H) g (dliom.h, Alignment 1)
void ndt_newton_step(const NdtSums& s, double delta[6]);

struct NdtRequest {
  double p[6];
  int what;  // DLIOM_NDT_EVAL_*
};

// dliom.h's ALIGNMENT and STEP LENGTH as a state machine between evaluations: start() gives the first evaluation, and
// advance() takes the sums as they stand after the evaluation last asked for and gives the next one, or says that the
// alignment is done.  The caller evaluates however it likes (ndt.hip: one pair, blocking; ndt_batch.hip: a round of many).
class NdtAlignment {
 public:
  void start(const dliom_ndt_options& options, const double guess16[16], NdtRequest* first);
  bool advance(const NdtSums& sums, NdtRequest* next);  // false: done
  // converged, reason, iterations, both evaluation counts, p, transform, score, transformation_probability and pairs of
  // *res for a source of n points; the rest of *res stays.  *P: T(p), what the final points are moved by.
  void finish(int64_t n, dliom_ndt_result* res, NdtPose* P) const;

 private:
  enum Phase { kGuess, kFirstTrial, kTrial, kHessianOnly, kDone };
  bool begin_iteration(NdtRequest* next);
  bool more_trials(NdtRequest* next);
  bool end_step(double a, NdtRequest* next);
  bool moved_and_done(double a);
  void ask(int what, NdtRequest* next);

  dliom_ndt_options o_ = {};
  Phase phase_ = kDone;
  NdtSums sums_;
  double p_[6] = {};
  int it_ = 0;
  int converged_ = 0, reason_ = DLIOM_NDT_NOT_CONVERGED, iterations_ = 0;
  int64_t with_hessian_ = 0, without_hessian_ = 0;
  // a step length in progress
  double dir_[6] = {}, x_[6] = {};
  double phi0_ = 0.0, dphi0_ = 0.0, a_t_ = 0.0;
  double a_l_ = 0.0, f_l_ = 0.0, g_l_ = 0.0, a_u_ = 0.0, f_u_ = 0.0, g_u_ = 0.0;
  double phi_t_ = 0.0, dphi_t_ = 0.0, psi_t_ = 0.0, dpsi_t_ = 0.0;
  bool open_ = true, interval_converged_ = false;
  int trials_ = 0;
};

}  // namespace dliom

#endif  // DLIOM_CSRC_NDT_INTERNAL_H_
