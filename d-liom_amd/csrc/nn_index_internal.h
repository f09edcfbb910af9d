// What the build of one index (nn_index.hip) and of many in one call (nn_index_batch.hip) share: the index itself, the
// host's choice of the grid, the ordered words of the bounding box and the bodies of the three build kernels.  Stated
// once, so that an index has the same cells, the same box and the same points whichever call builds it.  Only .hip files
// include this.
#ifndef DLIOM_CSRC_NN_INDEX_INTERNAL_H_
#define DLIOM_CSRC_NN_INDEX_INTERNAL_H_

#include <algorithm>
#include <cmath>
#include <cstring>

#include "device_common.h"
#include "nn_index.h"

struct dliom_nn_index {
  dliom_ctx* ctx = nullptr;
  int64_t n_target = 0, n_finite = 0;
  int dims[3] = {1, 1, 1};
  float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
  float inv = 0.f;
  double edge = 0.0;
  int search = DLIOM_NN_AUTO;
  dliom::DevBuf sorted, by_index, cell_start;
  // a batch-built index (nn_index_batch.hip): ONE allocation, by_index | cell_start | sorted.  The three above are then
  // views into it (p, and as cap the bytes the single build allocates) and are not released on their own
  dliom::DevBuf slab;
  dliom::DevBuf scratch;  // of the call that runs
  int poll_us = 150;      // poll window of a read-back's completion word: twice what the previous one took
};

namespace dliom {

constexpr int kNnThreads = 256;  // of every kernel of the index

// bytes of an index's three arrays, as DevBuf::reserve rounds what dliom_nn_index_create asks for
inline size_t nn_by_index_bytes(int64_t n) { return align256(16 * static_cast<size_t>(n)); }
inline size_t nn_cell_start_bytes(size_t cells) { return align256(4 * (cells + 1)); }
inline size_t nn_sorted_bytes(int64_t n_finite) { return align256(std::max<size_t>(16, 16 * static_cast<size_t>(n_finite))); }

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  const float inf = __int_as_float(0x7f800000);
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;  // false for NaN
}

// bit patterns that order like the floats they come from
__device__ __forceinline__ unsigned ordered_word(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float float_of_ordered_word(unsigned w) {
  const unsigned u = (w & 0x80000000u) ? (w & 0x7fffffffu) : ~w;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// The box of the finite points and their count, by integer atomics on ordered words.  lo_words: min x y z (preset to
// ~0), hi_words: max x y z (preset to 0) and the finite count.  Called by every lane of a workgroup.
__device__ __forceinline__ void nn_box_body(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n,
                                            unsigned* __restrict__ lo_words, unsigned* __restrict__ hi_words, int block) {
  const int i = block * kNnThreads + static_cast<int>(threadIdx.x);
  unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  bool ok = false;
  if (i < n) {
    const float p[3] = {x[i], y[i], z[i]};
    ok = finite3(p[0], p[1], p[2]);
    if (ok)
      for (int a = 0; a < 3; ++a) lo[a] = hi[a] = ordered_word(p[a]);
  }
  const unsigned long long votes = __ballot(ok);
  if (votes == 0ull) return;  // the whole wave
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    for (int a = 0; a < 3; ++a) {
      lo[a] = min(lo[a], static_cast<unsigned>(__shfl_xor(static_cast<int>(lo[a]), off, 64)));
      hi[a] = max(hi[a], static_cast<unsigned>(__shfl_xor(static_cast<int>(hi[a]), off, 64)));
    }
  if ((threadIdx.x & 63u) == 0u) {
    for (int a = 0; a < 3; ++a) {
      atomicMin(lo_words + a, lo[a]);
      atomicMax(hi_words + a, hi[a]);
    }
    atomicAdd(hi_words + 3, static_cast<unsigned>(__popcll(votes)));
  }
}

// The cell of a coordinate inside [lo, hi].  Monotone in x: the rounded subtraction, the rounded product with inv >= 0,
// floorf and the clamps all are -- what the stop rule of nn_shell_kernel stands on.  (A NaN product, inf * 0 under the
// one-cell grid of an unbounded box, is cell 0: fmaxf returns its other argument.)
__device__ __forceinline__ int nn_cell(float x, float lo, float inv, int dim, float* u_out = nullptr) {
  const float u = (x - lo) * inv;
  if (u_out != nullptr) *u_out = u;
  return static_cast<int>(fminf(fmaxf(floorf(u), 0.f), static_cast<float>(dim - 1)));
}

// what of a grid a point's cell depends on
struct NnCells {
  int dims[3];
  float lo[3];
  float inv;
};

__device__ __forceinline__ int nn_cell_index(const NnCells& g, float x, float y, float z) {
  const int cx = nn_cell(x, g.lo[0], g.inv, g.dims[0]);
  const int cy = nn_cell(y, g.lo[1], g.inv, g.dims[1]);
  const int cz = nn_cell(z, g.lo[2], g.inv, g.dims[2]);
  return (cz * g.dims[1] + cy) * g.dims[0] + cx;
}

// a point's cell (-1: not finite), the cells' populations (integer atomics) and the point's copy in the cloud's order
__device__ __forceinline__ void nn_count_body(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n,
                                              const NnCells& g, int* __restrict__ cell_of_point, int* __restrict__ counts,
                                              float4* __restrict__ by_index, int block) {
  const int i = block * kNnThreads + static_cast<int>(threadIdx.x);
  if (i >= n) return;
  const float px = x[i], py = y[i], pz = z[i];
  by_index[i] = make_float4(px, py, pz, 0.f);
  int c = -1;
  if (finite3(px, py, pz)) {
    c = nn_cell_index(g, px, py, pz);
    atomicAdd(counts + c, 1);
  }
  cell_of_point[i] = c;
}

// The counting sort's scatter.  starts: the exclusive sum of the populations, which may run on from the cells in front of
// this index's (a batched build scans many indices' cells at once): `before` is its value at the index's first cell.
__device__ __forceinline__ void nn_scatter_body(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n,
                                                const int* __restrict__ cell_of_point, const int* __restrict__ starts, int before,
                                                int* __restrict__ cursor, float4* __restrict__ sorted, int block) {
  const int i = block * kNnThreads + static_cast<int>(threadIdx.x);
  if (i >= n) return;
  const int c = cell_of_point[i];
  if (c < 0) return;
  const int at = (starts[c] - before) + atomicAdd(cursor + c, 1);  // < the next cell's start: the cursor counts what nn_count_body counted
  sorted[at] = make_float4(x[i], y[i], z[i], __int_as_float(i));
}

// The grid over a box of `extent` metres an axis for n points: edge0 (0: half the edge that puts a point a cell into the
// box's volume, area or length, whichever it has -- a scan's points lie on surfaces and crowd near the sensor, so most
// cells are empty, and an empty cell costs the walk nothing: a shell's row is one range of slots), grown by 26 % a step
// until the grid fits.  A box whose extent is not finite, or a
// single point, is one cell with inv = 0.
inline void nn_choose_grid(const double extent[3], int64_t n, double edge0, int dims[3], float* inv, double* edge) {
  dims[0] = dims[1] = dims[2] = 1;
  *inv = 0.f;
  *edge = 0.0;
  double product = 1.0;
  int axes = 0;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(extent[a])) return;
    if (extent[a] > 0.0) {
      product *= extent[a];
      ++axes;
    }
  }
  if (axes == 0 || !std::isfinite(product)) return;
  double e = edge0 > 0.0 ? edge0 : 0.5 * std::pow(product / static_cast<double>(std::max<int64_t>(n, 1)), 1.0 / axes);
  if (!(e >= 1e-6)) e = 1e-6;
  for (int step = 0; step < 400; ++step, e *= 1.26) {
    const float f = static_cast<float>(1.0 / e);
    if (!(f > 0.f) || !std::isfinite(f)) continue;
    double cells = 1.0;
    bool fits = true;
    int d[3];
    for (int a = 0; a < 3; ++a) {
      const double along = std::floor(extent[a] * static_cast<double>(f)) + 1.0;
      fits = fits && along <= DLIOM_NN_MAX_CELLS_PER_AXIS;
      d[a] = fits ? static_cast<int>(along) : 1;
      cells *= along;
    }
    if (!fits || cells > DLIOM_NN_MAX_CELLS) continue;
    dims[0] = d[0];
    dims[1] = d[1];
    dims[2] = d[2];
    *inv = f;
    *edge = 1.0 / static_cast<double>(f);
    return;
  }
}

// The box words of a build as the host reads them -> the index's box and grid.  lo_words, hi_words: nn_box_body's.
inline void nn_set_grid(dliom_nn_index* f, const unsigned* lo_words, const unsigned* hi_words, double edge0) {
  f->n_finite = hi_words[3];
  double extent[3] = {0.0, 0.0, 0.0};
  if (f->n_finite > 0)
    for (int a = 0; a < 3; ++a) {
      f->lo[a] = float_of_ordered_word(lo_words[a]);
      f->hi[a] = float_of_ordered_word(hi_words[a]);
      extent[a] = static_cast<double>(f->hi[a]) - static_cast<double>(f->lo[a]);
    }
  nn_choose_grid(extent, f->n_finite, edge0, f->dims, &f->inv, &f->edge);
}

inline NnCells nn_cells_of(const dliom_nn_index* f) {
  NnCells g;
  for (int a = 0; a < 3; ++a) {
    g.dims[a] = f->dims[a];
    g.lo[a] = f->lo[a];
  }
  g.inv = f->inv;
  return g;
}

// dliom_nn_index_create's check of its options (NULL: the defaults) -> the edge and the search mode
inline bool nn_index_options_ok(const dliom_nn_index_options* options, double* edge0, int* search) {
  *edge0 = 0.0;
  *search = DLIOM_NN_AUTO;
  if (options == nullptr) return true;
  if (!std::isfinite(options->cell_edge) || options->cell_edge < 0.0 || options->reserved != 0 ||
      (options->search != DLIOM_NN_AUTO && options->search != DLIOM_NN_BRUTE_FORCE))
    return false;
  *edge0 = options->cell_edge;
  *search = options->search;
  return true;
}

}  // namespace dliom

#endif  // DLIOM_CSRC_NN_INDEX_INTERNAL_H_
