// Exact nearest neighbours of 3-D points in HBM (dliom.h "scan alignment by ICP", Nearest neighbour): the search that
// pcl::IterativeClosestPoint asks of its kd-tree, stated as one float formula with one tie rule, so that a grid walk and
// a brute-force scan give the same (j, d2) bits.  This file is built with -ffp-contract=off like every other.
//
//   nn_box_kernel      bounding box and count of the finite target points (integer atomics on ordered words)
//   nn_count_kernel    a point's cell, and the cells' populations (integer atomics)
//   nn_scatter_kernel  the counting sort's scatter: (x, y, z, index) by cell.  The order inside a cell is whatever the
//                      atomics give; no result depends on it, because candidates are compared by (d2, index)
//   nn_shell_kernel    a lane a query: cubic shells of cells around the query's cell, at most DLIOM_NN_MAX_SHELLS + 1 of them;
//                      a query it cannot settle goes into a list (wave ballot + one integer atomic a wave)
//   nn_brute_kernel    the sorted points tiled through LDS, every listed (or every) query against every point; all lanes
//                      read one LDS address at a time (a broadcast).  The points are split into segments over the grid's
//                      second dimension, so that a handful of listed queries does not wait for one workgroup to scan the
//                      whole target; a segment's best goes into the query's 64-bit key (d2's bits, then the index) by an
//                      integer atomicMin, whose result no order of arrival can change
//   nn_resolve_kernel  a listed query's key -> (j, d2) under the distance bound
//   nn_transform_kernel  p = (float)(R p + t) in double
// The shell walk, the scan, the resolve and the transform are each ONE __device__ body over (view, search, bound,
// workgroup index).  nn_*_kernel runs it for the one search of its arguments; nn_*_batch_kernel for the searches of a table
// in HBM (nn_index.h NnBatchItem), with the pair as a grid dimension.  What is proven of a body -- the stop rule, the tie
// rule -- holds for both.  The three build kernels' bodies, the index and the host's choice of its grid are in
// nn_index_internal.h: many indices are built in one call by nn_index_batch.hip.
//
// Every loop's bound is known before it starts: the shells by DLIOM_NN_MAX_SHELLS, the rows of a shell by its width, a
// row's points by the index's size; the brute-force kernel by the index's size.  No kernel waits on another workgroup.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "nn_index_internal.h"

namespace dliom {
namespace {

constexpr int kThreads = kNnThreads;
constexpr int kTile = 1024;  // target points staged in LDS at a time (16 KiB)
// Target points a workgroup of nn_brute_kernel scans for its queries.  Every query: 4 tiles (many workgroups a SIMD hide
// the LDS latency).  Listed queries are few -- often a handful, one wave a SIMD -- and wait for the longest segment: a
// quarter tile, i.e. as many segments as the grid's second dimension is allowed (256), more atomics and a shorter tail.
constexpr int kBruteSegment = 4 * kTile, kListedSegment = kTile / 4;

// The three build kernels run the bodies of nn_index_internal.h, which a batched build (nn_index_batch.hip) runs too.
// words: [min x y z, unused | max x y z, finite count]
__global__ __launch_bounds__(kThreads) void nn_box_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ z, int n, unsigned* __restrict__ words) {
  nn_box_body(x, y, z, n, words, words + 4, static_cast<int>(blockIdx.x));
}

__global__ __launch_bounds__(kThreads) void nn_count_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ z, int n, NnCells g,
                                                            int* __restrict__ cell_of_point, int* __restrict__ counts,
                                                            float4* __restrict__ by_index) {
  nn_count_body(x, y, z, n, g, cell_of_point, counts, by_index, static_cast<int>(blockIdx.x));
}

__global__ __launch_bounds__(kThreads) void nn_scatter_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                              const float* __restrict__ z, int n,
                                                              const int* __restrict__ cell_of_point,
                                                              const int* __restrict__ cell_start, int* __restrict__ cursor,
                                                              float4* __restrict__ sorted) {
  nn_scatter_body(x, y, z, n, cell_of_point, cell_start, 0, cursor, sorted, static_cast<int>(blockIdx.x));
}

struct Best {
  float d2;
  int j;
};

// dliom.h: d2 = (dx*dx + dy*dy) + dz*dz in float, least d2, ties to the lowest j
__device__ __forceinline__ void consider(const float4 t, float px, float py, float pz, Best* b) {
  const float dx = px - t.x, dy = py - t.y, dz = pz - t.z;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  const int j = __float_as_int(t.w);
  if (d2 < b->d2 || (d2 == b->d2 && j < b->j)) {
    b->d2 = d2;
    b->j = j;
  }
}

__device__ __forceinline__ void scan_slots(const NnGridView& g, int first, int last, float px, float py, float pz, Best* b) {
  for (int k = first; k < last; ++k) consider(g.sorted[k], px, py, pz, b);
}

__device__ __forceinline__ void write_result(const NnSearch& s, int i, const Best& b, double max_d2) {
  const bool has = b.j != 0x7fffffff && static_cast<double>(b.d2) <= max_d2;
  s.j[i] = has ? b.j : -1;
  s.d2[i] = has ? b.d2 : __int_as_float(0x7f800000);
}

// STOP RULE.  Let q' be the query clamped into the box [lo, hi] axis by axis, c its cell, u(x) = fl(fl(x - lo) * inv) the
// float the cell function floors, and m = min over the axes of min(c + 1 - u(q'), u(q') - c), taken exactly (in double):
// how deep q' lies inside its own cell, in cells.  After the shells 0 .. s the query is settled when
//   (a) the cube [c - s, c + s]^3 holds the whole grid: nothing is unseen; or
//   (b) (double)best d2 < reach^2 (1 - 2^-21); or  (c) reach^2 (1 - 2^-21) > max_d2,   reach = (s + m - 0.01) / inv > 0.
// Proof of (b) and (c) against the FLOAT formula.  An unseen target t has, on some axis, a cell at least s + 1 away from
// c.  Take cell(t) >= c + s + 1 (the other side mirrors): cell(t) >= 1 is not clamped from below, so u(t) >= c + s + 1,
// and u(t) - u(q') >= s + (c + 1 - u(q')) >= s + m; on the other side u(t) < c - s gives u(q') - u(t) > s + (u(q') - c).
// (m may be negative for a q' on the box's upper face, where u(q') can reach dim: the rule then only stops later.)
// Both roundings of u are relative, |e| <= 2^-24 each (the subtraction is exact where it would underflow; an underflowing
// product errs by 2^-150 cells), so u(x) = (x - lo) inv (1 + d), |d| < 2^-22.9, and for x in the box (x - lo) inv < dim <=
// 1024 (the host chose dim = floor((hi - lo) inv) + 1).  Therefore (t - q') inv > s + m - 2 * 1024 * 2^-22.9 > s + m - 0.01,
// i.e. t - q' > reach as real numbers (edge = 1 / inv was rounded once, the device's product once more: 2^-52 each, far
// inside the margin below).  The query q itself lies on q' or beyond it, away from the box, so |q - t| >= |q' - t| and,
// rounding being monotone, |fl(q - t)| >= |fl(q' - t)| >= reach (1 - 2^-24).  Then fl(d_a * d_a) >= reach^2 (1 - 2^-24)^3 >
// reach^2 (1 - 2^-21) (reach^2 is far above the subnormals: the host keeps the edge >= 1e-6 and reach >= 0 is tested), and
// d2 = fl(fl(dx*dx + dy*dy) + dz*dz) >= fl(d_a * d_a) for each axis a, because adding a non-negative term to a float and
// rounding cannot go below that float.  So every unseen target's COMPUTED d2 is above the threshold: under (b) it is
// strictly worse than the best seen one (no tie to lose), under (c) it is beyond the correspondence distance like every
// other unseen one, and the best seen target decides.
__device__ __forceinline__ void nn_shell_body(const NnGridView& g, const NnSearch& s, double max_d2, int block) {
  const int i = block * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool searched = false, settled = false, non_finite = false;
  if (i < s.n) {
    const float px = s.px[i], py = s.py[i], pz = s.pz[i];
    Best b = {__int_as_float(0x7f800000), 0x7fffffff};
    if (!finite3(px, py, pz)) {
      non_finite = true;
      write_result(s, i, b, max_d2);
    } else if (g.n_finite == 0) {
      settled = true;
      write_result(s, i, b, max_d2);
    } else {
      searched = true;
      float ux, uy, uz;
      const int cx = nn_cell(fminf(fmaxf(px, g.lo[0]), g.hi[0]), g.lo[0], g.inv, g.dims[0], &ux);
      const int cy = nn_cell(fminf(fmaxf(py, g.lo[1]), g.hi[1]), g.lo[1], g.inv, g.dims[1], &uy);
      const int cz = nn_cell(fminf(fmaxf(pz, g.lo[2]), g.hi[2]), g.lo[2], g.inv, g.dims[2], &uz);
      // m of the stop rule: differences of a float and a small integer are exact in double.  (Under the one-cell grid
      // edge = 0 makes reach 0 or NaN and the threshold 0: nothing stops a walk there but (a), at shell 0.)
      const double inside = fmin(fmin(fmin(static_cast<double>(cx + 1) - ux, static_cast<double>(ux) - cx),
                                      fmin(static_cast<double>(cy + 1) - uy, static_cast<double>(uy) - cy)),
                                 fmin(static_cast<double>(cz + 1) - uz, static_cast<double>(uz) - cz));
      for (int sh = 0; sh <= kNnShells && !settled; ++sh) {
        const int z0 = max(cz - sh, 0), z1 = min(cz + sh, g.dims[2] - 1);
        const int y0 = max(cy - sh, 0), y1 = min(cy + sh, g.dims[1] - 1);
        const int x0 = max(cx - sh, 0), x1 = min(cx + sh, g.dims[0] - 1);
        for (int z = z0; z <= z1; ++z)
          for (int y = y0; y <= y1; ++y) {
            const int row = (z * g.dims[1] + y) * g.dims[0];
            if (abs(z - cz) == sh || abs(y - cy) == sh) {  // a face row of the shell: its cells are one run of slots
              scan_slots(g, g.cell_start[row + x0], g.cell_start[row + x1 + 1], px, py, pz, &b);
            } else {  // an inner row: the two end cells (0 < sh here)
              if (cx - sh >= 0) scan_slots(g, g.cell_start[row + cx - sh], g.cell_start[row + cx - sh + 1], px, py, pz, &b);
              if (cx + sh <= g.dims[0] - 1)
                scan_slots(g, g.cell_start[row + cx + sh], g.cell_start[row + cx + sh + 1], px, py, pz, &b);
            }
          }
        const bool whole = x0 == 0 && y0 == 0 && z0 == 0 && x1 == g.dims[0] - 1 && y1 == g.dims[1] - 1 && z1 == g.dims[2] - 1;
        const double reach = ((static_cast<double>(sh) + inside) - 0.01) * g.edge;
        const double threshold = reach > 0.0 ? (reach * reach) * (1.0 - 1.0 / 2097152.0) : 0.0;
        settled = whole || static_cast<double>(b.d2) < threshold || threshold > max_d2;
      }
      if (settled) write_result(s, i, b, max_d2);
    }
  }
  // the unsettled queries of the wave, in lane order, behind one integer atomic
  const bool listed = searched && !settled;
  const unsigned long long votes = __ballot(listed);
  const unsigned long long done = __ballot(settled);
  const unsigned long long bad = __ballot(non_finite);
  int base = 0;
  if (lane == 0) {
    if (votes != 0ull) base = atomicAdd(s.counters + kNnListCount, __popcll(votes));
    if (done != 0ull) atomicAdd(s.counters + kNnByGrid, __popcll(done));
    if (bad != 0ull) atomicAdd(s.counters + kNnNonFinite, __popcll(bad));
  }
  base = __shfl(base, 0, 64);
  if (listed) {
    s.list[base + __popcll(votes & ((1ull << lane) - 1ull))] = i;
    s.key[i] = ~0ull;  // nn_brute_kernel's atomicMin starts from "none"
  }
}

__global__ __launch_bounds__(kThreads) void nn_shell_kernel(NnGridView g, NnSearch s, double max_d2) {
  nn_shell_body(g, s, max_d2, static_cast<int>(blockIdx.x));
}

// listed: the queries list[0 .. counters[kNnListCount]); else every query (keys preset to ~0).  Workgroup (x, y) takes
// the tiles x, x + blocks, ... of 256 queries against the points [y * segment, (y + 1) * segment): both loops' bounds are
// the same for the whole workgroup and known on entry.  key = d2's bits << 32 | j orders like (d2, j): d2 >= +0.
__device__ __forceinline__ void nn_brute_body(const NnGridView& g, const NnSearch& s, bool listed, int segment, int block,
                                              int blocks, int segment_index) {
  __shared__ float4 tile[kTile];
  const int total = listed ? s.counters[kNnListCount] : s.n;
  const int first = segment_index * segment, last = min(first + segment, g.n_finite);
  for (int q0 = block * kThreads; q0 < total; q0 += blocks * kThreads) {
    const int k = q0 + threadIdx.x;
    const int i = k < total ? (listed ? s.list[k] : k) : -1;
    float px = 0.f, py = 0.f, pz = 0.f;
    bool live = false;
    if (i >= 0) {
      px = s.px[i];
      py = s.py[i];
      pz = s.pz[i];
      live = finite3(px, py, pz);
    }
    Best b = {__int_as_float(0x7f800000), 0x7fffffff};
    for (int base = first; base < last; base += kTile) {
      const int rows = min(kTile, last - base);
      __syncthreads();
      for (int e = threadIdx.x; e < rows; e += kThreads) tile[e] = g.sorted[base + e];
      __syncthreads();
      if (live) {
#pragma unroll 8
        for (int r = 0; r < rows; ++r) consider(tile[r], px, py, pz, &b);  // one address for the whole wave
      }
    }
    if (live && b.j != 0x7fffffff)
      atomicMin(s.key + i, (static_cast<unsigned long long>(__float_as_uint(b.d2)) << 32) | static_cast<unsigned>(b.j));
  }
}

__global__ __launch_bounds__(kThreads) void nn_brute_kernel(NnGridView g, NnSearch s, bool listed, int segment) {
  nn_brute_body(g, s, listed, segment, static_cast<int>(blockIdx.x), static_cast<int>(gridDim.x), static_cast<int>(blockIdx.y));
}

__device__ __forceinline__ void nn_resolve_body(const NnSearch& s, double max_d2, bool listed, int block) {
  const int total = listed ? s.counters[kNnListCount] : s.n;
  const int k = block * kThreads + threadIdx.x;
  if (block * kThreads >= total) return;  // the whole workgroup
  const int i = k < total ? (listed ? s.list[k] : k) : -1;
  bool live = false;
  if (i >= 0) {
    live = finite3(s.px[i], s.py[i], s.pz[i]);
    const unsigned long long key = s.key[i];
    Best b = {__int_as_float(0x7f800000), 0x7fffffff};
    if (live && key != ~0ull) {
      b.d2 = __uint_as_float(static_cast<unsigned>(key >> 32));
      b.j = static_cast<int>(key & 0xFFFFFFFFull);
    }
    write_result(s, i, b, max_d2);
  }
  const unsigned long long done = __ballot(live);
  const unsigned long long bad = __ballot(i >= 0 && !live);
  if ((threadIdx.x & 63) == 0) {
    if (done != 0ull) atomicAdd(s.counters + kNnByBruteForce, __popcll(done));
    if (bad != 0ull) atomicAdd(s.counters + kNnNonFinite, __popcll(bad));
  }
}

__global__ __launch_bounds__(kThreads) void nn_resolve_kernel(NnSearch s, double max_d2, bool listed) {
  nn_resolve_body(s, max_d2, listed, static_cast<int>(blockIdx.x));
}

// x/y/z may be ox/oy/oz: a lane reads its point before it writes it
__device__ __forceinline__ void nn_transform_body(const float* x, const float* y, const float* z, int n, const Rigid12& m, float* ox,
                                                  float* oy, float* oz, int block) {
  const int i = block * kThreads + threadIdx.x;
  if (i < n) {
    const double px = x[i], py = y[i], pz = z[i];
    const float rx = static_cast<float>(((m.m[0] * px + m.m[1] * py) + m.m[2] * pz) + m.m[3]);
    const float ry = static_cast<float>(((m.m[4] * px + m.m[5] * py) + m.m[6] * pz) + m.m[7]);
    const float rz = static_cast<float>(((m.m[8] * px + m.m[9] * py) + m.m[10] * pz) + m.m[11]);
    ox[i] = rx;
    oy[i] = ry;
    oz[i] = rz;
  }
}

__global__ __launch_bounds__(kThreads) void nn_transform_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                const float* __restrict__ z, int n, Rigid12 m, float* ox, float* oy,
                                                                float* oz) {
  nn_transform_body(x, y, z, n, m, ox, oy, oz, static_cast<int>(blockIdx.x));
}

// ---- the same bodies over a table of searches: blockIdx.y (z for the scan, whose y is the segment) is the pair.  A
// workgroup outside its pair's extent -- queries, segments -- leaves as a whole before any barrier or ballot.
__device__ __forceinline__ const NnBatchItem& nn_item(const char* table, size_t stride, unsigned pair) {
  return *reinterpret_cast<const NnBatchItem*>(table + stride * pair);
}

__global__ __launch_bounds__(kThreads) void nn_transform_batch_kernel(const char* __restrict__ table, size_t stride) {
  const NnBatchItem& d = nn_item(table, stride, blockIdx.y);
  const int block = static_cast<int>(blockIdx.x);
  if (d.transform == 0 || block * kThreads >= d.search.n) return;
  const Rigid12 m = d.m;
  nn_transform_body(d.sx, d.sy, d.sz, d.search.n, m, d.ox, d.oy, d.oz, block);
}

// a pair that searches by brute force has no walk: its keys are preset here, where nn_search_enqueue has a memset
__global__ __launch_bounds__(kThreads) void nn_shell_batch_kernel(const char* __restrict__ table, size_t stride) {
  const NnBatchItem& d = nn_item(table, stride, blockIdx.y);
  const int block = static_cast<int>(blockIdx.x);
  if (block * kThreads >= d.search.n) return;
  const NnSearch s = d.search;
  if (d.brute != 0) {
    const int i = block * kThreads + threadIdx.x;
    if (i < s.n) s.key[i] = ~0ull;
    return;
  }
  const NnGridView g = d.view;
  nn_shell_body(g, s, d.max_d2, block);
}

__global__ __launch_bounds__(kThreads) void nn_brute_batch_kernel(const char* __restrict__ table, size_t stride) {
  const NnBatchItem& d = nn_item(table, stride, blockIdx.z);
  const int block = static_cast<int>(blockIdx.x);
  if (static_cast<int>(blockIdx.y) >= d.segments || block * kThreads >= d.search.n) return;
  const NnGridView g = d.view;
  const NnSearch s = d.search;
  nn_brute_body(g, s, d.brute == 0, d.segment, block, static_cast<int>(gridDim.x), static_cast<int>(blockIdx.y));
}

__global__ __launch_bounds__(kThreads) void nn_resolve_batch_kernel(const char* __restrict__ table, size_t stride) {
  const NnBatchItem& d = nn_item(table, stride, blockIdx.y);
  const int block = static_cast<int>(blockIdx.x);
  if (block * kThreads >= d.search.n) return;
  const NnSearch s = d.search;
  nn_resolve_body(s, d.max_d2, d.brute == 0, block);
}

}  // namespace

NnGridView nn_view(const dliom_nn_index* index) {
  NnGridView g;
  g.sorted = index->sorted.as<float4>();
  g.by_index = index->by_index.as<float4>();
  g.cell_start = index->cell_start.as<int>();
  g.n_finite = static_cast<int>(index->n_finite);
  for (int a = 0; a < 3; ++a) {
    g.dims[a] = index->dims[a];
    g.lo[a] = index->lo[a];
    g.hi[a] = index->hi[a];
  }
  g.inv = index->inv;
  g.edge = index->edge;
  return g;
}
dliom_ctx* nn_ctx(const dliom_nn_index* index) { return index->ctx; }
DevBuf* nn_scratch(dliom_nn_index* index) { return &index->scratch; }
int* nn_poll_us(dliom_nn_index* index) { return &index->poll_us; }

// segments of about kBruteSegment (kListedSegment) points, at most 256 of them
void nn_batch_item(const dliom_nn_index* index, int search, NnBatchItem* item) {
  item->view = nn_view(index);
  const bool brute = search == DLIOM_NN_BRUTE_FORCE || (search == DLIOM_NN_AUTO && index->search == DLIOM_NN_BRUTE_FORCE);
  item->brute = brute ? 1 : 0;
  const int wanted = brute ? kBruteSegment : kListedSegment;
  item->segments = std::max(1, std::min(256, (item->view.n_finite + wanted - 1) / wanted));
  item->segment = std::max(1, (item->view.n_finite + item->segments - 1) / item->segments);
}

int nn_search_enqueue(dliom_nn_index* index, const NnSearch& s, double max_d2, int search) {
  if (s.n <= 0) return DLIOM_OK;
  hipStream_t stream = index->ctx->stream;
  NnBatchItem geometry;
  nn_batch_item(index, search, &geometry);
  const NnGridView g = geometry.view;
  const dim3 grid(blocks_of(s.n, kThreads)), block(kThreads);
  const bool brute = geometry.brute != 0;
  if (brute)
    DLIOM_HIP_TRY(hipMemsetAsync(s.key, 0xFF, sizeof(unsigned long long) * static_cast<size_t>(s.n), stream));
  else
    hipLaunchKernelGGL(nn_shell_kernel, grid, block, 0, stream, g, s, max_d2);
  // tiles of queries strided over at most 128 workgroups
  const dim3 brute_grid(std::min(grid.x, 128u), static_cast<unsigned>(geometry.segments));
  hipLaunchKernelGGL(nn_brute_kernel, brute_grid, block, 0, stream, g, s, !brute, geometry.segment);
  hipLaunchKernelGGL(nn_resolve_kernel, grid, block, 0, stream, s, max_d2, !brute);
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

// Launches sized by the largest pair of the table; a key cannot be lost to the stride of the tiles (an atomicMin's result
// does not depend on which workgroup brought a segment's best).  A launch holds at most 2^30 lanes: a table of many large
// pairs goes in runs of pairs, one behind the other.
int nn_batch_pairs_per_launch(int max_n) { return std::max(1, (1 << 22) / static_cast<int>(blocks_of(std::max(max_n, 1), kThreads))); }

int nn_search_batch_enqueue(dliom_ctx* ctx, const void* table, size_t stride, int count, int max_n, int max_segments) {
  if (count <= 0 || max_n <= 0) return DLIOM_OK;
  const unsigned blocks = blocks_of(max_n, kThreads);
  const dim3 block(kThreads);
  const int run = nn_batch_pairs_per_launch(max_n);
  for (int first = 0; first < count; first += run) {
    const char* const t = static_cast<const char*>(table) + stride * static_cast<size_t>(first);
    const unsigned pairs = static_cast<unsigned>(std::min(run, count - first));
    hipLaunchKernelGGL(nn_shell_batch_kernel, dim3(blocks, pairs), block, 0, ctx->stream, t, stride);
    hipLaunchKernelGGL(nn_brute_batch_kernel, dim3(std::min(blocks, 128u), static_cast<unsigned>(std::max(max_segments, 1)), pairs),
                       block, 0, ctx->stream, t, stride);
    hipLaunchKernelGGL(nn_resolve_batch_kernel, dim3(blocks, pairs), block, 0, ctx->stream, t, stride);
  }
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

int nn_transform_batch_enqueue(dliom_ctx* ctx, const void* table, size_t stride, int count, int max_n) {
  if (count <= 0 || max_n <= 0) return DLIOM_OK;
  const int run = nn_batch_pairs_per_launch(max_n);
  for (int first = 0; first < count; first += run)
    hipLaunchKernelGGL(nn_transform_batch_kernel, dim3(blocks_of(max_n, kThreads), static_cast<unsigned>(std::min(run, count - first))),
                       dim3(kThreads), 0, ctx->stream, static_cast<const char*>(table) + stride * static_cast<size_t>(first), stride);
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

int nn_transform_enqueue(dliom_ctx* ctx, const float* x, const float* y, const float* z, int n, const Rigid12& m, float* ox,
                         float* oy, float* oz) {
  if (n <= 0) return DLIOM_OK;
  hipLaunchKernelGGL(nn_transform_kernel, dim3(blocks_of(n, kThreads)), dim3(kThreads), 0, ctx->stream, x, y, z, n, m, ox, oy, oz);
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

}  // namespace dliom

extern "C" {

int dliom_nn_index_create(dliom_ctx* ctx, const dliom_cloud* target, const dliom_nn_index_options* options,
                          dliom_nn_index** index) {
  using namespace dliom;
  if (ctx == nullptr || target == nullptr || index == nullptr || target->ctx != ctx) return DLIOM_ERR_INVALID_ARGUMENT;
  if (target->n < 1 || target->n > DLIOM_NN_MAX_POINTS) return DLIOM_ERR_INVALID_ARGUMENT;
  double edge0 = 0.0;
  int search = DLIOM_NN_AUTO;
  if (!nn_index_options_ok(options, &edge0, &search)) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const int n = static_cast<int>(target->n);
  struct Guard {  // a failure on the way frees what was made
    dliom_nn_index* p;
    ~Guard() { dliom_nn_index_destroy(p); }
  } guard{new dliom_nn_index()};
  dliom_nn_index* f = guard.p;
  f->ctx = ctx;
  f->n_target = n;
  f->search = search;
  // the bounding box of the finite points: one polled read-back
  const size_t ids_bytes = align256(4 * static_cast<size_t>(n));
  DLIOM_TRY(f->scratch.reserve(256 + ids_bytes));
  unsigned* const words = f->scratch.as<unsigned>();
  int* const cell_of_point = reinterpret_cast<int*>(f->scratch.as<char>() + 256);
  const FillJob fills[2] = {{words, 16, 0xFFFFFFFFu}, {words + 4, 16, 0u}};
  DLIOM_TRY(fill_multi(ctx, fills, 2));
  const dim3 grid(blocks_of(n, kThreads)), block(kThreads);
  hipLaunchKernelGGL(nn_box_kernel, grid, block, 0, ctx->stream, target->d_x, target->d_y, target->d_z, n, words);
  DLIOM_HIP_TRY(hipGetLastError());
  unsigned* const host = pinned_at<unsigned>(ctx, kPinReadback);
  const GatherJob job{words, 8};
  DLIOM_TRY(gather_and_wait(ctx, &job, 1, host));
  nn_set_grid(f, host, host + 4, edge0);
  const size_t cells = static_cast<size_t>(f->dims[0]) * f->dims[1] * f->dims[2];
  // counting sort by cell: populations, their exclusive sum (cells + 1 entries: the last is the total), scatter
  size_t tmp = 0;
  DLIOM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, static_cast<const int*>(nullptr), static_cast<int*>(nullptr),
                                                 static_cast<int>(cells + 1), ctx->stream));
  const size_t per = align256(4 * (cells + 1));
  DevBuf work;  // populations | cursors | the scan's storage
  struct Release {
    DevBuf* b;
    ~Release() { b->release(); }
  } release{&work};
  DLIOM_TRY(work.reserve(2 * per + align256(tmp)));
  DLIOM_TRY(f->cell_start.reserve(per));
  DLIOM_TRY(f->sorted.reserve(std::max<size_t>(16, 16 * static_cast<size_t>(f->n_finite))));
  DLIOM_TRY(f->by_index.reserve(16 * static_cast<size_t>(n)));
  int* const counts = work.as<int>();
  int* const cursor = reinterpret_cast<int*>(work.as<char>() + per);
  DLIOM_HIP_TRY(hipMemsetAsync(work.p, 0, 2 * per, ctx->stream));
  const NnCells g = nn_cells_of(f);
  hipLaunchKernelGGL(nn_count_kernel, grid, block, 0, ctx->stream, target->d_x, target->d_y, target->d_z, n, g, cell_of_point, counts,
                     f->by_index.as<float4>());
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(work.as<char>() + 2 * per, tmp, counts, f->cell_start.as<int>(),
                                                 static_cast<int>(cells + 1), ctx->stream));
  hipLaunchKernelGGL(nn_scatter_kernel, grid, block, 0, ctx->stream, target->d_x, target->d_y, target->d_z, n, cell_of_point,
                     f->cell_start.as<int>(), cursor, f->sorted.as<float4>());
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // `work` goes; the target cloud is the caller's again
  ++ctx->host_syncs;
  guard.p = nullptr;
  *index = f;
  return DLIOM_OK;
}

void dliom_nn_index_destroy(dliom_nn_index* index) {
  if (index == nullptr) return;
  (void)hipSetDevice(index->ctx->device);
  (void)hipStreamSynchronize(index->ctx->stream);
  if (index->slab.p != nullptr) index->sorted = index->by_index = index->cell_start = dliom::DevBuf{};  // views into the slab
  index->slab.release();
  index->sorted.release();
  index->by_index.release();
  index->cell_start.release();
  index->scratch.release();
  delete index;
}

int dliom_nn_index_memory_stats(const dliom_nn_index* index, dliom_nn_index_memory* out) {
  if (index == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  out->points = index->n_target;
  out->finite_points = index->n_finite;
  out->cells = static_cast<int64_t>(index->dims[0]) * index->dims[1] * index->dims[2];
  for (int a = 0; a < 3; ++a) out->dims[a] = index->dims[a];
  out->index_bytes = static_cast<int64_t>(index->sorted.cap + index->by_index.cap + index->cell_start.cap);
  out->scratch_bytes = static_cast<int64_t>(index->scratch.cap);
  out->cell_edge = index->edge;
  return DLIOM_OK;
}

int dliom_nn_index_query(dliom_nn_index* index, const dliom_cloud* queries, const double* transform16, double max_distance,
                         int search, int32_t* j_out, float* d2_out, dliom_nn_query_stats* stats) {
  using namespace dliom;
  if (index == nullptr || queries == nullptr || queries->ctx != index->ctx || queries->n < 0 || queries->n > DLIOM_NN_MAX_POINTS)
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (queries->n > 0 && (j_out == nullptr || d2_out == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (std::isnan(max_distance) || max_distance < 0.0 || (search != DLIOM_NN_AUTO && search != DLIOM_NN_BRUTE_FORCE))
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (transform16 != nullptr)
    for (int k = 0; k < 16; ++k)
      if (!std::isfinite(transform16[k])) return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_nn_query_stats st = {};
  st.queries = queries->n;
  dliom_ctx* ctx = index->ctx;
  const int n = static_cast<int>(queries->n);
  if (n > 0) {
    DLIOM_HIP_TRY(hipSetDevice(ctx->device));
    const size_t per = align256(4 * static_cast<size_t>(n));
    DLIOM_TRY(index->scratch.reserve(256 + 8 * per));
    char* const base = index->scratch.as<char>();
    int* const counters = reinterpret_cast<int*>(base);
    float* const px = reinterpret_cast<float*>(base + 256);
    float* const py = reinterpret_cast<float*>(base + 256 + per);
    float* const pz = reinterpret_cast<float*>(base + 256 + 2 * per);
    NnSearch s;
    s.px = queries->d_x;
    s.py = queries->d_y;
    s.pz = queries->d_z;
    s.n = n;
    s.j = reinterpret_cast<int*>(base + 256 + 3 * per);
    s.d2 = reinterpret_cast<float*>(base + 256 + 4 * per);
    s.list = reinterpret_cast<int*>(base + 256 + 5 * per);
    s.key = reinterpret_cast<unsigned long long*>(base + 256 + 6 * per);
    s.counters = counters;
    const FillJob fill{counters, 16, 0u};
    DLIOM_TRY(fill_multi(ctx, &fill, 1));
    if (transform16 != nullptr) {
      Rigid12 m;
      std::memcpy(m.m, transform16, sizeof(m.m));
      DLIOM_TRY(nn_transform_enqueue(ctx, queries->d_x, queries->d_y, queries->d_z, n, m, px, py, pz));
      s.px = px;
      s.py = py;
      s.pz = pz;
    }
    const bool timed = ctx->profiling && stats != nullptr;
    struct Events {  // destroyed on every way out
      hipEvent_t e[2] = {nullptr, nullptr};
      ~Events() {
        for (hipEvent_t x : e)
          if (x != nullptr) (void)hipEventDestroy(x);
      }
    } events;
    if (timed) {
      for (hipEvent_t& e : events.e) DLIOM_HIP_TRY(hipEventCreate(&e));
      DLIOM_HIP_TRY(hipEventRecord(events.e[0], ctx->stream));
    }
    DLIOM_TRY(nn_search_enqueue(index, s, max_distance * max_distance, search));
    if (timed) DLIOM_HIP_TRY(hipEventRecord(events.e[1], ctx->stream));
    int host_counters[kNnCounterWords];
    DLIOM_HIP_TRY(hipMemcpyAsync(j_out, s.j, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipMemcpyAsync(d2_out, s.d2, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipMemcpyAsync(host_counters, counters, sizeof(host_counters), hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    ++ctx->host_syncs;
    st.read_backs = 1;
    st.settled_by_grid = host_counters[kNnByGrid];
    st.settled_by_brute_force = host_counters[kNnByBruteForce];
    st.non_finite = host_counters[kNnNonFinite];
    if (timed) {
      float ms = 0.f;
      DLIOM_HIP_TRY(hipEventElapsedTime(&ms, events.e[0], events.e[1]));
      st.search_ms = ms;
    }
  }
  if (stats != nullptr) *stats = st;
  return DLIOM_OK;
}

}  // extern "C"
