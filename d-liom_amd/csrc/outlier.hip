// Moving-object removal of the points-processor pipeline on the device: io::OutlierRemovingPointsProcessor
// (io/outlier_removing_points_processor.{h,cc}, action "voxel_filter_and_remove_moving_objects") and
// io::MinMaxRangeFiteringPointsProcessor (io/min_max_range_filtering_points_processor.cc), equal to the reference
// count for count.
//
// The reference keeps a HybridGridBase<VoxelData {int hits; int rays;}> and streams every batch three times: mark
// hits, count the rays that pass through voxels with hits, drop the points of voxels with rays >= 3 * hits.  Here the
// grid is a sparse table in HBM:
//   * a hash table "leaf key -> slot" (open addressing, linear probing, 64-bit keys: three 11-bit leaf coordinates),
//     a leaf being the 8x8x8 block of voxels that the reference's FlatGrid is;
//   * a pool of leaves, slot * 1024 ints: {hits, rays} of cell ((z&7)<<6 | (y&7)<<3 | (x&7)) side by side, so that the
//     samples of a ray, which move one voxel at a time, stay in the cache lines of one leaf for several steps.
// Only pass 1 inserts, and the table and the pool grow between launches.  Passes 2 and 3 look up and add to `rays`.
// Everything accumulated is a 32-bit integer, so no result depends on the order of the atomics; everything that decides
// a voxel is float arithmetic in the reference's order, without contraction, with IEEE division and square root.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "voxel_hash.h"

// Leaf edge 2^kLeafBits voxels.  3: the layout that ships.  0 turns the table into a flat hash of single voxels (an
// experiment build: tools/outlier_bench.py --lib, DESIGN.md section 3.10 for the comparison).
#ifndef DLIOM_OUTLIER_LEAF_BITS
#define DLIOM_OUTLIER_LEAF_BITS 3
#endif

namespace dliom {
namespace {

constexpr int kLeafBits = DLIOM_OUTLIER_LEAF_BITS;
constexpr int kLeafCells = 1 << (3 * kLeafBits);
constexpr int kLeafInts = 2 * kLeafCells;  // {hits, rays} per cell
constexpr int kLeafMask = (1 << kLeafBits) - 1;
constexpr unsigned kFlagRayTooLong = 4u;  // beside kFlagNonFinite and kFlagExtent
constexpr int kBlock = 256;

// device words of a remover
enum { kWordLeaves = 0, kWordFlag = 1, kWordSamples = 2 /* u64 */, kWordProbes = 4 /* u64 */, kWordCursor = 6 /* u64 */, kNumWords = 8 };

struct TableView {
  uint64_t* keys;    // capacity entries, kEmptyKey: free
  unsigned* slots;   // slot of the entry's leaf
  unsigned mask;     // capacity - 1 (a power of two)
  int* pool;         // slot * kLeafInts + 2 * cell: hits, + 1: rays
  float resolution;  // float(voxel_size): HybridGridBase(const float resolution)
};

__device__ __forceinline__ uint64_t leaf_key(int cx, int cy, int cz) { return dliom::leaf_key(cx, cy, cz, kLeafBits); }
__device__ __forceinline__ int cell_in_leaf(int cx, int cy, int cz) { return dliom::cell_in_leaf(cx, cy, cz, kLeafBits); }

// slot of the leaf `key`, kNoSlot if the table has none; *probes += entries read
__device__ __forceinline__ unsigned find_leaf(const TableView& t, uint64_t key, unsigned* probes) {
  return hash_find(t.keys, t.slots, t.mask, key, probes);
}

// ---- pass 1 -----------------------------------------------------------------------------------------------------
// What the reference would abort on (a hit the grid cannot grow to) or leaves undefined (lround of a non-finite float)
// is found before anything is inserted.
__global__ __launch_bounds__(kBlock) void outlier_check_hits_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                    const float* __restrict__ z, unsigned n, float resolution,
                                                                    unsigned* __restrict__ words) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  unsigned flag = 0;
  int c;
  if (!finite3(x[i], y[i], z[i])) flag = kFlagNonFinite;
  else if (!cell_in_extent(x[i], resolution, &c) || !cell_in_extent(y[i], resolution, &c) || !cell_in_extent(z[i], resolution, &c))
    flag = kFlagExtent;
  if (flag != 0) atomicOr(&words[kWordFlag], flag);
}

// Leaves of the batch's hits that the table does not hold yet: key claimed with one compare-and-swap, slot taken from
// the counter by the winner.  Nothing waits for another thread: the hits themselves are counted by the next launch.
__global__ __launch_bounds__(kBlock) void outlier_insert_leaves_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                       const float* __restrict__ z, unsigned n, TableView t,
                                                                       uint64_t* __restrict__ slot_key, unsigned* __restrict__ words) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || words[kWordFlag] != 0u) return;
  int cx, cy, cz;
  if (!cell_in_extent(x[i], t.resolution, &cx) || !cell_in_extent(y[i], t.resolution, &cy) || !cell_in_extent(z[i], t.resolution, &cz))
    return;  // (flagged by the check kernel)
  hash_claim(t.keys, t.slots, t.mask, leaf_key(cx, cy, cz), &words[kWordLeaves], slot_key);
}

__global__ __launch_bounds__(kBlock) void outlier_mark_hits_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                   const float* __restrict__ z, unsigned n, TableView t) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int cx, cy, cz;
  if (!cell_in_extent(x[i], t.resolution, &cx) || !cell_in_extent(y[i], t.resolution, &cy) || !cell_in_extent(z[i], t.resolution, &cz))
    return;
  unsigned probes = 0;
  const unsigned slot = find_leaf(t, leaf_key(cx, cy, cz), &probes);
  if (slot == kNoSlot) return;  // (cannot happen: inserted by the launch before)
  atomicAdd(&t.pool[static_cast<size_t>(slot) * kLeafInts + 2 * cell_in_leaf(cx, cy, cz)], 1);  // ++hits (.cc:88)
}

// ---- pass 2 -----------------------------------------------------------------------------------------------------
// delta.norm() of a Vector3f: Eigen's reduction order (preprocess.hip's range)
__device__ __forceinline__ float norm3(float dx, float dy, float dz) { return sqrtf(dx * dx + (dy * dy + dz * dz)); }

// A ray whose loop would not end in the reference: `x += voxel_size_` stops advancing once voxel_size is below half
// an ulp of x.  Below voxel_size * 2^24 every step advances (ulp(x) <= x * 2^-23 < 2 * voxel_size).
__global__ __launch_bounds__(kBlock) void outlier_check_rays_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                    const float* __restrict__ z, unsigned n, float ox, float oy,
                                                                    float oz, double length_limit, unsigned* __restrict__ words) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  unsigned flag = 0;
  if (!finite3(x[i], y[i], z[i])) flag = kFlagNonFinite;
  else if (!(static_cast<double>(norm3(x[i] - ox, y[i] - oy, z[i] - oz)) < length_limit)) flag = kFlagRayTooLong;
  if (flag != 0) atomicOr(&words[kWordFlag], flag);
}

// ProcessInPhaseTwo (.cc:92-108), one ray a thread.  The leaf of the previous sample stays in registers: a ray moves one
// voxel a step, so the hash table is asked once per leaf crossed, not once per sample.
__global__ __launch_bounds__(kBlock) void outlier_count_rays_kernel(const float* __restrict__ px, const float* __restrict__ py,
                                                                    const float* __restrict__ pz, unsigned n, float ox, float oy,
                                                                    float oz, double voxel_size, TableView t,
                                                                    unsigned* __restrict__ words) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  unsigned samples = 0, probes = 0;
  if (i < n && words[kWordFlag] == 0u) {
    const float dx = px[i] - ox, dy = py[i] - oy, dz = pz[i] - oz;  // delta = points[i] - origin
    const float length = norm3(dx, dy, dz);
    uint64_t last_key = kEmptyKey;
    unsigned slot = kNoSlot;
    for (float x = 0.f; x < length; x = static_cast<float>(static_cast<double>(x) + voxel_size)) {  // x += voxel_size_ (double)
      ++samples;
      const float s = x / length;
      int cx, cy, cz;  // GetCellIndex(origin + (x / length) * delta)
      if (!cell_in_extent(ox + s * dx, t.resolution, &cx) || !cell_in_extent(oy + s * dy, t.resolution, &cy) ||
          !cell_in_extent(oz + s * dz, t.resolution, &cz))
        continue;  // value() outside the grid: ValueType(), hits == 0 (hybrid_grid.h:266-271)
      const uint64_t key = leaf_key(cx, cy, cz);
      if (key != last_key) {
        slot = find_leaf(t, key, &probes);
        last_key = key;
      }
      if (slot == kNoSlot) continue;
      int* cell = &t.pool[static_cast<size_t>(slot) * kLeafInts + 2 * cell_in_leaf(cx, cy, cz)];
      if (cell[0] > 0) atomicAdd(&cell[1], 1);  // if (hits > 0) ++rays
    }
  }
  samples = wave_sum_lane63(samples);  // < 2^24 a ray: no overflow
  probes = wave_sum_lane63(probes);
  if ((threadIdx.x & 63u) == 63u && samples != 0u) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&words[kWordSamples]), static_cast<unsigned long long>(samples));
    atomicAdd(reinterpret_cast<unsigned long long*>(&words[kWordProbes]), static_cast<unsigned long long>(probes));
  }
}

// ---- pass 3 and the range filter: a keep flag per point, then compact.hip's order-preserving compaction ------------------
// One atomic a kept point, not device_common.h's norm_word and wavefront fold: the two kernels here leave early for
// i >= n, and on norm_word (a select, then a test for zero) they are no longer the instructions that were measured.
__device__ __forceinline__ void note_kept(float x, float y, float z, unsigned* max_sq) {
  const float sq = x * x + (y * y + z * z);  // cloud_max_norm's order; bit patterns of non-negative floats keep their order
  if (sq == sq) atomicMax(max_sq, __float_as_uint(sq));
}

// ProcessInPhaseThree (.cc:110-124): removed when !(rays < 3.0 * hits) -- exact in integers as well
__global__ __launch_bounds__(kBlock) void outlier_keep_flags_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                    const float* __restrict__ z, unsigned n, TableView t,
                                                                    unsigned* __restrict__ keep, unsigned* __restrict__ words,
                                                                    unsigned* __restrict__ max_sq) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  unsigned k = 0;
  if (!finite3(x[i], y[i], z[i])) {
    atomicOr(&words[kWordFlag], kFlagNonFinite);
  } else {
    int cx, cy, cz;
    if (cell_in_extent(x[i], t.resolution, &cx) && cell_in_extent(y[i], t.resolution, &cy) && cell_in_extent(z[i], t.resolution, &cz)) {
      unsigned probes = 0;
      const unsigned slot = find_leaf(t, leaf_key(cx, cy, cz), &probes);
      if (slot != kNoSlot) {
        const int* cell = &t.pool[static_cast<size_t>(slot) * kLeafInts + 2 * cell_in_leaf(cx, cy, cz)];
        k = static_cast<long long>(cell[1]) < 3ll * cell[0] ? 1u : 0u;
      }
    }  // outside the grid: VoxelData(), !(0 < 0): removed
  }
  keep[i] = k;
  if (k) note_kept(x[i], y[i], z[i], max_sq);
}

// MinMaxRangeFiteringPointsProcessor::Process (.cc:40-51): float range, double bounds
__global__ __launch_bounds__(kBlock) void range_keep_flags_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                  const float* __restrict__ z, unsigned n, float ox, float oy,
                                                                  float oz, double min_range, double max_range,
                                                                  unsigned* __restrict__ keep, unsigned* __restrict__ max_sq) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double range = static_cast<double>(norm3(x[i] - ox, y[i] - oy, z[i] - oz));
  const unsigned k = (min_range <= range && range <= max_range) ? 1u : 0u;
  keep[i] = k;
  if (k) note_kept(x[i], y[i], z[i], max_sq);
}

// ---- the table's contents (tests, statistics) -----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void outlier_count_voxels_kernel(const int* __restrict__ pool, unsigned long long cells,
                                                                      unsigned* __restrict__ words) {
  const unsigned long long c = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  const int hit = c < cells && pool[2 * c] > 0 ? 1 : 0;
  const int total = __syncthreads_count(hit);
  if (threadIdx.x == 0 && total > 0)
    atomicAdd(reinterpret_cast<unsigned long long*>(&words[kWordCursor]), static_cast<unsigned long long>(total));
}

struct VoxelRecord {
  uint64_t key;  // (z, y, x) biased, z most significant
  int hits, rays;
};

__global__ __launch_bounds__(kBlock) void outlier_emit_voxels_kernel(const int* __restrict__ pool, const uint64_t* __restrict__ slot_key,
                                                                     unsigned long long cells, unsigned long long capacity,
                                                                     VoxelRecord* __restrict__ out, unsigned* __restrict__ words) {
  const unsigned long long c = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (c >= cells || pool[2 * c] <= 0) return;
  const unsigned long long at = atomicAdd(reinterpret_cast<unsigned long long*>(&words[kWordCursor]), 1ull);
  if (at >= capacity) return;
  const uint64_t lk = slot_key[c / kLeafCells];
  const unsigned in = static_cast<unsigned>(c % kLeafCells);
  const uint64_t vx = ((lk & kKeyMask) << kLeafBits) | (in & kLeafMask);
  const uint64_t vy = (((lk >> 14) & kKeyMask) << kLeafBits) | ((in >> kLeafBits) & kLeafMask);
  const uint64_t vz = (((lk >> 28) & kKeyMask) << kLeafBits) | ((in >> (2 * kLeafBits)) & kLeafMask);
  out[at] = VoxelRecord{(vz << 28) | (vy << 14) | vx, pool[2 * c], pool[2 * c + 1]};
}

inline unsigned blocks_of(int64_t n) { return dliom::blocks_of(n, kBlock); }

int status_of_ray_flag(unsigned flag) {  // the shared bits first
  const int st = status_of_flag(flag);
  return st == DLIOM_OK && (flag & kFlagRayTooLong) ? DLIOM_ERR_RAY_TOO_LONG : st;
}

bool finite_origin(const float o[3]) { return std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]); }

}  // namespace
}  // namespace dliom

using namespace dliom;

struct dliom_outlier_remover {
  dliom_ctx* ctx = nullptr;
  std::shared_ptr<MemoryLedger> ledger;
  double voxel_size = 0.0;  // voxel_size_ stays double (.h:79)
  float resolution = 0.f;   // voxels_(voxel_size_): HybridGridBase(const float)
  int phase = 1;            // State (.h:59-63)
  KeyTable table;         // leaf key -> slot
  int* d_pool = nullptr;  // leaf_capacity leaves; those past `leaves` are zero
  int64_t leaf_capacity = 0;
  int64_t leaves = 0;  // exact: read back by every mark_hits
  unsigned* d_words = nullptr;
  int64_t growths = 0, booked = 0;

  TableView view() const {
    const HashView t = table.view();
    return TableView{t.keys, t.slots, t.mask, d_pool, resolution};
  }
  int64_t bytes() const { return table.bytes() + leaf_capacity * kLeafInts * 4 + kNumWords * 4; }
  void book() {
    if (ledger) ledger->outlier_table_bytes += bytes() - booked;
    booked = bytes();
  }
  int grow_pool(int64_t want_leaves);
};

int dliom_outlier_remover::grow_pool(int64_t want_leaves) {
  if (want_leaves <= leaf_capacity) return DLIOM_OK;
  const int64_t cap = std::max<int64_t>(want_leaves, leaf_capacity + leaf_capacity / 2);
  int* pool = nullptr;
  DLIOM_TRY(grown_copy(ctx, d_pool, leaves * kLeafInts, cap * kLeafInts, &pool));
  if (d_pool) (void)hipFree(d_pool);
  d_pool = pool;
  if (leaf_capacity > 0) ++growths;
  leaf_capacity = cap;
  book();
  return DLIOM_OK;
}

// Pass 3's keep flags of `points` (n > 0) into freshly carved scratch, for the cloud and the batch entry point
static int flag_by_voxels(dliom_outlier_remover* r, const dliom_cloud* points, CompactScratch* s) {
  dliom_ctx* ctx = r->ctx;
  const unsigned n = static_cast<unsigned>(points->n);
  DLIOM_TRY(carve_compact(ctx, points->n, s));
  const FillJob fill{r->d_words + kWordFlag, 4, 0u};
  DLIOM_TRY(fill_multi(ctx, &fill, 1));
  hipLaunchKernelGGL(outlier_keep_flags_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, points->d_x, points->d_y,
                     points->d_z, n, r->view(), s->keep, r->d_words, s->max_sq);
  return hipGetLastError() == hipSuccess ? DLIOM_OK : DLIOM_ERR_HIP;
}

static int flag_by_range(dliom_ctx* ctx, const dliom_cloud* in, const float origin[3], double min_range, double max_range,
                         CompactScratch* s) {
  const unsigned n = static_cast<unsigned>(in->n);
  DLIOM_TRY(carve_compact(ctx, in->n, s));
  hipLaunchKernelGGL(range_keep_flags_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, in->d_x, in->d_y, in->d_z, n,
                     origin[0], origin[1], origin[2], min_range, max_range, s->keep, s->max_sq);
  return hipGetLastError() == hipSuccess ? DLIOM_OK : DLIOM_ERR_HIP;
}

extern "C" {

int dliom_outlier_remover_create(dliom_ctx* ctx, double voxel_size, dliom_outlier_remover** out) {
  if (ctx == nullptr || out == nullptr || !(voxel_size > 0.0) || !std::isfinite(voxel_size) ||
      !(static_cast<float>(voxel_size) > 0.f) || !std::isfinite(static_cast<float>(voxel_size)))
    return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  dliom_outlier_remover* r = new dliom_outlier_remover;
  r->ctx = ctx;
  r->ledger = ctx->ledger;
  r->voxel_size = voxel_size;
  r->resolution = static_cast<float>(voxel_size);
  int st = hipMalloc(&r->d_words, kNumWords * 4) == hipSuccess ? DLIOM_OK : DLIOM_ERR_HIP;
  if (st == DLIOM_OK && hipMemsetAsync(r->d_words, 0, kNumWords * 4, ctx->stream) != hipSuccess) st = DLIOM_ERR_HIP;
  if (st == DLIOM_OK) st = r->table.grow(ctx, 512, 0, &r->growths);
  if (st == DLIOM_OK) st = r->grow_pool(64);
  if (st != DLIOM_OK) {
    dliom_outlier_remover_destroy(r);
    return st;
  }
  *out = r;
  return DLIOM_OK;
}

int dliom_outlier_remover_destroy(dliom_outlier_remover* r) {
  if (r == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  (void)hipSetDevice(r->ctx->device);
  (void)hipStreamSynchronize(r->ctx->stream);
  r->table.release();
  if (r->d_pool) (void)hipFree(r->d_pool);
  if (r->d_words) (void)hipFree(r->d_words);
  if (r->ledger) r->ledger->outlier_table_bytes -= r->booked;
  delete r;
  return DLIOM_OK;
}

int dliom_outlier_remover_mark_hits(dliom_outlier_remover* r, const dliom_cloud* points) {
  if (r == nullptr || points == nullptr || r->phase != 1 || points->n > INT32_MAX) return DLIOM_ERR_INVALID_ARGUMENT;
  if (points->n == 0) return DLIOM_OK;
  dliom_ctx* ctx = r->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const unsigned n = static_cast<unsigned>(points->n);
  // every hit in a leaf of its own: the bound the call knows
  DLIOM_TRY(r->table.grow(ctx, r->leaves + points->n, r->leaves, &r->growths));
  r->book();
  const FillJob fill{r->d_words + kWordFlag, 4, 0u};
  DLIOM_TRY(fill_multi(ctx, &fill, 1));
  hipLaunchKernelGGL(outlier_check_hits_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, points->d_x, points->d_y,
                     points->d_z, n, r->resolution, r->d_words);
  hipLaunchKernelGGL(outlier_insert_leaves_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, points->d_x, points->d_y,
                     points->d_z, n, r->view(), r->table.slot_key, r->d_words);
  DLIOM_HIP_TRY(hipGetLastError());
  unsigned host[2];
  DLIOM_TRY(read_words(ctx, r->d_words, 0, 2, host));  // leaves, flag
  if (host[kWordFlag] != 0u) return status_of_flag(host[kWordFlag]);  // nothing was inserted
  const int64_t leaves = host[kWordLeaves];
  DLIOM_TRY(r->grow_pool(leaves));  // copies the `r->leaves` leaves in use; the new ones are zero
  r->leaves = leaves;
  hipLaunchKernelGGL(outlier_mark_hits_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, points->d_x, points->d_y,
                     points->d_z, n, r->view());
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

int dliom_outlier_remover_count_rays(dliom_outlier_remover* r, const float origin[3], const dliom_cloud* points) {
  if (r == nullptr || origin == nullptr || points == nullptr || r->phase > 2 || points->n > INT32_MAX || !finite_origin(origin))
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (points->n == 0) {
    r->phase = 2;
    return DLIOM_OK;
  }
  dliom_ctx* ctx = r->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const unsigned n = static_cast<unsigned>(points->n);
  const FillJob fill{r->d_words + kWordFlag, 4, 0u};
  DLIOM_TRY(fill_multi(ctx, &fill, 1));
  hipLaunchKernelGGL(outlier_check_rays_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, points->d_x, points->d_y,
                     points->d_z, n, origin[0], origin[1], origin[2], r->voxel_size * 16777216.0, r->d_words);
  hipLaunchKernelGGL(outlier_count_rays_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, points->d_x, points->d_y,
                     points->d_z, n, origin[0], origin[1], origin[2], r->voxel_size, r->view(), r->d_words);
  DLIOM_HIP_TRY(hipGetLastError());
  unsigned flag;
  DLIOM_TRY(read_words(ctx, r->d_words, kWordFlag, 1, &flag));
  if (flag != 0u) return status_of_ray_flag(flag);  // no ray was walked
  r->phase = 2;
  return DLIOM_OK;
}

int dliom_outlier_remover_filter(dliom_outlier_remover* r, const dliom_cloud* points, dliom_cloud** kept, int32_t* kept_index,
                                 int64_t capacity, int64_t* num_kept) {
  if (r == nullptr || points == nullptr || kept == nullptr || num_kept == nullptr || capacity < 0 || points->n > INT32_MAX)
    return DLIOM_ERR_INVALID_ARGUMENT;
  *kept = nullptr;
  *num_kept = 0;
  dliom_ctx* ctx = r->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  if (points->n == 0) {
    r->phase = 3;
    return empty_cloud(ctx, kept);
  }
  CompactScratch s;
  DLIOM_TRY(flag_by_voxels(r, points, &s));
  unsigned flag = 0;
  DLIOM_TRY(compact_kept(ctx, points, s, r->d_words + kWordFlag, &flag, kept, kept_index, capacity, num_kept));
  if (flag != 0u) return status_of_flag(flag);  // (non-finite: the only one this pass raises)
  r->phase = 3;
  return DLIOM_OK;
}

int dliom_outlier_remover_voxels(const dliom_outlier_remover* r, int32_t* xyz, int32_t* hits, int32_t* rays, int64_t capacity,
                                 int64_t* count) {
  if (r == nullptr || count == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  *count = 0;
  dliom_ctx* ctx = r->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  if (r->leaves == 0) return DLIOM_OK;
  const unsigned long long cells = static_cast<unsigned long long>(r->leaves) * kLeafCells;
  const unsigned blocks = static_cast<unsigned>((cells + kBlock - 1) / kBlock);
  const FillJob fill{r->d_words + kWordCursor, 8, 0u};
  DLIOM_TRY(fill_multi(ctx, &fill, 1));
  hipLaunchKernelGGL(outlier_count_voxels_kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, r->d_pool, cells, r->d_words);
  DLIOM_HIP_TRY(hipGetLastError());
  unsigned host[2];
  DLIOM_TRY(read_words(ctx, r->d_words, kWordCursor, 2, host));
  const int64_t total = words64(host, 0);
  *count = total;
  if (xyz == nullptr && hits == nullptr && rays == nullptr) return DLIOM_OK;  // size query
  if (xyz == nullptr || hits == nullptr || rays == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  if (capacity < total) return DLIOM_ERR_CAPACITY;
  if (total == 0) return DLIOM_OK;
  DLIOM_TRY(ctx->outlier.reserve(static_cast<size_t>(total) * sizeof(VoxelRecord)));
  VoxelRecord* d_records = ctx->outlier.as<VoxelRecord>();
  DLIOM_TRY(fill_multi(ctx, &fill, 1));
  hipLaunchKernelGGL(outlier_emit_voxels_kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, r->d_pool, r->table.slot_key, cells,
                     static_cast<unsigned long long>(total), d_records, r->d_words);
  DLIOM_HIP_TRY(hipGetLastError());
  std::vector<VoxelRecord> records(static_cast<size_t>(total));
  DLIOM_HIP_TRY(hipMemcpyAsync(records.data(), d_records, records.size() * sizeof(VoxelRecord), hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  std::sort(records.begin(), records.end(), [](const VoxelRecord& a, const VoxelRecord& b) { return a.key < b.key; });
  for (int64_t i = 0; i < total; ++i) {
    key_xyz(records[i].key, &xyz[3 * i]);
    hits[i] = records[i].hits;
    rays[i] = records[i].rays;
  }
  return DLIOM_OK;
}

int dliom_outlier_remover_stats(const dliom_outlier_remover* r, dliom_outlier_stats* out) {
  if (r == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  std::memset(out, 0, sizeof *out);
  dliom_ctx* ctx = r->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  unsigned host[kNumWords];
  DLIOM_TRY(read_words(ctx, r->d_words, 0, kNumWords, host));
  out->leaves = r->leaves;
  out->leaf_capacity = r->leaf_capacity;
  out->table_capacity = r->table.capacity;
  out->table_bytes = r->bytes();
  out->growths = r->growths;
  out->samples_walked = words64(host, kWordSamples);
  out->probes = words64(host, kWordProbes);
  out->phase = r->phase;
  int64_t voxels = 0;
  DLIOM_TRY(dliom_outlier_remover_voxels(r, nullptr, nullptr, nullptr, 0, &voxels));
  out->voxels = voxels;
  return DLIOM_OK;
}

int dliom_cloud_min_max_range_filter(dliom_ctx* ctx, const dliom_cloud* in, const float origin[3], double min_range,
                                     double max_range, dliom_cloud** out, int32_t* kept_index, int64_t capacity,
                                     int64_t* num_kept) {
  if (ctx == nullptr || in == nullptr || origin == nullptr || out == nullptr || num_kept == nullptr || capacity < 0 ||
      in->n > INT32_MAX || std::isnan(min_range) || std::isnan(max_range))
    return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  *num_kept = 0;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  if (in->n == 0) return empty_cloud(ctx, out);
  CompactScratch s;
  DLIOM_TRY(flag_by_range(ctx, in, origin, min_range, max_range, &s));
  return compact_kept(ctx, in, s, nullptr, nullptr, out, kept_index, capacity, num_kept);
}

// ---- the same two stages on a batch: compacted in place, attributes gathered on the device (dliom.h, "batches in HBM")
int dliom_outlier_remover_filter_batch(dliom_outlier_remover* r, dliom_points_batch* batch) {
  if (r == nullptr || batch == nullptr || batch->ctx != r->ctx || batch->cloud->n > INT32_MAX) return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_ctx* ctx = r->ctx;
  if (batch->cloud->n == 0) {
    r->phase = 3;
    return DLIOM_OK;
  }
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  CompactScratch s;
  DLIOM_TRY(flag_by_voxels(r, batch->cloud, &s));
  unsigned flag = 0;
  int64_t kept = 0;
  DLIOM_TRY(compact_batch(batch, s, r->d_words + kWordFlag, &flag, &kept));
  if (flag != 0u) return status_of_flag(flag);
  r->phase = 3;
  return DLIOM_OK;
}

int dliom_points_batch_min_max_range_filter(dliom_points_batch* batch, double min_range, double max_range) {
  if (batch == nullptr || batch->cloud->n > INT32_MAX || std::isnan(min_range) || std::isnan(max_range))
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (batch->cloud->n == 0) return DLIOM_OK;
  dliom_ctx* ctx = batch->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  CompactScratch s;
  DLIOM_TRY(flag_by_range(ctx, batch->cloud, batch->origin, min_range, max_range, &s));
  int64_t kept = 0;
  return compact_batch(batch, s, nullptr, nullptr, &kept);
}

}  // extern "C"
