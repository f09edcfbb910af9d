// X-ray images of point clouds on the device: io::XRayPointsProcessor (io/xray_points_processor.{h,cc}, the pipeline
// action "write_xray_image"), equal to the reference bit for bit.
//
// One dliom_points_xray is one Aggregation (.h:68-71): the HybridGridBase<bool> of occupied voxels and the
// std::map<(y, z), ColumnData {float sum_r, sum_g, sum_b; uint32 count}>.  Here both are sparse tables in HBM, in the
// layout of outlier.hip (voxel_hash.h):
//   * "leaf key -> slot" over 8x8x8 blocks of voxels, a leaf being a 512-bit mask (16 words);
//   * "column key (y, z) -> slot" with, per slot, the ColumnData, the number of occupied voxels in the column
//     (what WriteVoxels counts while it iterates the grid, .cc:164-175) and a per-batch counter.
// Voxel bits and the per-column voxel counts are integer atomics and do not depend on any order.  The colour sums are
// float sums in point order (.cc:208-210) and do: a batch's points are grouped by column without changing their order,
// and one lane (a long column: one wavefront) adds a column's colours to the stored sums one after the other.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "voxel_hash.h"

namespace dliom {
namespace {

constexpr int kBlock = 256;
constexpr int kLeafBits = 3;
constexpr int kLeafWords = 16;  // 512 voxels, one bit each
// a column with more points than this in one batch is summed by a wavefront (xray_long_columns_kernel), not by one lane
constexpr unsigned kShortSegment = 64;

// device words of an aggregator
enum {
  kWordLeaves = 0,
  kWordColumns = 1,
  kWordFlag = 2,
  kWordLongest = 3,      // longest run of one column in a batch so far
  kWordVoxels = 4,       // u64
  kWordProbes = 6,       // u64
  kWordLongCount = 8,    // entries of the long-column list of the batch in flight
  kWordMaxOccupied = 9,  // filled by draw
  kWordBoxMin = 10,      // 3 ints, INT_MAX while empty
  kWordBoxMax = 13,      // 3 ints, INT_MIN while empty
  kWordCursor = 16,      // u64
  kNumWords = 20
};

struct ColumnData {  // xray_points_processor.h:61-66
  float sum_r, sum_g, sum_b;
  unsigned count;
};
static_assert(sizeof(ColumnData) == 16, "one 16-byte load and store a column");

struct XrayView {
  uint64_t* leaf_keys;
  unsigned* leaf_slots;
  unsigned leaf_mask;
  unsigned* masks;  // slot * kLeafWords + (cell >> 5), bit cell & 31, cell = (z&7)<<6 | (y&7)<<3 | (x&7)
  uint64_t* col_keys;
  unsigned* col_slots;
  unsigned col_mask;
  float resolution;  // float(voxel_size): HybridGridBase(const float resolution)
  Quat4 q;           // transform_ (Rigid3f)
  float tx, ty, tz;
};

__device__ __forceinline__ uint64_t leaf_key(int cx, int cy, int cz) { return dliom::leaf_key(cx, cy, cz, kLeafBits); }
__device__ __forceinline__ int cell_in_leaf(int cx, int cy, int cz) { return dliom::cell_in_leaf(cx, cy, cz, kLeafBits); }
__host__ __device__ inline uint64_t column_key(int cy, int cz) {  // ascending keys: the std::map's order of (y, z)
  return key_field(cy, kKeyBias, 1) | key_field(cz, kKeyBias, 0);
}

// camera_point = transform_ * batch.points[i] (.cc:199): rotation * p + translation
__device__ __forceinline__ void camera_point(const XrayView& v, float x, float y, float z, float* cx, float* cy, float* cz) {
  float rx, ry, rz;
  rotate_point(v.q, x, y, z, rx, ry, rz);
  *cx = rx + v.tx;
  *cy = ry + v.ty;
  *cz = rz + v.tz;
}

// cells of point i; false where the reference would abort or is undefined (*flag says which)
__device__ __forceinline__ bool cells_of(const XrayView& v, float x, float y, float z, int* cx, int* cy, int* cz, unsigned* flag) {
  float px, py, pz;
  camera_point(v, x, y, z, &px, &py, &pz);
  if (!finite3(px, py, pz)) {
    *flag = kFlagNonFinite;
    return false;
  }
  if (!cell_in_extent(px, v.resolution, cx) || !cell_in_extent(py, v.resolution, cy) || !cell_in_extent(pz, v.resolution, cz)) {
    *flag = kFlagExtent;
    return false;
  }
  return true;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// ---- insert ---------------------------------------------------------------------------------------------------------
// What the reference would abort on (mutable_value -> Grow() -> CHECK_LE(new_bits, 8)) or leaves undefined (lround of a
// non-finite float) is found before anything is written.
__global__ __launch_bounds__(kBlock) void xray_check_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ z, unsigned n, XrayView v,
                                                            unsigned* __restrict__ words) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  unsigned flag = 0;
  int cx, cy, cz;
  if (!cells_of(v, x[i], y[i], z[i], &cx, &cy, &cz, &flag)) atomicOr(&words[kWordFlag], flag);
}

// the leaves and the columns of the batch that the tables do not hold yet (nothing waits: voxel_hash.h)
__global__ __launch_bounds__(kBlock) void xray_claim_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ z, unsigned n, XrayView v,
                                                            uint64_t* __restrict__ leaf_of_slot, uint64_t* __restrict__ col_of_slot,
                                                            unsigned* __restrict__ words) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || words[kWordFlag] != 0u) return;
  unsigned flag = 0;
  int cx, cy, cz;
  if (!cells_of(v, x[i], y[i], z[i], &cx, &cy, &cz, &flag)) return;  // (flagged by the check kernel)
  hash_claim(v.leaf_keys, v.leaf_slots, v.leaf_mask, leaf_key(cx, cy, cz), &words[kWordLeaves], leaf_of_slot);
  hash_claim(v.col_keys, v.col_slots, v.col_mask, column_key(cy, cz), &words[kWordColumns], col_of_slot);
}

// *mutable_value(cell_index) = true; bounding_box_.extend(cell_index) (.cc:202-203); the column slot of every point.
// pending (may be null): ++ per point of a column, for the batches whose points all carry the same colour.
__global__ __launch_bounds__(kBlock) void xray_mark_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ z, unsigned n, XrayView v,
                                                           unsigned* __restrict__ occupied, unsigned* __restrict__ pending,
                                                           unsigned* __restrict__ point_column, unsigned* __restrict__ point_index,
                                                           unsigned columns, unsigned* __restrict__ words) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  unsigned probes = 0;
  bool fresh = false;
  if (i < n) {
    unsigned flag = 0, column = columns;  // `columns`: no column (cannot happen: checked and claimed by the launches before)
    int cx, cy, cz;
    if (cells_of(v, x[i], y[i], z[i], &cx, &cy, &cz, &flag)) {
      const unsigned leaf = hash_find(v.leaf_keys, v.leaf_slots, v.leaf_mask, leaf_key(cx, cy, cz), &probes);
      const unsigned col = hash_find(v.col_keys, v.col_slots, v.col_mask, column_key(cy, cz), &probes);
      if (leaf != kNoSlot && col < columns) {
        column = col;
        const int cell = cell_in_leaf(cx, cy, cz);
        const unsigned bit = 1u << (cell & 31);
        fresh = (atomicOr(&v.masks[static_cast<size_t>(leaf) * kLeafWords + (cell >> 5)], bit) & bit) == 0u;
        if (fresh) atomicAdd(&occupied[col], 1u);
        if (pending != nullptr) atomicAdd(&pending[col], 1u);
        lo[0] = hi[0] = cx;
        lo[1] = hi[1] = cy;
        lo[2] = hi[2] = cz;
      }
    }
    point_column[i] = column;
    if (point_index != nullptr) point_index[i] = i;
  }
  const unsigned long long fresh_lanes = __ballot(fresh);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = wave_min(lo[k]);
    hi[k] = wave_max(hi[k]);
  }
  probes = wave_sum_lane63(probes);
  if ((threadIdx.x & 63u) == 63u) {
    if (lo[0] <= hi[0]) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        atomicMin(reinterpret_cast<int*>(&words[kWordBoxMin + k]), lo[k]);
        atomicMax(reinterpret_cast<int*>(&words[kWordBoxMax + k]), hi[k]);
      }
    }
    if (fresh_lanes != 0ull)
      atomicAdd(reinterpret_cast<unsigned long long*>(&words[kWordVoxels]), static_cast<unsigned long long>(__popcll(fresh_lanes)));
    atomicAdd(reinterpret_cast<unsigned long long*>(&words[kWordProbes]), static_cast<unsigned long long>(probes));
  }
}

__device__ __forceinline__ void note_longest(unsigned* words, unsigned length) {
  if (length > words[kWordLongest]) atomicMax(&words[kWordLongest], length);
}

// A batch without colours (kDefaultColor, .cc:197) or with one colour for all its points: a column's sums after the
// batch depend on how many of its points fell into the column and on nothing else.  The one thread that takes a
// column's counter adds the colour that many times, one addition after the other as the reference does.
__global__ __launch_bounds__(kBlock) void xray_settle_kernel(const unsigned* __restrict__ point_column, unsigned n, unsigned columns,
                                                             unsigned* __restrict__ pending, ColumnData* __restrict__ data, float r,
                                                             float g, float b, int add, unsigned* __restrict__ words) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const unsigned col = point_column[i];
  if (col >= columns) return;
  const unsigned k = atomicExch(&pending[col], 0u);
  if (k == 0u) return;
  ColumnData d = data[col];
  if (add) {  // adding 0.f changes no sum (and no sum is -0: they start at +0)
    for (unsigned j = 0; j < k; ++j) {
      d.sum_r += r;
      d.sum_g += g;
      d.sum_b += b;
    }
  }
  d.count += k;
  data[col] = d;
  note_longest(words, k);
}

// the colours of a batch in the order of the stable sort by column
__global__ __launch_bounds__(kBlock) void xray_gather_colors_kernel(const unsigned* __restrict__ sorted_index,
                                                                    const float* __restrict__ colors_rgb, unsigned n,
                                                                    float4* __restrict__ sorted_rgb) {
  const unsigned j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const size_t i = sorted_index[j];
  sorted_rgb[j] = make_float4(colors_rgb[3 * i], colors_rgb[3 * i + 1], colors_rgb[3 * i + 2], 0.f);
}

// Per-point colours.  sorted_column: the points' column slots, sorted stably, so that a column's points are a run in
// batch order.  The lane at the head of a run walks it; a run longer than kShortSegment goes to the list instead.
__global__ __launch_bounds__(kBlock) void xray_short_columns_kernel(const unsigned* __restrict__ sorted_column,
                                                                    const float4* __restrict__ sorted_rgb, unsigned n,
                                                                    unsigned columns, ColumnData* __restrict__ data,
                                                                    unsigned* __restrict__ long_list, unsigned* __restrict__ words) {
  const unsigned j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const unsigned col = sorted_column[j];
  if (col >= columns || (j > 0u && sorted_column[j - 1u] == col)) return;
  ColumnData d = data[col];
  unsigned k = 0;
  for (; k < kShortSegment; ++k) {
    const unsigned jj = j + k;
    if (jj >= n || sorted_column[jj] != col) break;
    const float4 c = sorted_rgb[jj];
    d.sum_r += c.x;  // column_data.sum_r += color[0] (.cc:208-211)
    d.sum_g += c.y;
    d.sum_b += c.z;
  }
  if (k == kShortSegment && j + kShortSegment < n && sorted_column[j + kShortSegment] == col) {
    long_list[atomicAdd(&words[kWordLongCount], 1u)] = j;  // at most n / (kShortSegment + 1) entries
    return;
  }
  d.count += k;
  data[col] = d;
  note_longest(words, k);
}

// One wavefront per long run: 64 colours are loaded side by side, then every lane adds them in order from lane 0 up
// (v_readlane with a constant lane), so the sum is the sequential one and the loads are coalesced.
__global__ __launch_bounds__(kBlock) void xray_long_columns_kernel(const unsigned* __restrict__ sorted_column,
                                                                   const float4* __restrict__ sorted_rgb, unsigned n,
                                                                   const unsigned* __restrict__ long_list, ColumnData* __restrict__ data,
                                                                   unsigned* __restrict__ words) {
  const unsigned wave = (blockIdx.x * kBlock + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
  if (wave >= words[kWordLongCount]) return;  // the whole wavefront
  const unsigned head = long_list[wave];
  const unsigned col = sorted_column[head];
  ColumnData d = data[col];
  unsigned total = 0;
  for (unsigned base = head;; base += 64u) {
    const unsigned jj = base + lane;
    const bool mine = jj < n && sorted_column[jj] == col;  // a prefix of the lanes: the keys are sorted
    const float4 c = mine ? sorted_rgb[jj] : make_float4(0.f, 0.f, 0.f, 0.f);
    const unsigned count = static_cast<unsigned>(__popcll(__ballot(mine)));
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      if (static_cast<unsigned>(k) < count) {  // uniform
        d.sum_r += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.x), k));
        d.sum_g += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.y), k));
        d.sum_b += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.z), k));
      }
    }
    total += count;
    if (count < 64u) break;
  }
  if (lane == 0u) {
    d.count += total;
    data[col] = d;
    note_longest(words, total);
  }
}

// ---- the tables' contents ---------------------------------------------------------------------------------------------
// every occupied voxel as (z, y, x) biased by 8192, z most significant
__global__ __launch_bounds__(kBlock) void xray_emit_voxels_kernel(const unsigned* __restrict__ masks,
                                                                  const uint64_t* __restrict__ leaf_of_slot, unsigned long long num_words,
                                                                  unsigned long long capacity, uint64_t* __restrict__ out,
                                                                  unsigned* __restrict__ words) {
  const unsigned long long w = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (w >= num_words) return;
  unsigned m = masks[w];
  if (m == 0u) return;
  unsigned long long at = atomicAdd(reinterpret_cast<unsigned long long*>(&words[kWordCursor]), static_cast<unsigned long long>(__popc(m)));
  const uint64_t lk = leaf_of_slot[w / kLeafWords];
  const unsigned first = static_cast<unsigned>(w % kLeafWords) * 32u;
  while (m != 0u) {
    const unsigned cell = first + static_cast<unsigned>(__ffs(static_cast<int>(m)) - 1);
    m &= m - 1u;
    const uint64_t vx = ((lk & kKeyMask) << 3) | (cell & 7u);
    const uint64_t vy = (((lk >> 14) & kKeyMask) << 3) | ((cell >> 3) & 7u);
    const uint64_t vz = (((lk >> 28) & kKeyMask) << 3) | ((cell >> 6) & 7u);
    if (at < capacity) out[at] = (vz << 28) | (vy << 14) | vx;
    ++at;
  }
}

__global__ __launch_bounds__(kBlock) void xray_max_occupied_kernel(const unsigned* __restrict__ occupied, unsigned columns,
                                                                   unsigned* __restrict__ words) {
  const unsigned c = blockIdx.x * kBlock + threadIdx.x;
  const int v = wave_max(c < columns ? static_cast<int>(occupied[c]) : 0);  // <= 16384
  if ((threadIdx.x & 63u) == 0u && v > 0) atomicMax(&words[kWordMaxOccupied], static_cast<unsigned>(v));
}

// ---- painting: IntoImage (.cc:46-84) ----------------------------------------------------------------------------------
__host__ __device__ inline float mix(float a, float b, float t) {  // Mix (.cc:46-48): a * (1. - t) + t * b, t * b in float
  const float tb = t * b;
  return static_cast<float>(static_cast<double>(a) * (1. - static_cast<double>(t)) + static_cast<double>(tb));
}
__host__ __device__ inline uint32_t component_to_uint8(float c) {  // FloatComponentToUint8 (io/color.h:35-38)
  c = c > 1.f ? 1.f : (c < 0.f ? 0.f : c);                         // common::Clamp
  const float scaled = c * 255;
#ifdef __HIP_DEVICE_COMPILE__
  return static_cast<uint32_t>(lround_away(scaled)) & 0xFFu;
#else
  return static_cast<uint32_t>(std::lround(scaled)) & 0xFFu;
#endif
}
// log_n: std::log(num_occupied_cells_in_column) of the host's libm; max: IntoImage's `max`
__host__ __device__ inline uint32_t paint_pixel(double log_n, float max, float mean_r, float mean_g, float mean_b) {
  const float saturation = static_cast<float>(log_n / static_cast<double>(max));
  return 0xFF000000u | (component_to_uint8(mix(1.f, mean_r, saturation)) << 16) |
         (component_to_uint8(mix(1.f, mean_g, saturation)) << 8) | component_to_uint8(mix(1.f, mean_b, saturation));
}
float image_max(uint32_t max_occupied) {  // .cc:53-62; the float of the log is monotone in n
  float max = std::numeric_limits<float>::min();
  if (max_occupied > 0u) max = std::max<float>(max, std::log(static_cast<double>(max_occupied)));
  return max;
}

__global__ __launch_bounds__(kBlock) void xray_fill_white_kernel(uint32_t* __restrict__ argb, unsigned long long pixels) {
  const unsigned long long p = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (p < pixels) argb[p] = 0xFFFFFFFFu;  // image.SetPixel(x, y, {{255, 255, 255}})
}

// WriteVoxels (.cc:151-175) and IntoImage, one column a thread; the caller has checked that every column is inside the box
__global__ __launch_bounds__(kBlock) void xray_paint_kernel(const uint64_t* __restrict__ col_of_slot, const ColumnData* __restrict__ data,
                                                            const unsigned* __restrict__ occupied, unsigned columns, int box_max_y,
                                                            int box_max_z, int width, int height, const double* __restrict__ log_table,
                                                            unsigned table_size, float max, uint32_t* __restrict__ argb) {
  const unsigned c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= columns) return;
  const unsigned n = occupied[c];
  if (n == 0u || n >= table_size) return;
  const uint64_t key = col_of_slot[c];
  const int cy = key_coord(key, 1), cz = key_coord(key, 0);
  const int px = box_max_y - cy, py = box_max_z - cz;  // voxel_index_to_pixel: the y axis flipped
  if (px < 0 || px >= width || py < 0 || py >= height) return;
  const ColumnData d = data[c];
  const float count = static_cast<float>(d.count);  // sum_r / count: float / uint32_t
  argb[static_cast<size_t>(py) * static_cast<size_t>(width) + static_cast<size_t>(px)] =
      paint_pixel(log_table[n], max, d.sum_r / count, d.sum_g / count, d.sum_b / count);
}

inline unsigned blocks_of(int64_t n) { return dliom::blocks_of(n, kBlock); }

}  // namespace
}  // namespace dliom

using namespace dliom;

struct dliom_points_xray {
  dliom_ctx* ctx = nullptr;
  std::shared_ptr<MemoryLedger> ledger;
  float resolution = 0.f;  // HybridGridBase<bool>(voxel_size): float
  Quat4 q{1.f, 0.f, 0.f, 0.f};
  float t[3] = {0.f, 0.f, 0.f};
  KeyTable leaf_table, column_table;
  unsigned* d_masks = nullptr;  // leaf_capacity * kLeafWords
  int64_t leaf_capacity = 0, leaves = 0;
  ColumnData* d_data = nullptr;  // column_capacity each
  unsigned* d_occupied = nullptr;
  unsigned* d_pending = nullptr;  // zero between inserts
  int64_t column_capacity = 0, columns = 0;
  unsigned* d_words = nullptr;
  DevBuf scratch;  // a batch's column slots, their sorted copy and colours; a table dump; the image
  int64_t growths = 0, inserts = 0, points = 0, booked = 0;

  XrayView view() const {
    const HashView l = leaf_table.view(), c = column_table.view();
    return XrayView{l.keys, l.slots, l.mask, d_masks, c.keys, c.slots, c.mask, resolution, q, t[0], t[1], t[2]};
  }
  int64_t bytes() const {
    return leaf_table.bytes() + column_table.bytes() + leaf_capacity * kLeafWords * 4 + column_capacity * (16 + 4 + 4) + kNumWords * 4 +
           static_cast<int64_t>(scratch.cap);
  }
  void book() {
    if (ledger) ledger->points_xray_bytes += bytes() - booked;
    booked = bytes();
  }
  int reserve_scratch(size_t size) {
    const int st = scratch.reserve(size);
    book();
    return st;
  }
  // The pools grow by whole copies of what is allocated (slots past the ones in use are zero), so that growing needs no
  // count of slots in use: `leaves` and `columns` may run ahead of the pools after a growth that failed (pools_ready()).
  int grow_leaves(int64_t want) {
    if (want <= leaf_capacity) return DLIOM_OK;
    const int64_t cap = std::max<int64_t>(want, leaf_capacity + leaf_capacity / 2);
    unsigned* masks = nullptr;
    DLIOM_TRY(grown_copy(ctx, d_masks, leaf_capacity * kLeafWords, cap * kLeafWords, &masks));
    if (d_masks) (void)hipFree(d_masks);
    d_masks = masks;
    if (leaf_capacity > 0) ++growths;
    leaf_capacity = cap;
    book();
    return DLIOM_OK;
  }
  int grow_columns(int64_t want) {
    if (want <= column_capacity) return DLIOM_OK;
    const int64_t cap = std::max<int64_t>(want, column_capacity + column_capacity / 2);
    // three new arrays first, the old ones freed after all three exist: a failure leaves the pools as they were
    ColumnData* data = nullptr;
    unsigned *occ = nullptr, *pend = nullptr;
    int st = grown_copy(ctx, d_data, column_capacity, cap, &data);
    if (st == DLIOM_OK) st = grown_copy(ctx, d_occupied, column_capacity, cap, &occ);
    if (st == DLIOM_OK) st = grown_copy(ctx, d_pending, 0, cap, &pend);  // zero between inserts
    if (st != DLIOM_OK) {
      if (data) (void)hipFree(data);
      if (occ) (void)hipFree(occ);
      return st;
    }
    if (d_data) (void)hipFree(d_data);
    if (d_occupied) (void)hipFree(d_occupied);
    if (d_pending) (void)hipFree(d_pending);
    d_data = data;
    d_occupied = occ;
    d_pending = pend;
    if (column_capacity > 0) ++growths;
    column_capacity = cap;
    book();
    return DLIOM_OK;
  }
  // Every slot the tables name has its place in the pools.  Always so, except after an insert whose pool growth failed
  // (out of memory): its keys are in the tables -- the counts were taken over, so a later rehash keeps them -- but its
  // points were not inserted.  The next call that needs the pools grows them here, or fails in the same way.
  int pools_ready() {
    DLIOM_TRY(grow_leaves(leaves));
    return grow_columns(columns);
  }
};

extern "C" {

int dliom_points_xray_create(dliom_ctx* ctx, double voxel_size, const float transform7[7], dliom_points_xray** out) {
  if (ctx == nullptr || out == nullptr || transform7 == nullptr || !(voxel_size > 0.0) || !std::isfinite(voxel_size) ||
      !(static_cast<float>(voxel_size) > 0.f) || !std::isfinite(static_cast<float>(voxel_size)))
    return DLIOM_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(transform7[k])) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  dliom_points_xray* x = new dliom_points_xray;
  x->ctx = ctx;
  x->ledger = ctx->ledger;
  x->resolution = static_cast<float>(voxel_size);
  x->t[0] = transform7[0];
  x->t[1] = transform7[1];
  x->t[2] = transform7[2];
  x->q = Quat4{transform7[3], transform7[4], transform7[5], transform7[6]};
  unsigned init[kNumWords] = {};
  for (int k = 0; k < 3; ++k) {
    init[kWordBoxMin + k] = static_cast<unsigned>(INT_MAX);
    init[kWordBoxMax + k] = static_cast<unsigned>(INT_MIN);
  }
  int st = hipMalloc(&x->d_words, kNumWords * 4) == hipSuccess ? DLIOM_OK : DLIOM_ERR_HIP;
  if (st == DLIOM_OK && (hipMemcpyAsync(x->d_words, init, sizeof init, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                         hipStreamSynchronize(ctx->stream) != hipSuccess))
    st = DLIOM_ERR_HIP;
  if (st == DLIOM_OK) st = x->leaf_table.grow(ctx, 512, 0, &x->growths);
  if (st == DLIOM_OK) st = x->column_table.grow(ctx, 512, 0, &x->growths);
  if (st == DLIOM_OK) st = x->grow_leaves(512);
  if (st == DLIOM_OK) st = x->grow_columns(512);
  if (st != DLIOM_OK) {
    dliom_points_xray_destroy(x);
    return st;
  }
  x->book();
  *out = x;
  return DLIOM_OK;
}

int dliom_points_xray_destroy(dliom_points_xray* x) {
  if (x == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  (void)hipSetDevice(x->ctx->device);
  (void)hipStreamSynchronize(x->ctx->stream);
  x->leaf_table.release();
  x->column_table.release();
  if (x->d_masks) (void)hipFree(x->d_masks);
  if (x->d_data) (void)hipFree(x->d_data);
  if (x->d_occupied) (void)hipFree(x->d_occupied);
  if (x->d_pending) (void)hipFree(x->d_pending);
  if (x->d_words) (void)hipFree(x->d_words);
  x->scratch.release();
  if (x->ledger) x->ledger->points_xray_bytes -= x->booked;
  delete x;
  return DLIOM_OK;
}

}  // extern "C"

// Insert with the colours where they are.  num_colors 0 or 1: `rgb` is the batch's colour (host, 3 floats; unread for 0).
// One a point: d_colors (device, r g b a point) is read in place; when it is null, h_colors (host) is uploaded first.
static int xray_insert(dliom_points_xray* x, const dliom_cloud* points, int64_t num_colors, const float* rgb, const float* d_colors,
                       const float* h_colors) {
  if (points->n == 0) return DLIOM_OK;
  dliom_ctx* ctx = x->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const unsigned n = static_cast<unsigned>(points->n);
  const bool per_point = num_colors == points->n && points->n > 1;
  // every point in a leaf and a column of its own: the bound the call knows
  DLIOM_TRY(x->leaf_table.grow(ctx, x->leaves + points->n, x->leaves, &x->growths));
  DLIOM_TRY(x->column_table.grow(ctx, x->columns + points->n, x->columns, &x->growths));
  x->book();
  DLIOM_TRY(x->pools_ready());
  const FillJob fills[2] = {{x->d_words + kWordFlag, 4, 0u}, {x->d_words + kWordLongCount, 4, 0u}};
  DLIOM_TRY(fill_multi(ctx, fills, 2));
  hipLaunchKernelGGL(xray_check_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, points->d_x, points->d_y, points->d_z, n,
                     x->view(), x->d_words);
  hipLaunchKernelGGL(xray_claim_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, points->d_x, points->d_y, points->d_z, n,
                     x->view(), x->leaf_table.slot_key, x->column_table.slot_key, x->d_words);
  DLIOM_HIP_TRY(hipGetLastError());
  unsigned host[3];
  DLIOM_TRY(read_words(x->ctx, x->d_words, 0, 3, host));  // leaves, columns, flag
  if (host[kWordFlag] != 0u) return status_of_flag(host[kWordFlag]);  // nothing was claimed or written
  // The keys are in the tables now: the counts are taken over first, so that a rehash always moves every key, and the
  // pools grow to them.  Should that fail, nothing of the batch is inserted: its new columns stay at count 0, which
  // dliom_points_xray_columns skips, and its new leaves empty.
  x->leaves = host[kWordLeaves];
  x->columns = host[kWordColumns];
  DLIOM_TRY(x->pools_ready());
  const int64_t columns = x->columns;

  // scratch: point_column | point_index | sorted_column | sorted_index | long_list | sorted_rgb | colours | sort storage
  const size_t per = align256(4 * static_cast<size_t>(n));
  size_t sort_bytes = 0;
  int end_bit = 1;
  while ((int64_t{1} << end_bit) <= columns) ++end_bit;  // the keys are <= columns
  if (per_point)
    DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, static_cast<const unsigned*>(nullptr),
                                                     static_cast<unsigned*>(nullptr), static_cast<const unsigned*>(nullptr),
                                                     static_cast<unsigned*>(nullptr), static_cast<int>(n), 0, end_bit, ctx->stream));
  DLIOM_TRY(x->reserve_scratch(per_point ? 5 * per + align256(16 * static_cast<size_t>(n)) + align256(12 * static_cast<size_t>(n)) +
                                               align256(sort_bytes)
                                         : per));
  char* b = static_cast<char*>(x->scratch.p);
  unsigned* point_column = reinterpret_cast<unsigned*>(b);
  unsigned* point_index = reinterpret_cast<unsigned*>(b + per);
  unsigned* sorted_column = reinterpret_cast<unsigned*>(b + 2 * per);
  unsigned* sorted_index = reinterpret_cast<unsigned*>(b + 3 * per);
  unsigned* long_list = reinterpret_cast<unsigned*>(b + 4 * per);
  float4* sorted_rgb = reinterpret_cast<float4*>(b + 5 * per);
  float* colors = reinterpret_cast<float*>(b + 5 * per + align256(16 * static_cast<size_t>(n)));
  void* sort_tmp = b + 5 * per + align256(16 * static_cast<size_t>(n)) + align256(12 * static_cast<size_t>(n));

  if (per_point && d_colors == nullptr) {
    // The caller's buffer is free when the call returns, page-locked or not; everything before the copy has finished.
    DLIOM_HIP_TRY(hipMemcpyAsync(colors, h_colors, 12 * static_cast<size_t>(n), hipMemcpyHostToDevice, ctx->stream));
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    ++ctx->host_syncs;
    d_colors = colors;
  }
  hipLaunchKernelGGL(xray_mark_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, points->d_x, points->d_y, points->d_z, n,
                     x->view(), x->d_occupied, per_point ? nullptr : x->d_pending, point_column, per_point ? point_index : nullptr,
                     static_cast<unsigned>(columns), x->d_words);
  if (!per_point) {
    const float r = num_colors == 1 ? rgb[0] : 0.f, g = num_colors == 1 ? rgb[1] : 0.f, bl = num_colors == 1 ? rgb[2] : 0.f;
    hipLaunchKernelGGL(xray_settle_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, point_column, n,
                       static_cast<unsigned>(columns), x->d_pending, x->d_data, r, g, bl, num_colors == 1 ? 1 : 0, x->d_words);
  } else {
    DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(sort_tmp, sort_bytes, point_column, sorted_column, point_index, sorted_index,
                                                     static_cast<int>(n), 0, end_bit, ctx->stream));
    hipLaunchKernelGGL(xray_gather_colors_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, sorted_index, d_colors, n, sorted_rgb);
    hipLaunchKernelGGL(xray_short_columns_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, sorted_column, sorted_rgb, n,
                       static_cast<unsigned>(columns), x->d_data, long_list, x->d_words);
    // a wavefront per list entry; the list has at most n / (kShortSegment + 1) of them
    const int64_t max_long = n / (kShortSegment + 1u);
    if (max_long > 0)
      hipLaunchKernelGGL(xray_long_columns_kernel, dim3(blocks_of(max_long * 64)), dim3(kBlock), 0, ctx->stream, sorted_column,
                         sorted_rgb, n, long_list, x->d_data, x->d_words);
  }
  DLIOM_HIP_TRY(hipGetLastError());
  ++x->inserts;
  x->points += points->n;
  return DLIOM_OK;
}

extern "C" {

int dliom_points_xray_insert(dliom_points_xray* x, const dliom_cloud* points, const float* colors_rgb, int64_t num_colors) {
  if (x == nullptr || points == nullptr || points->n > INT32_MAX) return DLIOM_ERR_INVALID_ARGUMENT;
  if (num_colors != 0 && num_colors != 1 && num_colors != points->n) return DLIOM_ERR_INVALID_ARGUMENT;
  if (num_colors != 0 && colors_rgb == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  return xray_insert(x, points, num_colors, colors_rgb, nullptr, colors_rgb);
}

int dliom_points_xray_insert_batch(dliom_points_xray* x, const dliom_points_batch* batch) {
  if (x == nullptr || batch == nullptr || batch->ctx != x->ctx || batch->cloud->n > INT32_MAX) return DLIOM_ERR_INVALID_ARGUMENT;
  const dliom_cloud* points = batch->cloud;
  if (!batch->has_colors()) return xray_insert(x, points, 0, nullptr, nullptr, nullptr);
  if (batch->single_color) return xray_insert(x, points, 1, batch->rgb, nullptr, nullptr);
  if (points->n == 1) {  // one point, one colour: the single-colour path reads it from the host, as the host entry does
    float rgb[3];
    DLIOM_HIP_TRY(hipSetDevice(x->ctx->device));
    DLIOM_HIP_TRY(hipMemcpyAsync(rgb, batch->colors.p, 12, hipMemcpyDeviceToHost, x->ctx->stream));
    DLIOM_HIP_TRY(hipStreamSynchronize(x->ctx->stream));
    ++x->ctx->host_syncs;
    return xray_insert(x, points, 1, rgb, nullptr, nullptr);
  }
  return xray_insert(x, points, points->n, nullptr, batch->colors.p, nullptr);
}

int dliom_points_xray_bounding_box(const dliom_points_xray* x, int32_t box_min[3], int32_t box_max[3], int* empty) {
  if (x == nullptr || box_min == nullptr || box_max == nullptr || empty == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(x->ctx->device));
  unsigned host[6];
  DLIOM_TRY(read_words(x->ctx, x->d_words, kWordBoxMin, 6, host));
  for (int k = 0; k < 3; ++k) {
    box_min[k] = static_cast<int32_t>(host[k]);
    box_max[k] = static_cast<int32_t>(host[3 + k]);
  }
  *empty = box_min[0] > box_max[0] ? 1 : 0;  // Eigen::AlignedBox3i::isEmpty
  return DLIOM_OK;
}

int dliom_points_xray_columns(const dliom_points_xray* cx, int32_t* yz, float* sums_rgb, uint32_t* counts, uint32_t* occupied,
                              int64_t capacity, int64_t* count) {
  if (cx == nullptr || count == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  *count = 0;
  const bool size_only = yz == nullptr && sums_rgb == nullptr && counts == nullptr && occupied == nullptr;
  if (!size_only && (yz == nullptr || sums_rgb == nullptr || counts == nullptr || occupied == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_points_xray* x = const_cast<dliom_points_xray*>(cx);  // (pools_ready)
  if (x->columns == 0) return DLIOM_OK;
  dliom_ctx* ctx = x->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(x->pools_ready());
  const size_t n = static_cast<size_t>(x->columns);
  std::vector<uint64_t> keys(n);
  std::vector<ColumnData> data(n);
  std::vector<unsigned> occ(n);
  DLIOM_HIP_TRY(hipMemcpyAsync(data.data(), x->d_data, n * sizeof(ColumnData), hipMemcpyDeviceToHost, ctx->stream));
  if (!size_only) {
    DLIOM_HIP_TRY(hipMemcpyAsync(keys.data(), x->column_table.slot_key, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipMemcpyAsync(occ.data(), x->d_occupied, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  // a slot without points is no entry of column_data: the key of an insert that failed while the pools grew
  std::vector<unsigned> order;
  for (size_t s = 0; s < n; ++s)
    if (data[s].count > 0u) order.push_back(static_cast<unsigned>(s));
  *count = static_cast<int64_t>(order.size());
  if (size_only) return DLIOM_OK;
  if (capacity < *count) return DLIOM_ERR_CAPACITY;
  std::sort(order.begin(), order.end(), [&](unsigned a, unsigned b) { return keys[a] < keys[b]; });
  for (size_t i = 0; i < order.size(); ++i) {
    const unsigned s = order[i];
    yz[2 * i] = key_coord(keys[s], 1);
    yz[2 * i + 1] = key_coord(keys[s], 0);
    sums_rgb[3 * i] = data[s].sum_r;
    sums_rgb[3 * i + 1] = data[s].sum_g;
    sums_rgb[3 * i + 2] = data[s].sum_b;
    counts[i] = data[s].count;
    occupied[i] = occ[s];
  }
  return DLIOM_OK;
}

int dliom_points_xray_voxels(const dliom_points_xray* cx, int32_t* xyz, int64_t capacity, int64_t* count) {
  if (cx == nullptr || count == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_points_xray* x = const_cast<dliom_points_xray*>(cx);  // the scratch buffer is a cache
  *count = 0;
  dliom_ctx* ctx = x->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  unsigned host[2];
  DLIOM_TRY(read_words(x->ctx, x->d_words, kWordVoxels, 2, host));
  const int64_t total = words64(host, 0);
  *count = total;
  if (xyz == nullptr) return DLIOM_OK;  // size query
  if (capacity < total) return DLIOM_ERR_CAPACITY;
  if (total == 0) return DLIOM_OK;
  DLIOM_TRY(x->pools_ready());
  DLIOM_TRY(x->reserve_scratch(static_cast<size_t>(total) * 8));
  uint64_t* d_out = x->scratch.as<uint64_t>();
  const FillJob fill{x->d_words + kWordCursor, 8, 0u};
  DLIOM_TRY(fill_multi(ctx, &fill, 1));
  const unsigned long long num_words = static_cast<unsigned long long>(x->leaves) * kLeafWords;
  hipLaunchKernelGGL(xray_emit_voxels_kernel, dim3(static_cast<unsigned>((num_words + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     ctx->stream, x->d_masks, x->leaf_table.slot_key, num_words, static_cast<unsigned long long>(total), d_out,
                     x->d_words);
  DLIOM_HIP_TRY(hipGetLastError());
  std::vector<uint64_t> keys(static_cast<size_t>(total));
  DLIOM_HIP_TRY(hipMemcpyAsync(keys.data(), d_out, keys.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  std::sort(keys.begin(), keys.end());
  for (int64_t i = 0; i < total; ++i) key_xyz(keys[static_cast<size_t>(i)], &xyz[3 * i]);
  return DLIOM_OK;
}

int dliom_points_xray_draw(const dliom_points_xray* cx, const int32_t box_min[3], const int32_t box_max[3], uint32_t* argb,
                           int64_t capacity, int32_t* width, int32_t* height) {
  if (cx == nullptr || width == nullptr || height == nullptr || capacity < 0 || (box_min == nullptr) != (box_max == nullptr))
    return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_points_xray* x = const_cast<dliom_points_xray*>(cx);
  *width = *height = 0;
  dliom_ctx* ctx = x->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(x->pools_ready());
  const FillJob fill{x->d_words + kWordMaxOccupied, 4, 0u};
  DLIOM_TRY(fill_multi(ctx, &fill, 1));
  if (x->columns > 0) {
    hipLaunchKernelGGL(xray_max_occupied_kernel, dim3(blocks_of(x->columns)), dim3(kBlock), 0, ctx->stream, x->d_occupied,
                       static_cast<unsigned>(x->columns), x->d_words);
    DLIOM_HIP_TRY(hipGetLastError());
  }
  unsigned host[7];
  DLIOM_TRY(read_words(x->ctx, x->d_words, kWordMaxOccupied, 7, host));
  const uint32_t max_occupied = host[0];
  int own_min[3], own_max[3], lo[3], hi[3];
  for (int k = 0; k < 3; ++k) {
    own_min[k] = static_cast<int>(host[1 + k]);
    own_max[k] = static_cast<int>(host[4 + k]);
    lo[k] = box_min != nullptr ? box_min[k] : own_min[k];
    hi[k] = box_max != nullptr ? box_max[k] : own_max[k];
  }
  const bool own_empty = own_min[0] > own_max[0];
  if (lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) {  // bounding_box_.isEmpty(): "Not writing output" (.cc:146-149)
    return own_empty ? DLIOM_OK : DLIOM_ERR_INVALID_ARGUMENT;
  }
  for (int k = 0; k < 3; ++k) {
    if (lo[k] < kMinIndex || hi[k] > kMaxIndex) return DLIOM_ERR_INVALID_ARGUMENT;
    // a voxel outside the box would be a pixel outside the reference's matrix
    if (!own_empty && (own_min[k] < lo[k] || own_max[k] > hi[k])) return DLIOM_ERR_INVALID_ARGUMENT;
  }
  const int w = hi[1] - lo[1] + 1, h = hi[2] - lo[2] + 1;  // bounding_box_.sizes()[1] + 1, [2] + 1 (.cc:161-162)
  *width = w;
  *height = h;
  const int64_t pixels = static_cast<int64_t>(w) * h;
  if (argb == nullptr) return DLIOM_OK;  // sizes only
  if (capacity < pixels) return DLIOM_ERR_CAPACITY;
  // std::log of the host's libm for every count an image can hold (the device's log is not pinned to it)
  std::vector<double> log_table(static_cast<size_t>(max_occupied) + 1, 0.0);
  for (uint32_t n = 1; n <= max_occupied; ++n) log_table[n] = std::log(static_cast<double>(n));
  const size_t image_bytes = align256(static_cast<size_t>(pixels) * 4);
  DLIOM_TRY(x->reserve_scratch(image_bytes + log_table.size() * 8));
  uint32_t* d_argb = x->scratch.as<uint32_t>();
  double* d_log = reinterpret_cast<double*>(static_cast<char*>(x->scratch.p) + image_bytes);
  DLIOM_HIP_TRY(hipMemcpyAsync(d_log, log_table.data(), log_table.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(xray_fill_white_kernel, dim3(static_cast<unsigned>((pixels + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                     d_argb, static_cast<unsigned long long>(pixels));
  if (x->columns > 0)
    hipLaunchKernelGGL(xray_paint_kernel, dim3(blocks_of(x->columns)), dim3(kBlock), 0, ctx->stream, x->column_table.slot_key,
                       x->d_data, x->d_occupied, static_cast<unsigned>(x->columns), hi[1], hi[2], w, h, d_log,
                       static_cast<unsigned>(log_table.size()), image_max(max_occupied), d_argb);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipMemcpyAsync(argb, d_argb, static_cast<size_t>(pixels) * 4, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  return DLIOM_OK;
}

int dliom_points_xray_stats(const dliom_points_xray* x, dliom_points_xray_statistics* out) {
  if (x == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  std::memset(out, 0, sizeof *out);
  DLIOM_HIP_TRY(hipSetDevice(x->ctx->device));
  unsigned host[kNumWords];
  DLIOM_TRY(read_words(x->ctx, x->d_words, 0, kNumWords, host));
  out->voxels = words64(host, kWordVoxels);
  out->columns = x->columns;
  out->leaves = x->leaves;
  out->table_bytes = x->bytes();
  out->probes = words64(host, kWordProbes);
  out->longest_segment = host[kWordLongest];
  out->growths = x->growths;
  out->inserts = x->inserts;
  out->points = x->points;
  return DLIOM_OK;
}

int dliom_points_xray_pixel(uint32_t occupied, uint32_t max_occupied, const float mean_rgb[3], uint32_t* argb) {
  if (mean_rgb == nullptr || argb == nullptr || occupied > max_occupied) return DLIOM_ERR_INVALID_ARGUMENT;
  *argb = occupied == 0u ? 0xFFFFFFFFu
                         : paint_pixel(std::log(static_cast<double>(occupied)), image_max(max_occupied), mean_rgb[0], mean_rgb[1],
                                       mean_rgb[2]);
  return DLIOM_OK;
}

}  // extern "C"
