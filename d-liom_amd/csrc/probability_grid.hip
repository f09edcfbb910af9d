// The 2D probability grid of the export pipeline on the device: io::ProbabilityGridPointsProcessor
// (io/probability_grid_points_processor.{h,cc}, action "write_probability_grid") and
// cartographer_ros::RosMapWritingPointsProcessor (ros_map_writing_points_processor.cc, "write_ros_map"), equal to the
// reference bit for bit.
//
// mapping::ProbabilityGrid is a dense array of uint16 correspondence-cost values, row-major num_x_cells * y + x
// (grid_2d.cc:168-171); here it lives in HBM, MapLimits and the known-cells box on the host.  One Insert
// (probability_grid_range_data_inserter_2d.cc:48-64 -> CastRays, ray_casting.cc:166-203) is
//   bounds pass   float min / max of the points (GrowAsNeeded, :148-162) and the non-finite flag; read back
//   (host)        GrowLimits on the limits alone (grid_2d.cc:116-145); one device copy into a larger array if it grew
//   hits pass     superscaled end of every point (map_limits.h:69-76 in double), hit table on its pixel
//   ray pass      one CastRay(begin, end) a thread (ray_casting.cc:29-146), miss table          <- the hot path
//   clear pass    FinishUpdate (grid_2d.cc:76-83) over the batch's pixel box; the error words are read back
// Within one Insert a cell ends as hit_table[v] if an end pixel falls in it, else miss_table[v] if a ray visits it,
// else v: ApplyLookupTable (probability_grid.cc:52-64) skips cells that carry the update marker, so the order of the
// visits cannot show.  Hence plain 16-bit loads and stores, like grid.hip's insertion: every racing writer of a pass
// stores the same value, computed from the same old value, and the passes are separate launches.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "device_common.h"
#include "probability_values.h"
#include "voxel_hash.h"  // read_words, words64

namespace dliom {
namespace {

constexpr int kBlock = 256;
constexpr int kSubpixelScale = 1000;  // ray_casting.cc:24
constexpr unsigned kUpdateMarker = 32768u;
constexpr unsigned kFlagNonFinite = 1u, kFlagExtent = 2u;
constexpr unsigned kErrVisitOutside = 1u, kErrEndOfRay = 2u;

// device words of a grid; the minima are kept as the maxima of the inverted keys, so that one 16-byte fill resets all four
enum { kWordFlag = 0, kWordError = 1, kWordVisits = 2 /* u64 */, kWordNotMinX = 4, kWordNotMinY = 5, kWordMaxX = 6, kWordMaxY = 7, kNumWords = 8 };

struct Cells {
  uint16_t* cells;
  int nx, ny;
};

// MapLimits of the superscaled grid (ray_casting.cc:174-178): resolution / 1000 computed once, in double
struct SuperLimits {
  double resolution, max_x, max_y;
  int nx, ny;  // num cells * 1000
};

// order-preserving map of finite floats to unsigned (-0 below +0)
__host__ __device__ inline unsigned float_key(float f) {
#ifdef __HIP_DEVICE_COMPILE__
  const unsigned u = __float_as_uint(f);
#else
  unsigned u;
  std::memcpy(&u, &f, 4);
#endif
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float key_float(unsigned k) {
  const unsigned u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

__device__ __forceinline__ bool finite1(float v) { return fabsf(v) <= 3.4028234e38f; }  // false for NaN

// GrowAsNeeded's bounding box of the returns (ray_casting.cc:150-154): min and max do not depend on the order for finite
// input (-0 and +0 differ only until the padding is added)
__global__ __launch_bounds__(kBlock) void pg_bounds_kernel(const float* __restrict__ x, const float* __restrict__ y, unsigned n,
                                                           unsigned* __restrict__ words) {
  unsigned lo_x = 0xFFFFFFFFu, lo_y = 0xFFFFFFFFu, hi_x = 0u, hi_y = 0u, bad = 0u;
  for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const float px = x[i], py = y[i];
    if (!finite1(px) || !finite1(py)) {
      bad = kFlagNonFinite;
      continue;
    }
    const unsigned kx = float_key(px), ky = float_key(py);
    lo_x = min(lo_x, kx);
    hi_x = max(hi_x, kx);
    lo_y = min(lo_y, ky);
    hi_y = max(hi_y, ky);
  }
  for (int m = 32; m >= 1; m >>= 1) {
    lo_x = min(lo_x, static_cast<unsigned>(__shfl_xor(static_cast<int>(lo_x), m)));
    lo_y = min(lo_y, static_cast<unsigned>(__shfl_xor(static_cast<int>(lo_y), m)));
    hi_x = max(hi_x, static_cast<unsigned>(__shfl_xor(static_cast<int>(hi_x), m)));
    hi_y = max(hi_y, static_cast<unsigned>(__shfl_xor(static_cast<int>(hi_y), m)));
    bad |= static_cast<unsigned>(__shfl_xor(static_cast<int>(bad), m));
  }
  if ((threadIdx.x & 63u) == 0u) {
    atomicMax(&words[kWordNotMinX], ~lo_x);
    atomicMax(&words[kWordNotMinY], ~lo_y);
    atomicMax(&words[kWordMaxX], hi_x);
    atomicMax(&words[kWordMaxY], hi_y);
    if (bad != 0u) atomicOr(&words[kWordFlag], bad);
  }
}

// common::RoundToInt(double) = std::lround, narrowed to int (map_limits.h:73-75), for |q| < 2^31; false beyond
__host__ __device__ inline bool round_index(double q, int* out) {
  if (!(fabs(q) < 2147483000.0)) return false;
  const double t = trunc(q);
  const double d = q - t;  // exact
  int k = static_cast<int>(t);
  k += (d >= 0.5) ? 1 : 0;
  k -= (d <= -0.5) ? 1 : 0;
  *out = k;
  return true;
}

// MapLimits::GetCellIndex (map_limits.h:69-76): x from max.y - p.y, y from max.x - p.x
__host__ __device__ inline bool cell_index(double resolution, double max_x, double max_y, float px, float py, int* cx, int* cy) {
  const bool a = round_index((max_y - static_cast<double>(py)) / resolution - 0.5, cx);
  const bool b = round_index((max_x - static_cast<double>(px)) / resolution - 0.5, cy);
  return a && b;
}

__device__ __forceinline__ void apply_table(const Cells& g, int x, int y, const uint16_t* __restrict__ table, unsigned* err) {
  if (static_cast<unsigned>(x) >= static_cast<unsigned>(g.nx) || static_cast<unsigned>(y) >= static_cast<unsigned>(g.ny)) {
    *err |= kErrVisitOutside;  // CHECK(limits_.Contains(cell_index)) grid_2d.cc:169
    return;
  }
  uint16_t* cell = g.cells + (static_cast<size_t>(g.nx) * static_cast<size_t>(y) + static_cast<size_t>(x));
  const unsigned v = *cell;
  if (v < kUpdateMarker) *cell = table[v];  // probability_grid.cc:57-61
}

// ends.push_back(superscaled_limits.GetCellIndex(hit)) (ray_casting.cc:184-185).  A superscaled index outside the grid is
// what the reference aborts on (CHECK_GE :38-40, CHECK(Contains) grid_2d.cc:169): flagged here, in a launch of its own,
// so that no later pass writes anything.
__global__ __launch_bounds__(kBlock) void pg_ends_kernel(const float* __restrict__ x, const float* __restrict__ y, unsigned n,
                                                         SuperLimits s, int2* __restrict__ ends, unsigned* __restrict__ words) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int ex = -1, ey = -1;
  const bool ok = cell_index(s.resolution, s.max_x, s.max_y, x[i], y[i], &ex, &ey) && ex >= 0 && ey >= 0 && ex < s.nx && ey < s.ny;
  ends[i] = make_int2(ex, ey);
  if (!ok) atomicOr(&words[kWordFlag], kFlagExtent);
}

__global__ __launch_bounds__(kBlock) void pg_apply_hits_kernel(const int2* __restrict__ ends, unsigned n, Cells g,
                                                               const uint16_t* __restrict__ hit_table, unsigned* __restrict__ words) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || words[kWordFlag] != 0u) return;
  const int2 e = ends[i];
  unsigned err = 0;
  apply_table(g, e.x / kSubpixelScale, e.y / kSubpixelScale, hit_table, &err);
  if (err != 0u) atomicOr(&words[kWordError], err);
}

// CastRay(begin, end) (ray_casting.cc:29-146), one ray a thread, the reference's recurrence and order of visits.
__global__ __launch_bounds__(kBlock) void pg_cast_rays_kernel(const int2* __restrict__ ends, unsigned n, int origin_x, int origin_y,
                                                              Cells g, const uint16_t* __restrict__ miss_table,
                                                              unsigned* __restrict__ words) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  unsigned visits = 0, err = 0;
  if (i < n && words[kWordFlag] == 0u) {
    constexpr int S = kSubpixelScale;
    int bx = origin_x, by = origin_y;
    const int2 e = ends[i];
    int ex = e.x, ey = e.y;
    if (bx > ex) {  // :33-36
      const int tx = bx, ty = by;
      bx = ex;
      by = ey;
      ex = tx;
      ey = ty;
    }
    if (bx / S == ex / S) {  // :44-52 a vertical line in full pixels
      const int cx = bx / S;
      const int end_y = max(by, ey) / S;
      for (int cy = min(by, ey) / S; cy <= end_y; ++cy) {
        apply_table(g, cx, cy, miss_table, &err);
        ++visits;
      }
    } else {
      const long long dx = ex - bx;
      const long long dy = ey - by;
      const long long denominator = 2ll * S * dx;
      int cx = bx / S, cy = by / S;
      long long sub_y = (2ll * (by % S) + 1) * dx;
      const int first_pixel = 2 * S - 2 * (bx % S) - 1;
      const int last_pixel = 2 * (ex % S) + 1;
      const int end_x = ex / S;  // max(begin.x, end.x) / S after the swap
      sub_y += dy * first_pixel;
      if (dy > 0) {
        for (;;) {
          apply_table(g, cx, cy, miss_table, &err);
          ++visits;
          while (sub_y > denominator) {
            sub_y -= denominator;
            ++cy;
            apply_table(g, cx, cy, miss_table, &err);
            ++visits;
          }
          ++cx;
          if (sub_y == denominator) {
            sub_y -= denominator;
            ++cy;
          }
          if (cx == end_x) break;
          sub_y += dy * 2 * S;
        }
        sub_y += dy * last_pixel;
        apply_table(g, cx, cy, miss_table, &err);
        ++visits;
        while (sub_y > denominator) {
          sub_y -= denominator;
          ++cy;
          apply_table(g, cx, cy, miss_table, &err);
          ++visits;
        }
        if (sub_y == denominator || cy != ey / S) err |= kErrEndOfRay;  // CHECK_NE, CHECK_EQ :114-115
      } else {
        for (;;) {
          apply_table(g, cx, cy, miss_table, &err);
          ++visits;
          while (sub_y < 0) {
            sub_y += denominator;
            --cy;
            apply_table(g, cx, cy, miss_table, &err);
            ++visits;
          }
          ++cx;
          if (sub_y == 0) {
            sub_y += denominator;
            --cy;
          }
          if (cx == end_x) break;
          sub_y += dy * 2 * S;
        }
        sub_y += dy * last_pixel;
        apply_table(g, cx, cy, miss_table, &err);
        ++visits;
        while (sub_y < 0) {
          sub_y += denominator;
          --cy;
          apply_table(g, cx, cy, miss_table, &err);
          ++visits;
        }
        if (sub_y == 0 || cy != ey / S) err |= kErrEndOfRay;  // :144-145
      }
    }
  }
  if (err != 0u) atomicOr(&words[kWordError], err);
  visits = wave_sum_lane63(visits);  // < 2^25 a ray (23170 + 23170 pixels at the largest grid): no overflow in a wave
  if ((threadIdx.x & 63u) == 63u && visits != 0u)
    atomicAdd(reinterpret_cast<unsigned long long*>(&words[kWordVisits]), static_cast<unsigned long long>(visits));
}

// FinishUpdate (grid_2d.cc:76-83) over the pixel box [x0, x0 + w) x [y0, y0 + h) of the batch: outside an Insert no cell
// carries the marker, and a supercover line stays inside the pixel box of its two ends
__global__ __launch_bounds__(kBlock) void pg_clear_marker_kernel(Cells g, int x0, int y0, int w, int h) {
  const int x = blockIdx.x * kBlock + threadIdx.x;
  if (x >= w) return;
  for (int y = blockIdx.y; y < h; y += gridDim.y) {
    uint16_t* cell = g.cells + (static_cast<size_t>(g.nx) * static_cast<size_t>(y0 + y) + static_cast<size_t>(x0 + x));
    const unsigned v = *cell;
    if (v >= kUpdateMarker) *cell = static_cast<uint16_t>(v - kUpdateMarker);
  }
}

// GrowLimits' copy (grid_2d.cc:127-139): the old cells at x_offset + stride * y_offset of the new array (already zero)
__global__ __launch_bounds__(kBlock) void pg_copy_cells_kernel(const uint16_t* __restrict__ from, int nx, int ny, uint16_t* __restrict__ to,
                                                               int stride, int x_offset, int y_offset) {
  const int x = blockIdx.x * kBlock + threadIdx.x;
  if (x >= nx) return;
  for (int y = blockIdx.y; y < ny; y += gridDim.y)
    to[static_cast<size_t>(stride) * static_cast<size_t>(y + y_offset) + static_cast<size_t>(x + x_offset)] =
        from[static_cast<size_t>(nx) * static_cast<size_t>(y) + static_cast<size_t>(x)];
}

// DrawProbabilityGrid's loop (probability_grid_points_processor.cc:137-146), with Image::Rotate90DegreesClockwise
// (io/image.cc:67-76: new pixel (h - 1 - y, x) = old pixel (x, y), the new width is h) when `rotate`
__global__ __launch_bounds__(kBlock) void pg_draw_kernel(Cells g, int x0, int y0, int w, int h, const uint8_t* __restrict__ color,
                                                         int rotate, uint8_t* __restrict__ gray) {
  const int x = blockIdx.x * kBlock + threadIdx.x;
  if (x >= w) return;
  for (int y = blockIdx.y; y < h; y += gridDim.y) {
    const unsigned v = g.cells[static_cast<size_t>(g.nx) * static_cast<size_t>(y0 + y) + static_cast<size_t>(x0 + x)] & 32767u;
    const size_t at = rotate ? static_cast<size_t>(x) * static_cast<size_t>(h) + static_cast<size_t>(h - 1 - y)
                             : static_cast<size_t>(y) * static_cast<size_t>(w) + static_cast<size_t>(x);
    gray[at] = color[v];
  }
}

__global__ __launch_bounds__(kBlock) void pg_gather_cells_kernel(Cells g, const int* __restrict__ xy, unsigned n,
                                                                 unsigned* __restrict__ out) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int x = xy[2 * i], y = xy[2 * i + 1];
  const bool inside = static_cast<unsigned>(x) < static_cast<unsigned>(g.nx) && static_cast<unsigned>(y) < static_cast<unsigned>(g.ny);
  out[i] = inside ? g.cells[static_cast<size_t>(g.nx) * static_cast<size_t>(y) + static_cast<size_t>(x)] : 0xFFFFFFFFu;
}

inline unsigned blocks_of(int64_t n) { return dliom::blocks_of(n, kBlock); }
inline dim3 grid_2d(int w, int h) { return dim3(blocks_of(w), static_cast<unsigned>(std::min(h, 32768))); }

// ---- the tables of a 2D inserter and of the drawing (host, the reference's float expressions: probability_values.h) ----
void correspondence_cost_odds_table(float odds, uint16_t* t) {
  t[0] = static_cast<uint16_t>(correspondence_cost_to_value(1.f - probability_from_odds(odds)) + kUpdateMarker);
  for (unsigned cell = 1; cell != 32768u; ++cell) {
    const float p = 1.f - value_to_correspondence_cost(cell);
    t[cell] = static_cast<uint16_t>(correspondence_cost_to_value(1.f - probability_from_odds(odds * odds_of(p))) + kUpdateMarker);
  }
}

// ProbabilityToColor(GetProbability(index)) (probability_grid_points_processor.cc:49-54, :140-144)
void color_table(uint8_t* t) {
  t[0] = 128;  // kUnknownValue
  for (unsigned v = 1; v != 32768u; ++v) {
    const float probability_from_grid = 1.f - value_to_correspondence_cost(v);
    const float probability = 1.f - probability_from_grid;
    t[v] = static_cast<uint8_t>(std::lround(255 * ((probability - kMinProbability) / (kMaxProbability - kMinProbability))));
  }
}

// ---- limits (host) -------------------------------------------------------------------------------------------------
struct Limits {
  double resolution, max_x, max_y;
  int nx, ny;
};

// GrowLimits (grid_2d.cc:116-145) on the limits; ox / oy: where the old cell (0, 0) lands
int grow_limits(Limits* l, float px, float py, int64_t budget_bytes, int* ox, int* oy, int* doublings) {
  Limits g = *l;
  int x_total = 0, y_total = 0, turns = 0;
  for (;;) {
    int cx, cy;
    if (!cell_index(g.resolution, g.max_x, g.max_y, px, py, &cx, &cy)) return DLIOM_ERR_GRID_EXTENT;  // long -> int would wrap
    if (0 <= cx && 0 <= cy && cx < g.nx && cy < g.ny) break;
    const int x_offset = g.nx / 2, y_offset = g.ny / 2;
    if (g.nx > INT_MAX / (2 * kSubpixelScale) || g.ny > INT_MAX / (2 * kSubpixelScale)) return DLIOM_ERR_GRID_EXTENT;
    if (2ll * g.nx * 2ll * g.ny * 2ll > budget_bytes) return DLIOM_ERR_GRID_EXTENT;
    g.max_x = g.max_x + g.resolution * static_cast<double>(y_offset);  // limits_.max() + resolution * Vector2d(y_offset, x_offset)
    g.max_y = g.max_y + g.resolution * static_cast<double>(x_offset);
    x_total += x_offset;  // the array is embedded, not scaled: offsets add up
    y_total += y_offset;
    g.nx *= 2;
    g.ny *= 2;
    ++turns;
  }
  *l = g;
  *ox = x_total;
  *oy = y_total;
  *doublings = turns;
  return DLIOM_OK;
}

}  // namespace
}  // namespace dliom

using namespace dliom;

struct dliom_probability_grid {
  dliom_ctx* ctx = nullptr;
  std::shared_ptr<MemoryLedger> ledger;
  Limits limits{};
  uint16_t* d_cells = nullptr;
  uint8_t* d_color = nullptr;   // 32768 gray values
  unsigned* d_words = nullptr;  // kNumWords
  int64_t budget = 0;
  int box[4] = {0, 0, -1, -1};  // known_cells_box_: min x, min y, max x, max y; min > max: empty
  int64_t growths = 0, inserts = 0, visits = 0, booked = 0;
  unsigned error_word = 0;

  bool box_empty() const { return box[0] > box[2]; }
  int64_t cell_bytes() const { return 2ll * limits.nx * limits.ny; }
  int64_t bytes() const { return cell_bytes() + 32768 + kNumWords * 4; }
  Cells view() const { return Cells{d_cells, limits.nx, limits.ny}; }
  void book() {
    if (ledger) ledger->probability_grid_bytes += bytes() - booked;
    booked = bytes();
  }
};

struct dliom_inserter2d {
  dliom_ctx* ctx = nullptr;
  std::shared_ptr<MemoryLedger> ledger;
  bool insert_free_space = true;
  uint16_t* d_tables = nullptr;  // [hit 32768 | miss 32768]
};

namespace {

int create_grid(dliom_ctx* ctx, const Limits& limits, int64_t budget_bytes, dliom_probability_grid** out) {
  if (ctx == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!(limits.resolution > 0.0) || !std::isfinite(limits.resolution) || !std::isfinite(limits.max_x) || !std::isfinite(limits.max_y) ||
      limits.nx <= 0 || limits.ny <= 0 || !(limits.resolution / kSubpixelScale > 0.0))
    return DLIOM_ERR_INVALID_ARGUMENT;
  const int64_t budget = budget_bytes > 0 ? budget_bytes : DLIOM_PROBABILITY_GRID_DEFAULT_BUDGET_BYTES;
  if (limits.nx > INT_MAX / kSubpixelScale || limits.ny > INT_MAX / kSubpixelScale || 2ll * limits.nx * limits.ny > budget)
    return DLIOM_ERR_GRID_EXTENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  dliom_probability_grid* g = new dliom_probability_grid;
  g->ctx = ctx;
  g->ledger = ctx->ledger;
  g->limits = limits;
  g->budget = budget;
  std::vector<uint8_t> color(32768);
  color_table(color.data());
  int st = DLIOM_OK;
  if (hipMalloc(&g->d_cells, static_cast<size_t>(g->cell_bytes())) != hipSuccess || hipMalloc(&g->d_color, 32768) != hipSuccess ||
      hipMalloc(&g->d_words, kNumWords * 4) != hipSuccess)
    st = DLIOM_ERR_HIP;
  if (st == DLIOM_OK &&
      (hipMemsetAsync(g->d_cells, 0, static_cast<size_t>(g->cell_bytes()), ctx->stream) != hipSuccess ||
       hipMemsetAsync(g->d_words, 0, kNumWords * 4, ctx->stream) != hipSuccess ||
       hipMemcpyAsync(g->d_color, color.data(), 32768, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
       hipStreamSynchronize(ctx->stream) != hipSuccess))
    st = DLIOM_ERR_HIP;
  if (st != DLIOM_OK) {
    dliom_probability_grid_destroy(g);
    return st;
  }
  g->book();
  *out = g;
  return DLIOM_OK;
}

// the superscaled pixel of a point that the limits are known to contain (host twin of pg_ends_kernel)
bool super_pixel(const SuperLimits& s, float px, float py, int* x, int* y) {
  int sx, sy;
  if (!cell_index(s.resolution, s.max_x, s.max_y, px, py, &sx, &sy) || sx < 0 || sy < 0 || sx >= s.nx || sy >= s.ny) return false;
  *x = sx / kSubpixelScale;
  *y = sy / kSubpixelScale;
  return true;
}

}  // namespace

extern "C" {

int dliom_probability_grid_create(dliom_ctx* ctx, double resolution, int64_t budget_bytes, dliom_probability_grid** out) {
  constexpr int kInitialProbabilityGridSize = 100;
  const double max = 0.5 * kInitialProbabilityGridSize * resolution;  // (0.5 * 100) * resolution, then * Ones()
  return create_grid(ctx, Limits{resolution, max, max, kInitialProbabilityGridSize, kInitialProbabilityGridSize}, budget_bytes, out);
}

int dliom_probability_grid_create_with_limits(dliom_ctx* ctx, double resolution, double max_x, double max_y, int32_t num_x_cells,
                                              int32_t num_y_cells, int64_t budget_bytes, dliom_probability_grid** out) {
  return create_grid(ctx, Limits{resolution, max_x, max_y, num_x_cells, num_y_cells}, budget_bytes, out);
}

int dliom_probability_grid_destroy(dliom_probability_grid* g) {
  if (g == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  (void)hipSetDevice(g->ctx->device);
  (void)hipStreamSynchronize(g->ctx->stream);
  if (g->d_cells) (void)hipFree(g->d_cells);
  if (g->d_color) (void)hipFree(g->d_color);
  if (g->d_words) (void)hipFree(g->d_words);
  if (g->ledger) g->ledger->probability_grid_bytes -= g->booked;
  delete g;
  return DLIOM_OK;
}

int dliom_probability_grid_limits(const dliom_probability_grid* g, double* resolution, double max_xy[2], int32_t num_cells[2]) {
  if (g == nullptr || resolution == nullptr || max_xy == nullptr || num_cells == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *resolution = g->limits.resolution;
  max_xy[0] = g->limits.max_x;
  max_xy[1] = g->limits.max_y;
  num_cells[0] = g->limits.nx;
  num_cells[1] = g->limits.ny;
  return DLIOM_OK;
}

int dliom_probability_grid_memory_stats(const dliom_probability_grid* g, dliom_memory_stats* out) {
  if (g == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  std::memset(out, 0, sizeof *out);
  out->probability_grid_bytes = g->bytes();  // `grids` counts HybridGrids: 0 here, as in the context's statistics
  return DLIOM_OK;
}

int dliom_probability_grid_get_stats(const dliom_probability_grid* g, dliom_probability_grid_stats* out) {
  if (g == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  std::memset(out, 0, sizeof *out);
  out->bytes = g->bytes();
  out->growths = g->growths;
  out->inserts = g->inserts;
  out->cells_visited = g->visits;
  for (int k = 0; k < 4; ++k) out->known_box[k] = g->box[k];
  out->error_word = static_cast<int32_t>(g->error_word);
  return DLIOM_OK;
}

int dliom_probability_grid_grow_limits(double resolution, double max_xy[2], int32_t num_cells[2], float px, float py,
                                       int64_t budget_bytes, int32_t offset[2], int32_t* doublings) {
  if (max_xy == nullptr || num_cells == nullptr || offset == nullptr || doublings == nullptr || !(resolution > 0.0) ||
      !std::isfinite(resolution) || !std::isfinite(max_xy[0]) || !std::isfinite(max_xy[1]) || num_cells[0] <= 0 || num_cells[1] <= 0 ||
      !std::isfinite(px) || !std::isfinite(py))
    return DLIOM_ERR_INVALID_ARGUMENT;
  Limits l{resolution, max_xy[0], max_xy[1], num_cells[0], num_cells[1]};
  int ox = 0, oy = 0, turns = 0;
  DLIOM_TRY(grow_limits(&l, px, py, budget_bytes > 0 ? budget_bytes : DLIOM_PROBABILITY_GRID_DEFAULT_BUDGET_BYTES, &ox, &oy, &turns));
  max_xy[0] = l.max_x;
  max_xy[1] = l.max_y;
  num_cells[0] = l.nx;
  num_cells[1] = l.ny;
  offset[0] = ox;
  offset[1] = oy;
  *doublings = turns;
  return DLIOM_OK;
}

int dliom_compute_lookup_table_to_apply_correspondence_cost_odds(float odds, uint16_t* table) {
  if (table == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  correspondence_cost_odds_table(odds, table);
  return DLIOM_OK;
}

int dliom_probability_grid_color_table(uint8_t* table) {
  if (table == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  color_table(table);
  return DLIOM_OK;
}

int dliom_inserter2d_create(dliom_ctx* ctx, double hit_probability, double miss_probability, int insert_free_space,
                            dliom_inserter2d** out) {
  if (ctx == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  // CHECK_GT(hit_probability, 0.5), CHECK_LT(miss_probability, 0.5) (:43-44); NaN fails both
  if (!(hit_probability > 0.5) || !(miss_probability < 0.5)) return DLIOM_ERR_INVALID_ARGUMENT;
  std::vector<uint16_t> tables(65536);
  correspondence_cost_odds_table(odds_of(static_cast<float>(hit_probability)), tables.data());           // Odds(float p)
  correspondence_cost_odds_table(odds_of(static_cast<float>(miss_probability)), tables.data() + 32768);
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  dliom_inserter2d* ins = new dliom_inserter2d;
  ins->ctx = ctx;
  ins->ledger = ctx->ledger;
  ins->insert_free_space = insert_free_space != 0;
  if (hipMalloc(&ins->d_tables, 131072) != hipSuccess ||
      hipMemcpyAsync(ins->d_tables, tables.data(), 131072, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    if (ins->d_tables) (void)hipFree(ins->d_tables);
    delete ins;
    return DLIOM_ERR_HIP;
  }
  ins->ledger->probability_grid_bytes += 131072;
  *out = ins;
  return DLIOM_OK;
}

int dliom_inserter2d_destroy(dliom_inserter2d* ins) {
  if (ins == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  (void)hipSetDevice(ins->ctx->device);
  (void)hipStreamSynchronize(ins->ctx->stream);
  if (ins->d_tables) (void)hipFree(ins->d_tables);
  if (ins->ledger) ins->ledger->probability_grid_bytes -= 131072;
  delete ins;
  return DLIOM_OK;
}

int dliom_inserter2d_tables(const dliom_inserter2d* ins, uint16_t* hit_table, uint16_t* miss_table) {
  if (ins == nullptr || hit_table == nullptr || miss_table == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_ctx* ctx = ins->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_HIP_TRY(hipMemcpyAsync(hit_table, ins->d_tables, 65536, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipMemcpyAsync(miss_table, ins->d_tables + 32768, 65536, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  return DLIOM_OK;
}

int dliom_inserter2d_insert_cloud(dliom_inserter2d* ins, dliom_probability_grid* g, const float origin[3], const dliom_cloud* points) {
  if (ins == nullptr || g == nullptr || origin == nullptr || points == nullptr || ins->ctx != g->ctx || points->ctx != g->ctx ||
      points->n < 0 || points->n > INT32_MAX)
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(origin[0]) || !std::isfinite(origin[1])) return DLIOM_ERR_INVALID_ARGUMENT;  // origin.head<2>(): z is never read
  dliom_ctx* ctx = g->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const unsigned n = static_cast<unsigned>(points->n);
  unsigned* host = pinned_at<unsigned>(ctx, kPinReadback);

  // GrowAsNeeded (ray_casting.cc:148-162): the box of the origin and the returns
  float lo_x = origin[0], lo_y = origin[1], hi_x = origin[0], hi_y = origin[1];
  float pts_lo_x = 0.f, pts_lo_y = 0.f, pts_hi_x = 0.f, pts_hi_y = 0.f;  // of the returns alone (n > 0)
  int span = -1;
  if (n > 0) {
    const FillJob fills[2] = {{g->d_words + kWordFlag, 4, 0u}, {g->d_words + kWordNotMinX, 16, 0u}};
    DLIOM_TRY(fill_multi(ctx, fills, 2));
    span = ctx->begin_span(DLIOM_KERNEL_PG_HITS);
    hipLaunchKernelGGL(pg_bounds_kernel, dim3(std::min(blocks_of(n), 256u)), dim3(kBlock), 0, ctx->stream, points->d_x, points->d_y, n,
                       g->d_words);
    ctx->end_span(span);
    DLIOM_HIP_TRY(hipGetLastError());
    const GatherJob back[2] = {{g->d_words + kWordFlag, 1}, {g->d_words + kWordNotMinX, 4}};
    DLIOM_TRY(gather_and_wait(ctx, back, 2, host));
    if (host[0] != 0u) return DLIOM_ERR_INVALID_ARGUMENT;  // a non-finite coordinate: nothing was touched
    pts_lo_x = key_float(~host[1]);
    pts_lo_y = key_float(~host[2]);
    pts_hi_x = key_float(host[3]);
    pts_hi_y = key_float(host[4]);
    lo_x = std::min(lo_x, pts_lo_x);
    lo_y = std::min(lo_y, pts_lo_y);
    hi_x = std::max(hi_x, pts_hi_x);
    hi_y = std::max(hi_y, pts_hi_y);
  }
  constexpr float kPadding = 1e-6f;
  Limits grown = g->limits;
  int ox1 = 0, oy1 = 0, ox2 = 0, oy2 = 0, turns1 = 0, turns2 = 0;
  DLIOM_TRY(grow_limits(&grown, lo_x - kPadding * 1.f, lo_y - kPadding * 1.f, g->budget, &ox1, &oy1, &turns1));  // the min corner first
  DLIOM_TRY(grow_limits(&grown, hi_x + kPadding * 1.f, hi_y + kPadding * 1.f, g->budget, &ox2, &oy2, &turns2));
  const int turns = turns1 + turns2;
  const int x_offset = ox1 + ox2, y_offset = oy1 + oy2;  // where the old cell (0, 0) lands after both calls

  // what a refusal after this point restores
  const Limits old_limits = g->limits;
  uint16_t* const old_cells = g->d_cells;
  bool grew = false;
  if (turns > 0) {
    uint16_t* cells = nullptr;
    const size_t bytes = 2 * static_cast<size_t>(grown.nx) * static_cast<size_t>(grown.ny);
    DLIOM_HIP_TRY(hipMalloc(&cells, bytes));
    if (hipMemsetAsync(cells, 0, bytes, ctx->stream) != hipSuccess) {
      (void)hipFree(cells);
      return DLIOM_ERR_HIP;
    }
    hipLaunchKernelGGL(pg_copy_cells_kernel, grid_2d(old_limits.nx, old_limits.ny), dim3(kBlock), 0, ctx->stream, old_cells,
                       old_limits.nx, old_limits.ny, cells, grown.nx, x_offset, y_offset);
    if (hipGetLastError() != hipSuccess) {
      (void)hipStreamSynchronize(ctx->stream);
      (void)hipFree(cells);
      return DLIOM_ERR_HIP;
    }
    g->d_cells = cells;
    g->limits = grown;
    grew = true;
  }
  auto restore = [&]() {  // the stream is idle (a read-back has just been waited for) or is drained here
    if (grew) {
      (void)hipStreamSynchronize(ctx->stream);
      (void)hipFree(g->d_cells);
      g->d_cells = old_cells;
      g->limits = old_limits;
    }
  };
  auto commit_growth = [&]() {
    if (!grew) return;
    (void)hipFree(old_cells);  // the stream has been waited for: the copy is done
    if (!g->box_empty()) {     // known_cells_box_.translate (grid_2d.cc:141-143), once per doubling
      g->box[0] += x_offset;
      g->box[2] += x_offset;
      g->box[1] += y_offset;
      g->box[3] += y_offset;
    }
    g->growths += turns;
    g->book();
  };

  if (n == 0) {  // an empty batch still grows to hold the origin; nothing is applied
    if (grew && hipStreamSynchronize(ctx->stream) != hipSuccess) {
      restore();
      return DLIOM_ERR_HIP;
    }
    commit_growth();
    ++g->inserts;
    return DLIOM_OK;
  }

  const SuperLimits super{g->limits.resolution / kSubpixelScale, g->limits.max_x, g->limits.max_y, g->limits.nx * kSubpixelScale,
                          g->limits.ny * kSubpixelScale};
  // The pixel box of the batch from its extreme coordinates: GetCellIndex is monotone (non-increasing) in the coordinate,
  // and the largest coordinates give the smallest indices.  It is the box FinishUpdate sweeps and what the known-cells box
  // is extended by: a supercover line stays inside the pixel box of its two ends.
  int begin_x = 0, begin_y = 0, ex0 = 0, ey0 = 0, ex1 = 0, ey1 = 0;
  bool ok = cell_index(super.resolution, super.max_x, super.max_y, origin[0], origin[1], &begin_x, &begin_y) && begin_x >= 0 &&
            begin_y >= 0 && begin_x < super.nx && begin_y < super.ny;
  ok = super_pixel(super, pts_hi_x, pts_hi_y, &ex0, &ey0) && ok;  // (min cell x, min cell y)
  ok = super_pixel(super, pts_lo_x, pts_lo_y, &ex1, &ey1) && ok;  // (max cell x, max cell y)
  if (!ok) {
    restore();
    return DLIOM_ERR_GRID_EXTENT;
  }
  const int bpx = begin_x / kSubpixelScale, bpy = begin_y / kSubpixelScale;
  int box_x0 = ex0, box_y0 = ey0, box_x1 = ex1, box_y1 = ey1;
  if (ins->insert_free_space) {
    box_x0 = std::min(box_x0, bpx);
    box_y0 = std::min(box_y0, bpy);
    box_x1 = std::max(box_x1, bpx);
    box_y1 = std::max(box_y1, bpy);
  }

  // The export stages' scratch (dliom_ctx::outlier, shared with compact.hip's compaction): every user's contents live
  // only within one call, in stream order, so the ends may sit there until this call's last read-back.
  if (ctx->outlier.reserve(static_cast<size_t>(n) * sizeof(int2)) != DLIOM_OK) {
    restore();
    return DLIOM_ERR_HIP;
  }
  int2* d_ends = ctx->outlier.as<int2>();
  const Cells cells = g->view();
  span = ctx->begin_span(DLIOM_KERNEL_PG_HITS);
  hipLaunchKernelGGL(pg_ends_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, points->d_x, points->d_y, n, super, d_ends,
                     g->d_words);
  hipLaunchKernelGGL(pg_apply_hits_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, d_ends, n, cells, ins->d_tables,
                     g->d_words);
  ctx->end_span(span);
  if (ins->insert_free_space) {
    span = ctx->begin_span(DLIOM_KERNEL_PG_RAYS);
    hipLaunchKernelGGL(pg_cast_rays_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, d_ends, n, begin_x, begin_y, cells,
                       ins->d_tables + 32768, g->d_words);
    ctx->end_span(span);
  }
  span = ctx->begin_span(DLIOM_KERNEL_PG_CLEAR);
  hipLaunchKernelGGL(pg_clear_marker_kernel, grid_2d(box_x1 - box_x0 + 1, box_y1 - box_y0 + 1), dim3(kBlock), 0, ctx->stream, cells,
                     box_x0, box_y0, box_x1 - box_x0 + 1, box_y1 - box_y0 + 1);
  ctx->end_span(span);
  if (hipGetLastError() != hipSuccess) {
    restore();
    return DLIOM_ERR_HIP;
  }
  unsigned back[4];  // flag, error, visits (u64)
  const int st = read_words(ctx, g->d_words, 0, 4, back);
  if (st != DLIOM_OK) {
    restore();
    return st;
  }
  if (back[0] != 0u) {  // a superscaled end outside the grid: no pass wrote anything
    restore();
    return DLIOM_ERR_GRID_EXTENT;
  }
  commit_growth();
  g->error_word = back[1];
  g->visits = words64(back, 2);
  // mutable_known_cells_box()->extend of every cell touched (probability_grid.cc:62); also when the error word is set: the
  // passes have written, and the box must go on agreeing with the cells
  if (g->box_empty()) {
    g->box[0] = box_x0;
    g->box[1] = box_y0;
    g->box[2] = box_x1;
    g->box[3] = box_y1;
  } else {
    g->box[0] = std::min(g->box[0], box_x0);
    g->box[1] = std::min(g->box[1], box_y0);
    g->box[2] = std::max(g->box[2], box_x1);
    g->box[3] = std::max(g->box[3], box_y1);
  }
  ++g->inserts;
  return g->error_word != 0u ? DLIOM_ERR_INTERNAL : DLIOM_OK;
}

int dliom_inserter2d_insert(dliom_inserter2d* ins, dliom_probability_grid* g, const float origin[3], const float* points_xyz,
                            int64_t n) {
  if (ins == nullptr || g == nullptr || origin == nullptr || ins->ctx != g->ctx || n < 0 || n > INT32_MAX ||
      (n > 0 && points_xyz == nullptr))
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(origin[0]) || !std::isfinite(origin[1])) return DLIOM_ERR_INVALID_ARGUMENT;  // origin.head<2>(): z is never read
  dliom_cloud* cloud = nullptr;
  DLIOM_TRY(dliom_cloud_create(g->ctx, points_xyz, n, &cloud));
  const int st = dliom_inserter2d_insert_cloud(ins, g, origin, cloud);
  dliom_cloud_destroy(cloud);
  return st;
}

int dliom_probability_grid_cells(const dliom_probability_grid* g, uint16_t* cells, int64_t capacity, int32_t offset[2],
                                 int32_t num_cells[2], int cropped) {
  if (g == nullptr || offset == nullptr || num_cells == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  int x0 = 0, y0 = 0, w = g->limits.nx, h = g->limits.ny;
  if (cropped) {  // ComputeCroppedLimits (grid_2d.cc:101-111)
    if (g->box_empty()) {
      w = h = 1;
    } else {
      x0 = g->box[0];
      y0 = g->box[1];
      w = g->box[2] - g->box[0] + 1;
      h = g->box[3] - g->box[1] + 1;
    }
  }
  offset[0] = x0;
  offset[1] = y0;
  num_cells[0] = w;
  num_cells[1] = h;
  if (cells == nullptr) return DLIOM_OK;
  if (capacity < static_cast<int64_t>(w) * h) return DLIOM_ERR_CAPACITY;
  dliom_ctx* ctx = g->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_HIP_TRY(hipMemcpy2DAsync(cells, static_cast<size_t>(w) * 2, g->d_cells + (static_cast<size_t>(g->limits.nx) * y0 + x0),
                                 static_cast<size_t>(g->limits.nx) * 2, static_cast<size_t>(w) * 2, static_cast<size_t>(h),
                                 hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  return DLIOM_OK;
}

int dliom_probability_grid_get_probabilities(const dliom_probability_grid* g, const int32_t* cell_xy, int64_t n, float* probabilities,
                                             uint8_t* known) {
  if (g == nullptr || n < 0 || n > INT32_MAX || (n > 0 && (cell_xy == nullptr || probabilities == nullptr)))
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (n == 0) return DLIOM_OK;
  dliom_ctx* ctx = g->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(ctx->misc.reserve(static_cast<size_t>(n) * 12));
  int* d_xy = ctx->misc.as<int>();
  unsigned* d_out = ctx->misc.as<unsigned>() + 2 * n;
  std::vector<unsigned> values(static_cast<size_t>(n));
  DLIOM_HIP_TRY(hipMemcpyAsync(d_xy, cell_xy, static_cast<size_t>(n) * 8, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(pg_gather_cells_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, g->view(), d_xy, static_cast<unsigned>(n),
                     d_out);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipMemcpyAsync(values.data(), d_out, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  for (int64_t i = 0; i < n; ++i) {
    const bool inside = values[i] != 0xFFFFFFFFu;
    // probability_grid.cc:69-73: !Contains -> kMinProbability, else CorrespondenceCostToProbability(ValueToCorrespondenceCost(cell))
    probabilities[i] = inside ? 1.f - value_to_correspondence_cost(values[i]) : kMinProbability;
    if (known != nullptr) known[i] = inside && (values[i] & 0xFFFFu) != 0u ? 1 : 0;
  }
  return DLIOM_OK;
}

int dliom_probability_grid_draw(const dliom_probability_grid* g, uint8_t* gray, int64_t capacity, int32_t offset[2], int32_t size[2],
                                int rotate_cw) {
  if (g == nullptr || offset == nullptr || size == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  int32_t num[2];
  DLIOM_TRY(dliom_probability_grid_cells(g, nullptr, 0, offset, num, 1));
  size[0] = rotate_cw ? num[1] : num[0];
  size[1] = rotate_cw ? num[0] : num[1];
  if (gray == nullptr) return DLIOM_OK;
  const int64_t pixels = static_cast<int64_t>(num[0]) * num[1];
  if (capacity < pixels) return DLIOM_ERR_CAPACITY;
  dliom_ctx* ctx = g->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(ctx->outlier.reserve(static_cast<size_t>(pixels)));  // the export stages' per-call scratch (see the insert)
  uint8_t* d_gray = ctx->outlier.as<uint8_t>();
  hipLaunchKernelGGL(pg_draw_kernel, grid_2d(num[0], num[1]), dim3(kBlock), 0, ctx->stream, g->view(), offset[0], offset[1], num[0], num[1],
                     g->d_color, rotate_cw ? 1 : 0, d_gray);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipMemcpyAsync(gray, d_gray, static_cast<size_t>(pixels), hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  return DLIOM_OK;
}

int dliom_ros_map_yaml_origin(double resolution, const double max_xy[2], const int32_t offset[2], int32_t width, int32_t height,
                              double origin[2]) {
  if (max_xy == nullptr || offset == nullptr || origin == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  // limits.max().x() - (offset.y() + image->width()) * limits.resolution(), ... (ros_map_writing_points_processor.cc:73-76)
  origin[0] = max_xy[0] - (offset[1] + width) * resolution;
  origin[1] = max_xy[1] - (offset[0] + height) * resolution;
  return DLIOM_OK;
}

static int copy_text(const std::string& text, char* buffer, int64_t capacity, int64_t* length) {
  *length = static_cast<int64_t>(text.size());
  if (buffer == nullptr || capacity < *length) return DLIOM_ERR_CAPACITY;
  std::memcpy(buffer, text.data(), text.size());
  return DLIOM_OK;
}

int dliom_ros_map_pgm_header(double resolution, int32_t width, int32_t height, char* buffer, int64_t capacity, int64_t* length) {
  if (length == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  const std::string header = "P5\n# Cartographer map; " + std::to_string(resolution) + " m/pixel\n" + std::to_string(width) + " " +
                             std::to_string(height) + "\n255\n";
  return copy_text(header, buffer, capacity, length);
}

int dliom_ros_map_yaml(double resolution, const double origin[2], const char* pgm_filename, char* buffer, int64_t capacity,
                       int64_t* length) {
  if (length == nullptr || origin == nullptr || pgm_filename == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  const std::string output = "image: " + std::string(pgm_filename) + "\n" + "resolution: " + std::to_string(resolution) + "\n" +
                             "origin: [" + std::to_string(origin[0]) + ", " + std::to_string(origin[1]) +
                             ", 0.0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n";
  return copy_text(output, buffer, capacity, length);
}

}  // extern "C"
