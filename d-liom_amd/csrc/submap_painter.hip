// Painting submap slices into one map (io::PaintSubmapSlices, io/submap_painter.cc:30-108, and CreateOccupancyGridMsg,
// cartographer_ros msg_conversion.cc:321-368) on the device: dliom.h "painting submap slices into one map" states the
// problem, submap_painter_layout.h is its host half (matrices, layout, inverse, list sizing), this file the gather.
//
// A paint is four launches whatever the number of slices:
//   1. painter_count_kernel   one thread a 16 x 16 tile: how many slices' reach (layout.h: reach) touch it
//   2. painter_scan_kernel    one workgroup: exclusive sum of the counts (at most 2^18 tiles, 4096 a round)
//   3. painter_fill_kernel    one thread a tile again: the touching slices' indices, in the order given
//   4. painter_paint_kernel   one workgroup a tile, one wave an 8 x 8 block, one thread a pixel: walks the tile's list --
//                             uniform over the workgroup, so a slice's record comes by scalar loads --, samples four
//                             texels a slice, composites in registers, writes the pixel (or its occupancy byte) once.
// No atomics and no float arithmetic on the device; a slice outside a tile's list contributes nothing to its pixels (the
// composite of a zero sample leaves a pixel as it is), so the lists change the work, never the result.
#include <cstring>
#include <vector>

#include "device_common.h"
#include "submap_painter_layout.h"

struct dliom_submap_slice {
  dliom_ctx* ctx = nullptr;
  uint8_t* d_cells = nullptr;  // height * width (intensity, alpha) pairs; null when there are none
  dliom_submap_slice_description d = {};
};

namespace dliom {
namespace {

using painter::kTile;

struct SliceRecord {  // 80 bytes, read by scalar loads
  long long A, B, E, C, D, G;
  const uint16_t* cells;  // intensity | alpha << 8
  int w, h;
  int x0, y0, x1, y1;  // reach, in pixels
};

struct PaintArgs {
  const SliceRecord* slices;
  int n;
  int width, height, tiles_x, tiles_y;
  unsigned* offsets;  // tiles + 1: counts, then their exclusive sum
  unsigned* list;
  unsigned pairs;  // the list's size as the host computed it (layout.h: tile_pairs)
  const int8_t* table;  // occupancy table
  uint32_t* pixels;
  int8_t* cells;
};

__device__ __forceinline__ bool touches(const SliceRecord& s, int tx, int ty) {
  return s.x0 <= tx * kTile + kTile - 1 && s.x1 >= tx * kTile && s.y0 <= ty * kTile + kTile - 1 && s.y1 >= ty * kTile;
}

__global__ void painter_count_kernel(PaintArgs a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, tiles = a.tiles_x * a.tiles_y;
  if (t > tiles) return;
  unsigned count = 0;
  if (t < tiles) {
    const int tx = t % a.tiles_x, ty = t / a.tiles_x;
    for (int i = 0; i < a.n; ++i) count += touches(a.slices[i], tx, ty) ? 1u : 0u;
  }
  a.offsets[t] = count;  // entry `tiles`: 0, the scan turns it into the total
}

constexpr int kScanThreads = 1024;
// In place, one workgroup, 4096 entries a round: a thread takes four neighbours (one 16-byte load), a wave scans its 64
// sums by shuffles, the 16 wave sums go through LDS, the rounds' total is carried in a register.
__global__ __launch_bounds__(kScanThreads) void painter_scan_kernel(unsigned* v, int m) {
  __shared__ unsigned wave_sums[kScanThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned carry = 0;
  for (int base = 0; base < m; base += 4 * kScanThreads) {
    const int i = base + 4 * static_cast<int>(threadIdx.x);
    unsigned c[4] = {0u, 0u, 0u, 0u};
    if (i + 3 < m) {
      const uint4 q = *reinterpret_cast<const uint4*>(v + i);  // v is 256-byte aligned, i a multiple of 4
      c[0] = q.x, c[1] = q.y, c[2] = q.z, c[3] = q.w;
    } else {
      for (int k = 0; k < 4; ++k)
        if (i + k < m) c[k] = v[i + k];
    }
    const unsigned own = c[0] + c[1] + c[2] + c[3];
    unsigned inclusive = own;
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned below = static_cast<unsigned>(__shfl_up(static_cast<int>(inclusive), d, 64));
      if (lane >= d) inclusive += below;
    }
    if (lane == 63) wave_sums[wave] = inclusive;
    __syncthreads();
    unsigned before = carry, total = 0;
    for (int w = 0; w < kScanThreads / 64; ++w) {
      const unsigned sum = wave_sums[w];
      before += w < wave ? sum : 0u;
      total += sum;
    }
    unsigned at = before + inclusive - own;
    if (i + 3 < m) {
      *reinterpret_cast<uint4*>(v + i) = make_uint4(at, at + c[0], at + c[0] + c[1], at + c[0] + c[1] + c[2]);
    } else {
      for (int k = 0; k < 4; ++k) {
        if (i + k < m) v[i + k] = at;
        at += c[k];
      }
    }
    carry += total;
    __syncthreads();  // wave_sums is written again in the next round
  }
}

__global__ void painter_fill_kernel(PaintArgs a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.tiles_x * a.tiles_y) return;
  const int tx = t % a.tiles_x, ty = t / a.tiles_x;
  unsigned at = a.offsets[t];
  const unsigned end = min(a.offsets[t + 1], a.pairs);
  for (int i = 0; i < a.n && at < end; ++i)
    if (touches(a.slices[i], tx, ty)) a.list[at++] = static_cast<unsigned>(i);
}

// the texel's (alpha, intensity, observed) or zeros outside the slice
__device__ __forceinline__ void fetch(const SliceRecord& s, int x, int y, unsigned* alpha, unsigned* red, unsigned* green) {
  const bool inside = static_cast<unsigned>(x) < static_cast<unsigned>(s.w) && static_cast<unsigned>(y) < static_cast<unsigned>(s.h);
  const unsigned v = inside ? s.cells[static_cast<size_t>(y) * s.w + x] : 0u;
  *alpha = v >> 8;
  *red = v & 255u;
  *green = v != 0u ? 255u : 0u;
}

__device__ __forceinline__ unsigned over(unsigned s, unsigned d, unsigned inverse_alpha) {
  const unsigned t = d * inverse_alpha + 128u;
  const unsigned r = s + (((t >> 8) + t) >> 8);
  return r > 255u ? 255u : r;
}

template <bool kOccupancy>
__global__ __launch_bounds__(kTile* kTile) void painter_paint_kernel(PaintArgs a) {
  const int tile = blockIdx.x, tx = tile % a.tiles_x, ty = tile / a.tiles_x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = tx * kTile + (wave & 1) * 8 + (lane & 7), y = ty * kTile + (wave >> 1) * 8 + (lane >> 3);
  unsigned alpha = 255u, red = 128u, green = 0u;  // 0xFF800000; blue starts at 0 and every texel's blue is 0: it stays 0
  const unsigned first = a.offsets[tile], end = min(a.offsets[tile + 1], a.pairs);
  for (unsigned k = first; k < end; ++k) {
    const SliceRecord& s = a.slices[a.list[k]];
    const long long half = 1ll << 31;
    const long long U = s.A * x + s.B * y + s.E + ((s.A + s.B) >> 1) - half;
    const long long V = s.C * x + s.D * y + s.G + ((s.C + s.D) >> 1) - half;
    const int x1 = static_cast<int>(U >> 32), y1 = static_cast<int>(V >> 32);
    if (x1 < -1 || x1 >= s.w || y1 < -1 || y1 >= s.h) continue;  // all four texels outside: a zero sample
    const unsigned dx = (static_cast<unsigned>(U >> 25) & 127u) << 1, dy = (static_cast<unsigned>(V >> 25) & 127u) << 1;
    const unsigned w_br = dx * dy, w_tr = (dx << 8) - w_br, w_bl = (dy << 8) - w_br;
    const unsigned w_tl = 65536u - (dx << 8) - (dy << 8) + w_br;
    unsigned ta[4], tr[4], tg[4];
    fetch(s, x1, y1, &ta[0], &tr[0], &tg[0]);
    fetch(s, x1 + 1, y1, &ta[1], &tr[1], &tg[1]);
    fetch(s, x1, y1 + 1, &ta[2], &tr[2], &tg[2]);
    fetch(s, x1 + 1, y1 + 1, &ta[3], &tr[3], &tg[3]);
    const unsigned sa = (ta[0] * w_tl + ta[1] * w_tr + ta[2] * w_bl + ta[3] * w_br) >> 16;
    const unsigned sr = (tr[0] * w_tl + tr[1] * w_tr + tr[2] * w_bl + tr[3] * w_br) >> 16;
    const unsigned sg = (tg[0] * w_tl + tg[1] * w_tr + tg[2] * w_bl + tg[3] * w_br) >> 16;
    const unsigned inverse_alpha = 255u - sa;
    alpha = over(sa, alpha, inverse_alpha);
    red = over(sr, red, inverse_alpha);
    green = over(sg, green, inverse_alpha);
  }
  if (x >= a.width || y >= a.height) return;
  if (kOccupancy) {
    a.cells[static_cast<size_t>(a.height - 1 - y) * a.width + x] = green == 0u ? static_cast<int8_t>(-1) : a.table[red];
  } else {
    a.pixels[static_cast<size_t>(y) * a.width + x] = alpha << 24 | red << 16 | green << 8;
  }
}

int check_pose(const double* p) { return p != nullptr && painter::finite7(p) ? DLIOM_OK : DLIOM_ERR_INVALID_ARGUMENT; }

int new_slice(dliom_ctx* ctx, int32_t width, int32_t height, double resolution, const double* slice_pose7, const double* pose7,
              dliom_submap_slice** out) {
  dliom_submap_slice* s = new dliom_submap_slice;
  s->ctx = ctx;
  s->d.width = width;
  s->d.height = height;
  s->d.resolution = resolution;
  std::memcpy(s->d.slice_pose7, slice_pose7, sizeof s->d.slice_pose7);
  std::memcpy(s->d.pose7, pose7, sizeof s->d.pose7);
  const size_t bytes = static_cast<size_t>(width) * height * 2;
  if (bytes > 0) {
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_cells), bytes);
    if (e != hipSuccess) {
      delete s;
      DLIOM_HIP_TRY(e);
    }
  }
  *out = s;
  return DLIOM_OK;
}

// sizes, then (buffer given and large enough) the paint; exactly one of pixels / cells is non-null for a paint
int paint(dliom_ctx* ctx, const dliom_submap_slice* const* slices, int64_t n, double resolution, uint32_t* pixels, int8_t* cells,
          int64_t capacity, int32_t* width, int32_t* height, float origin2f[2], double origin_xy[2], bool occupancy) {
  if (slices == nullptr || width == nullptr || height == nullptr || capacity < 0 || n <= 0) return DLIOM_ERR_INVALID_ARGUMENT;
  if (ctx == nullptr && slices[0] != nullptr) ctx = slices[0]->ctx;  // dliom.h: NULL = the slices' context
  if (ctx == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  if (n > DLIOM_SUBMAP_PAINTER_MAX_SLICES) return DLIOM_ERR_TOO_LARGE;
  std::vector<dliom_submap_slice_description> d(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    if (slices[i] == nullptr || slices[i]->ctx != ctx) return DLIOM_ERR_INVALID_ARGUMENT;
    d[static_cast<size_t>(i)] = slices[i]->d;
  }
  painter::Layout L;
  const int status = painter::layout(d.data(), n, resolution, &L);
  if (status != DLIOM_OK && status != DLIOM_ERR_CAPACITY) return status;
  *width = L.width;
  *height = L.height;
  if (origin2f != nullptr) origin2f[0] = L.origin[0], origin2f[1] = L.origin[1];
  if (origin_xy != nullptr) painter::occupancy_origin(L.origin, L.height, resolution, origin_xy);
  if (status != DLIOM_OK) return status;
  std::vector<SliceRecord> records(static_cast<size_t>(n));
  std::vector<painter::Box> boxes(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    const size_t k = static_cast<size_t>(i);
    painter::Fixed f;
    DLIOM_TRY(painter::invert(L.matrices[k], L.origin, L.width, L.height, &f));
    boxes[k] = painter::reach(L.matrices[k], L.origin, d[k].width, d[k].height, L.width, L.height);
    records[k] = SliceRecord{f.A, f.B, f.E, f.C, f.D, f.G, reinterpret_cast<const uint16_t*>(slices[i]->d_cells),
                             d[k].width, d[k].height, boxes[k].x0, boxes[k].y0, boxes[k].x1, boxes[k].y1};
  }
  const int64_t pairs = painter::tile_pairs(boxes.data(), n);
  if (pairs > DLIOM_SUBMAP_PAINTER_MAX_PAIRS) return DLIOM_ERR_TOO_LARGE;
  const int64_t count = static_cast<int64_t>(L.width) * L.height;
  if (pixels == nullptr && cells == nullptr) return DLIOM_OK;
  if (capacity < count) return DLIOM_ERR_CAPACITY;

  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int tiles_x = (L.width + kTile - 1) / kTile, tiles_y = (L.height + kTile - 1) / kTile, tiles = tiles_x * tiles_y;
  const size_t record_bytes = sizeof(SliceRecord) * static_cast<size_t>(n);
  const size_t o_table = align256(record_bytes), o_offsets = o_table + 256,
               o_list = o_offsets + align256(4 * (static_cast<size_t>(tiles) + 1)),
               o_out = o_list + align256(4 * static_cast<size_t>(pairs) + 4),
               total = o_out + align256(static_cast<size_t>(count) * (occupancy ? 1 : 4));
  DLIOM_TRY(ctx->painter.reserve(total));
  char* base = static_cast<char*>(ctx->painter.p);
  // records and table in one upload; the staging vector lives until the synchronise below
  std::vector<char> staging(o_table + 256);
  std::memcpy(staging.data(), records.data(), record_bytes);
  painter::occupancy_table(reinterpret_cast<int8_t*>(staging.data() + o_table));
  DLIOM_HIP_TRY(hipMemcpyAsync(base, staging.data(), staging.size(), hipMemcpyHostToDevice, st));
  PaintArgs a;
  a.slices = reinterpret_cast<const SliceRecord*>(base);
  a.n = static_cast<int>(n);
  a.width = L.width;
  a.height = L.height;
  a.tiles_x = tiles_x;
  a.tiles_y = tiles_y;
  a.offsets = reinterpret_cast<unsigned*>(base + o_offsets);
  a.list = reinterpret_cast<unsigned*>(base + o_list);
  a.pairs = static_cast<unsigned>(pairs);
  a.table = reinterpret_cast<const int8_t*>(base + o_table);
  a.pixels = occupancy ? nullptr : reinterpret_cast<uint32_t*>(base + o_out);
  a.cells = occupancy ? reinterpret_cast<int8_t*>(base + o_out) : nullptr;
  int64_t launches = 0;
  hipLaunchKernelGGL(painter_count_kernel, dim3(blocks_of(tiles + 1, 256)), dim3(256), 0, st, a);
  DLIOM_HIP_TRY(hipGetLastError());
  ++launches;
  hipLaunchKernelGGL(painter_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, a.offsets, tiles + 1);
  DLIOM_HIP_TRY(hipGetLastError());
  ++launches;
  hipLaunchKernelGGL(painter_fill_kernel, dim3(blocks_of(tiles, 256)), dim3(256), 0, st, a);
  DLIOM_HIP_TRY(hipGetLastError());
  ++launches;
  if (occupancy) hipLaunchKernelGGL(painter_paint_kernel<true>, dim3(static_cast<unsigned>(tiles)), dim3(kTile * kTile), 0, st, a);
  else hipLaunchKernelGGL(painter_paint_kernel<false>, dim3(static_cast<unsigned>(tiles)), dim3(kTile * kTile), 0, st, a);
  DLIOM_HIP_TRY(hipGetLastError());
  ++launches;
  if (occupancy) DLIOM_HIP_TRY(hipMemcpyAsync(cells, base + o_out, static_cast<size_t>(count), hipMemcpyDeviceToHost, st));
  else DLIOM_HIP_TRY(hipMemcpyAsync(pixels, base + o_out, static_cast<size_t>(count) * 4, hipMemcpyDeviceToHost, st));
  DLIOM_HIP_TRY(hipStreamSynchronize(st));
  ++ctx->host_syncs;
  ctx->painter_launches = launches;
  ctx->painter_pairs = pairs;
  return DLIOM_OK;
}

}  // namespace
}  // namespace dliom

using namespace dliom;

extern "C" {

int dliom_submap_slice_create(dliom_ctx* ctx, const uint8_t* cells, int32_t width, int32_t height, double resolution,
                              const double slice_pose7[7], const double pose7[7], dliom_submap_slice** out) {
  if (ctx == nullptr || out == nullptr || width < 0 || height < 0 || !std::isfinite(resolution) || !(resolution > 0.) ||
      check_pose(slice_pose7) != DLIOM_OK || check_pose(pose7) != DLIOM_OK)
    return DLIOM_ERR_INVALID_ARGUMENT;
  const int64_t texels = static_cast<int64_t>(width) * height;
  if (texels > 0 && cells == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  if (texels > DLIOM_XRAY_MAX_PIXELS) return DLIOM_ERR_TOO_LARGE;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  dliom_submap_slice* s = nullptr;
  DLIOM_TRY(new_slice(ctx, width, height, resolution, slice_pose7, pose7, &s));
  if (texels > 0) {
    hipError_t e = hipMemcpyAsync(s->d_cells, cells, static_cast<size_t>(texels) * 2, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      dliom_submap_slice_destroy(s);
      DLIOM_HIP_TRY(e);
    }
    ++ctx->host_syncs;
    ctx->painter_texels_uploaded += texels;
  }
  *out = s;
  return DLIOM_OK;
}

int dliom_submap_slice_create_from_grid(const dliom_grid* grid, const double global_submap_pose7[7], dliom_submap_slice** out) {
  if (grid == nullptr || out == nullptr || check_pose(global_submap_pose7) != DLIOM_OK) return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_ctx* ctx = grid->ctx;
  const uint8_t* cells = nullptr;
  int32_t width = 0, height = 0;
  double resolution = 0., slice_pose[7];
  DLIOM_TRY(xray_texture_on_device(grid, global_submap_pose7, &cells, &width, &height, &resolution, slice_pose));
  dliom_submap_slice* s = nullptr;
  DLIOM_TRY(new_slice(ctx, width, height, resolution, slice_pose, global_submap_pose7, &s));
  if (s->d_cells != nullptr) {
    hipError_t e = hipMemcpyAsync(s->d_cells, cells, static_cast<size_t>(width) * height * 2, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the context's next projection reuses the source
    if (e != hipSuccess) {
      dliom_submap_slice_destroy(s);
      DLIOM_HIP_TRY(e);
    }
    ++ctx->host_syncs;
  }
  *out = s;
  return DLIOM_OK;
}

int dliom_submap_slice_set_pose(dliom_submap_slice* slice, const double pose7[7]) {
  if (slice == nullptr || check_pose(pose7) != DLIOM_OK) return DLIOM_ERR_INVALID_ARGUMENT;
  std::memcpy(slice->d.pose7, pose7, sizeof slice->d.pose7);
  return DLIOM_OK;
}

int dliom_submap_slice_info(const dliom_submap_slice* slice, dliom_submap_slice_description* out) {
  if (slice == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = slice->d;
  return DLIOM_OK;
}

int dliom_submap_slice_destroy(dliom_submap_slice* slice) {
  if (slice == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  if (slice->d_cells != nullptr) (void)hipFree(slice->d_cells);
  delete slice;
  return DLIOM_OK;
}

int dliom_submap_slices_layout(const dliom_submap_slice_description* slices, int64_t n, double resolution, int32_t* width,
                               int32_t* height, float origin2f[2], int64_t* fixed6) {
  if (width == nullptr || height == nullptr || origin2f == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  painter::Layout L;
  const int status = painter::layout(slices, n, resolution, &L);
  if (status != DLIOM_OK && status != DLIOM_ERR_CAPACITY) return status;
  *width = L.width;
  *height = L.height;
  origin2f[0] = L.origin[0];
  origin2f[1] = L.origin[1];
  if (status != DLIOM_OK) return status;
  std::vector<painter::Fixed> fixed(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i)
    DLIOM_TRY(painter::invert(L.matrices[static_cast<size_t>(i)], L.origin, L.width, L.height, &fixed[static_cast<size_t>(i)]));
  if (fixed6 != nullptr) {
    for (int64_t i = 0; i < n; ++i) {
      const painter::Fixed& f = fixed[static_cast<size_t>(i)];
      const int64_t v[6] = {f.A, f.B, f.E, f.C, f.D, f.G};
      std::memcpy(fixed6 + 6 * i, v, sizeof v);
    }
  }
  return DLIOM_OK;
}

int dliom_submap_occupancy_table(int8_t table256[256]) {
  if (table256 == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  painter::occupancy_table(table256);
  return DLIOM_OK;
}

int dliom_submap_slices_paint(dliom_ctx* ctx, const dliom_submap_slice* const* slices, int64_t n, double resolution,
                              uint32_t* pixels, int64_t capacity, int32_t* width, int32_t* height, float origin2f[2]) {
  if (origin2f == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  return paint(ctx, slices, n, resolution, pixels, nullptr, capacity, width, height, origin2f, nullptr, false);
}

int dliom_submap_slices_occupancy(dliom_ctx* ctx, const dliom_submap_slice* const* slices, int64_t n, double resolution,
                                  int8_t* data, int64_t capacity, int32_t* width, int32_t* height, float origin2f[2],
                                  double origin_xy[2]) {
  if (origin_xy == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  return paint(ctx, slices, n, resolution, nullptr, data, capacity, width, height, origin2f, origin_xy, true);
}

int dliom_ctx_submap_painter_stats(const dliom_ctx* ctx, dliom_submap_painter_stats* out) {
  if (ctx == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  out->launches = ctx->painter_launches;
  out->texels_uploaded = ctx->painter_texels_uploaded;
  out->tile_slice_pairs = ctx->painter_pairs;
  return DLIOM_OK;
}

}  // extern "C"
