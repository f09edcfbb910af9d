// X-ray projections of a device HybridGrid: the SubmapQuery texture (Submap3D::ToResponseProto ->
// AddToTextureProto, mapping/3d/submap_3d.cc:53-177, 253-262) and D-LIOM's loop-detection image
// (ProjectToCvMat, submap_3d.cc:381-443), byte for byte (DESIGN.md "X-ray projections").
//
// Both walk the grid in HybridGrid::Iterator order, keep the cells with ValueToProbability(v) >= 0.501,
// transform each cell centre, round it to a pixel and accumulate per pixel a count, min / max z, a float
// probability sum (in iterator order) and a maximum.  Only the float sum depends on the order.  Here:
//   1. xray_slot_key_kernel + radix sort: the used leaves in iterator order (grid_proto.cc's key: 64^3 meta
//      cells z-major, leaves z-major inside a meta cell; cells inside a leaf are z-major in the pool already).
//   2. xray_bound_kernel: one workgroup per leaf (sorted order): occupied count and the xy bounding box of
//      the rounded indices (integer atomics, order-free).  Inclusive scan of the counts.  ONE read-back:
//      the total and the box, which size the image.
//   3. xray_emit_kernel: the same leaves again, the occupied cells compacted in iterator order with their
//      pixel as key and (z, value) as payload; a stable radix sort by pixel keeps iterator order inside
//      every pixel.
//   4. xray_texture_kernel / xray_image_kernel: one thread per pixel, a sequential sum over its run.
// No float atomics anywhere, so every call gives the same bytes.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "device_common.h"
#include "host_math.h"
#include "probability_values.h"

namespace dliom {
namespace {

constexpr float kObstructedLimit = 0.501f;  // kXrayObstructedCellProbabilityLimit, submap_3d.cc:88, 405
constexpr int kNumLogOddsSteps = 254;       // ProbabilityToLogOddsInteger steps up 254 times from 1 to 255

// mapping/submaps.h:37-52 with glibc's logf, evaluated at run time (std::log(float) -> logf).
float host_logit(float p) { return std::log(p / (1.f - p)); }
int log_odds_formula(float p, float min_log_odds, float max_log_odds) {
  return static_cast<int>(std::lround((host_logit(p) - min_log_odds) * 254.f / (max_log_odds - min_log_odds))) + 1;
}
uint32_t float_bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}
float bits_float(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

// The device has no glibc logf.  ProbabilityToLogOddsInteger is monotone over [0.1, 0.9] (tests/test_xray_host.py
// checks every float there), so it is 1 + the number of step points <= p: step[k] is the smallest float whose result
// is >= k + 2, found by bisection over the (order-preserving) bit patterns of positive floats.  Built once, at load.
struct LogOddsSteps {
  float step[kNumLogOddsSteps];
  LogOddsSteps() {
    volatile float lo_p = kMinProbability, hi_p = kMaxProbability;  // glibc at run time, like the reference's statics
    const float min_lo = host_logit(lo_p), max_lo = host_logit(hi_p);
    for (int k = 0; k < kNumLogOddsSteps; ++k) {
      uint32_t lo = float_bits(kMinProbability), hi = float_bits(kMaxProbability);
      while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (log_odds_formula(bits_float(mid), min_lo, max_lo) >= k + 2) hi = mid;
        else lo = mid + 1;
      }
      step[k] = bits_float(lo);
    }
  }
};
const LogOddsSteps kLogOddsSteps;

__host__ __device__ inline int log_odds_from_steps(const float* step, float p) {
  int lo = 0, hi = kNumLogOddsSteps;  // first step > p
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (step[mid] <= p) lo = mid + 1;
    else hi = mid;
  }
  return 1 + lo;
}

__device__ __forceinline__ float value_to_probability(unsigned v, float scale, float offset) {
  v &= 0x7FFFu;  // the reference's table repeats above the update marker
  return v == 0u ? kMinProbability : static_cast<float>(static_cast<int>(v)) * scale + offset;
}

// the transform applied to a cell centre, as float (Rigid3f * Vector3f = rotation * v + translation)
struct XrayTransform {
  Quat4 q;
  float t[3];
  float resolution;      // GetCenterOfCell: index.cast<float>() * resolution
  float inv_resolution;  // resolution_inverse (texture: 1.f / res; image: float(1.0 / double(res)))
  unsigned threshold;    // smallest value with ValueToProbability >= 0.501
};

__device__ __forceinline__ void xray_pixel(const XrayTransform& T, int ix, int iy, int iz, int* px, int* py, int* pz) {
  float x, y, z;
  rotate_point(T.q, static_cast<float>(ix) * T.resolution, static_cast<float>(iy) * T.resolution,
               static_cast<float>(iz) * T.resolution, x, y, z);
  x = x + T.t[0];
  y = y + T.t[1];
  z = z + T.t[2];
  *px = lround_away(x * T.inv_resolution);
  *py = lround_away(y * T.inv_resolution);
  *pz = lround_away(z * T.inv_resolution);
}

__device__ __forceinline__ int floor_div64(int a) { return a >= 0 ? a / 64 : (a - 63) / 64; }

// the iterator's leaf order (grid_proto.cc): |cell| <= 8192 -> 10 biased bits per meta coordinate, 3 per leaf coordinate
__global__ void xray_slot_key_kernel(const int32_t* slot_coord, const uint32_t* d_count, int n, uint64_t* keys, uint32_t* ids) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned slot = static_cast<unsigned>(i) + 1u;
  uint64_t key = ~uint64_t{0};  // slots past the count hold no cells: last
  if (slot < *d_count) {
    const int o[3] = {slot_coord[3 * slot] * 8, slot_coord[3 * slot + 1] * 8, slot_coord[3 * slot + 2] * 8};
    const int mx = floor_div64(o[0]), my = floor_div64(o[1]), mz = floor_div64(o[2]);
    const int lx = (o[0] - 64 * mx) >> 3, ly = (o[1] - 64 * my) >> 3, lz = (o[2] - 64 * mz) >> 3;
    key = (static_cast<uint64_t>(mz + 512) << 29) | (static_cast<uint64_t>(my + 512) << 19) |
          (static_cast<uint64_t>(mx + 512) << 9) | (static_cast<uint64_t>(lz) << 6) | (static_cast<uint64_t>(ly) << 3) |
          static_cast<uint64_t>(lx);
  }
  keys[i] = key;
  ids[i] = slot;
}

constexpr int kLeafThreads = 512;  // one thread per cell of a leaf, 8 waves

// bbox: [min x, -max x, min y, -max y], all four kept as minima
__global__ __launch_bounds__(kLeafThreads) void xray_bound_kernel(const uint16_t* pool, const int32_t* slot_coord,
                                                                  const uint32_t* d_count, const uint32_t* ids,
                                                                  XrayTransform T, uint32_t* counts, int* bbox) {
  __shared__ unsigned wave_count[kLeafThreads / 64];
  __shared__ int wave_box[kLeafThreads / 64][4];
  const unsigned slot = ids[blockIdx.x];
  const int c = threadIdx.x, lane = c & 63, w = c >> 6;
  bool occ = false;
  int px = 0, py = 0, pz = 0;
  if (slot < *d_count) {
    const unsigned v = pool[static_cast<size_t>(slot) * 512u + c];
    occ = (v & 0x7FFFu) >= T.threshold;
    if (occ) {
      xray_pixel(T, slot_coord[3 * slot] * 8 + (c & 7), slot_coord[3 * slot + 1] * 8 + ((c >> 3) & 7),
                 slot_coord[3 * slot + 2] * 8 + (c >> 6), &px, &py, &pz);
    }
  }
  int b[4] = {occ ? px : INT_MAX, occ ? -px : INT_MAX, occ ? py : INT_MAX, occ ? -py : INT_MAX};  // all as minima
  for (int k = 0; k < 4; ++k) {
    // -INT_MIN does not occur: |px| < 2^31 - 1 after lround of a float below 2^31 (larger ones saturate, flagged by size)
    for (int m = 32; m >= 1; m >>= 1) b[k] = min(b[k], __shfl_xor(b[k], m, 64));
  }
  const unsigned long long ballot = __ballot(occ);
  if (lane == 0) {
    wave_count[w] = static_cast<unsigned>(__popcll(ballot));
    for (int k = 0; k < 4; ++k) wave_box[w][k] = b[k];
  }
  __syncthreads();
  if (c == 0) {
    unsigned n = 0;
    int r[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    for (int i = 0; i < kLeafThreads / 64; ++i) {
      n += wave_count[i];
      for (int k = 0; k < 4; ++k) r[k] = min(r[k], wave_box[i][k]);
    }
    counts[blockIdx.x] = n;
    if (n > 0)
      for (int k = 0; k < 4; ++k) atomicMin(&bbox[k], r[k]);
  }
}

// pixel of a cell: texture (max_x - px) * width + (max_y - py) (submap_3d.cc:66-68);
// image (py - min_y) * width + (px - min_x) (submap_3d.cc:436-438)
struct PixelMap {
  int texture;  // 1: texture layout, 0: image layout
  int min_x, max_x, min_y, max_y;
  int width;
};

__global__ __launch_bounds__(kLeafThreads) void xray_emit_kernel(const uint16_t* pool, const int32_t* slot_coord,
                                                                 const uint32_t* d_count, const uint32_t* ids,
                                                                 const uint32_t* counts, const uint32_t* inclusive,
                                                                 XrayTransform T, PixelMap M, uint32_t* keys,
                                                                 uint64_t* payload) {
  __shared__ unsigned wave_count[kLeafThreads / 64];
  const unsigned slot = ids[blockIdx.x];
  const int c = threadIdx.x, lane = c & 63, w = c >> 6;
  unsigned v = 0;
  bool occ = false;
  if (slot < *d_count) {
    v = pool[static_cast<size_t>(slot) * 512u + c];
    occ = (v & 0x7FFFu) >= T.threshold;
  }
  const unsigned long long ballot = __ballot(occ);
  if (lane == 0) wave_count[w] = static_cast<unsigned>(__popcll(ballot));
  __syncthreads();
  if (!occ) return;
  unsigned pos = inclusive[blockIdx.x] - counts[blockIdx.x];
  for (int i = 0; i < w; ++i) pos += wave_count[i];
  pos += static_cast<unsigned>(__popcll(ballot & ((1ull << lane) - 1ull)));
  int px, py, pz;
  xray_pixel(T, slot_coord[3 * slot] * 8 + (c & 7), slot_coord[3 * slot + 1] * 8 + ((c >> 3) & 7),
             slot_coord[3 * slot + 2] * 8 + (c >> 6), &px, &py, &pz);
  const int pixel = M.texture ? (M.max_x - px) * M.width + (M.max_y - py) : (py - M.min_y) * M.width + (px - M.min_x);
  keys[pos] = static_cast<uint32_t>(pixel);
  payload[pos] = (static_cast<uint64_t>(static_cast<uint32_t>(pz)) << 32) | v;
}

struct PixelArgs {
  const uint32_t* keys;     // sorted pixels of the occupied cells
  const uint64_t* payload;  // (z << 32 | value), iterator order inside a pixel
  int n;                    // occupied cells
  int64_t pixels;
  float scale, offset;      // ValueToProbability: v * scale + offset
  const float* steps;       // LogOddsSteps::step
  uint8_t* out;
};

__device__ __forceinline__ int first_at_or_above(const uint32_t* keys, int n, uint32_t p) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// AccumulatePixelData + ComputePixelValues (submap_3d.cc:53-78, 116-145): interleaved (value, alpha)
__global__ void xray_texture_kernel(PixelArgs a) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= a.pixels) return;
  int count = 0, min_z = INT_MAX, max_z = INT_MIN;
  float sum = 0.f, max_probability = 0.5f;
  for (int i = first_at_or_above(a.keys, a.n, static_cast<uint32_t>(p)); i < a.n && a.keys[i] == static_cast<uint32_t>(p); ++i) {
    const uint64_t e = a.payload[i];
    const int z = static_cast<int>(static_cast<uint32_t>(e >> 32));
    const float probability = value_to_probability(static_cast<unsigned>(e & 0xFFFFu), a.scale, a.offset);
    ++count;
    min_z = min(min_z, z);
    max_z = max(max_z, z);
    sum = sum + probability;
    max_probability = max_probability < probability ? probability : max_probability;  // std::max
  }
  uint8_t value = 0, alpha = 0;
  const float z_difference = count > 0 ? static_cast<float>(max_z - min_z) : 0.f;
  if (!(z_difference < 3.f)) {  // kMinZDifference
    const float free_minus_count = z_difference - static_cast<float>(count);
    const float free_space = free_minus_count < 0.f ? 0.f : free_minus_count;  // std::max(.., 0.f)
    const float free_space_weight = 0.15f * free_space;  // kFreeSpaceWeight
    const float total_weight = static_cast<float>(count) + free_space_weight;
    const float free_space_probability = 1.f - max_probability;
    float average = (sum + free_space_probability * free_space_weight) / total_weight;
    average = average > kMaxProbability ? kMaxProbability : (average < kMinProbability ? kMinProbability : average);
    const int delta = 128 - log_odds_from_steps(a.steps, average);
    alpha = static_cast<uint8_t>(delta > 0 ? 0 : -delta);
    value = static_cast<uint8_t>(delta > 0 ? delta : 0);
    if (value == 0 && alpha == 0) alpha = 1;
  }
  a.out[2 * p] = value;
  a.out[2 * p + 1] = alpha;
}

// submap_3d.cc:427-452, 455-461: RoundToInt((sum - kMinProbability) * (255 / 0.8)) stored into a uchar (modulo 256)
__global__ void xray_image_kernel(PixelArgs a, float gain) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= a.pixels) return;
  float sum = 0.f;
  for (int i = first_at_or_above(a.keys, a.n, static_cast<uint32_t>(p)); i < a.n && a.keys[i] == static_cast<uint32_t>(p); ++i)
    sum = sum + value_to_probability(static_cast<unsigned>(a.payload[i] & 0xFFFFu), a.scale, a.offset);
  a.out[p] = static_cast<uint8_t>(static_cast<unsigned>(lround_away((sum - kMinProbability) * gain)));
}


unsigned obstructed_threshold() {
  for (int v = 1; v < 32768; ++v)
    if (!(dliom::value_to_probability(v) < kObstructedLimit)) return static_cast<unsigned>(v);
  return 32768u;
}

struct XrayResult {
  int64_t width = 0, height = 0;
  int min_x = 0, max_x = 0, min_y = 0, max_y = 0;
};

// Runs the projection; out == nullptr or capacity too small: sizes only.  2 bytes per pixel (texture) or 1 (image).
// device_out != nullptr: the picture stays in HBM (ctx->xray_cells, valid until the next projection on the context);
// out and capacity are then not used and nothing is copied or waited for after the kernels.
int run_xray(const dliom_grid* g, const XrayTransform& T, bool texture, uint8_t* out, int64_t capacity, XrayResult* r,
             const uint8_t** device_out = nullptr) {
  dliom_ctx* ctx = g->ctx;
  const int64_t S = std::min<int64_t>(g->used_upper, g->capacity) - 1;  // candidate slots 1 .. S; the count is on the device
  if (S <= 0 || g->d_pool == nullptr) return DLIOM_OK;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int bpp = texture ? 2 : 1;

  // ---- phase 1: leaf order, counts, bounding box -----------------------------------------------------------------
  size_t sort_bytes = 0, scan_bytes = 0;
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, static_cast<const uint64_t*>(nullptr),
                                                   static_cast<uint64_t*>(nullptr), static_cast<const uint32_t*>(nullptr),
                                                   static_cast<uint32_t*>(nullptr), static_cast<int>(S), 0, 40, st));
  DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, static_cast<const uint32_t*>(nullptr),
                                                 static_cast<uint32_t*>(nullptr), static_cast<int>(S), st));
  const size_t off_keys_out = align256(8 * S), off_ids = off_keys_out + align256(8 * S), off_ids_out = off_ids + align256(4 * S),
               off_counts = off_ids_out + align256(4 * S), off_incl = off_counts + align256(4 * S),
               off_box = off_incl + align256(4 * S), off_tmp = off_box + 256,
               total1 = off_tmp + align256(std::max(sort_bytes, scan_bytes));
  DLIOM_TRY(ctx->xray_leaves.reserve(total1));
  char* b1 = static_cast<char*>(ctx->xray_leaves.p);
  uint64_t* keys = reinterpret_cast<uint64_t*>(b1);
  uint64_t* keys_out = reinterpret_cast<uint64_t*>(b1 + off_keys_out);
  uint32_t* ids = reinterpret_cast<uint32_t*>(b1 + off_ids);
  uint32_t* ids_out = reinterpret_cast<uint32_t*>(b1 + off_ids_out);
  uint32_t* counts = reinterpret_cast<uint32_t*>(b1 + off_counts);
  uint32_t* incl = reinterpret_cast<uint32_t*>(b1 + off_incl);
  int* box = reinterpret_cast<int*>(b1 + off_box);
  const FillJob fill{box, 16, static_cast<unsigned>(INT_MAX)};
  DLIOM_TRY(fill_multi(ctx, &fill, 1));
  hipLaunchKernelGGL(xray_slot_key_kernel, dim3(blocks_of(S, 256)), dim3(256), 0, st, g->d_slot_coord, g->d_count,
                     static_cast<int>(S), keys, ids);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(b1 + off_tmp, sort_bytes, keys, keys_out, ids, ids_out,
                                                   static_cast<int>(S), 0, 40, st));
  hipLaunchKernelGGL(xray_bound_kernel, dim3(static_cast<unsigned>(S)), dim3(kLeafThreads), 0, st, g->d_pool,
                     g->d_slot_coord, g->d_count, ids_out, T, counts, box);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(b1 + off_tmp, scan_bytes, counts, incl, static_cast<int>(S), st));
  const GatherJob back[2] = {{incl + (S - 1), 1}, {box, 4}};
  int* host = pinned_at<int>(ctx, kPinReadback);
  DLIOM_TRY(gather_and_wait(ctx, back, 2, host));
  const int64_t n = static_cast<uint32_t>(host[0]);
  if (n == 0) return DLIOM_OK;  // nothing at or above 0.501: 0 x 0 (the reference's box would overflow)
  r->min_x = host[1];
  r->max_x = -host[2];
  r->min_y = host[3];
  r->max_y = -host[4];
  const int64_t sx = static_cast<int64_t>(r->max_x) - r->min_x + 1, sy = static_cast<int64_t>(r->max_y) - r->min_y + 1;
  r->width = texture ? sy : sx;
  r->height = texture ? sx : sy;
  const int64_t pixels = sx * sy;
  if (pixels > DLIOM_XRAY_MAX_PIXELS) return DLIOM_ERR_CAPACITY;
  if (device_out == nullptr) {
    if (out == nullptr) return DLIOM_OK;
    if (capacity < bpp * pixels) return DLIOM_ERR_CAPACITY;
  }

  // ---- phase 2: occupied cells in iterator order, stable sort by pixel, one thread per pixel -----------------------
  int end_bit = 1;
  while (end_bit < 32 && (int64_t{1} << end_bit) < pixels) ++end_bit;
  size_t sort2_bytes = 0;
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort2_bytes, static_cast<const uint32_t*>(nullptr),
                                                   static_cast<uint32_t*>(nullptr), static_cast<const uint64_t*>(nullptr),
                                                   static_cast<uint64_t*>(nullptr), static_cast<int>(n), 0, end_bit, st));
  const size_t o_keys_out = align256(4 * n), o_pay = o_keys_out + align256(4 * n), o_pay_out = o_pay + align256(8 * n),
               o_steps = o_pay_out + align256(8 * n), o_img = o_steps + align256(4 * kNumLogOddsSteps),
               o_tmp = o_img + align256(bpp * pixels), total2 = o_tmp + align256(sort2_bytes);
  DLIOM_TRY(ctx->xray_cells.reserve(total2));
  char* b2 = static_cast<char*>(ctx->xray_cells.p);
  uint32_t* pk = reinterpret_cast<uint32_t*>(b2);
  uint32_t* pk_out = reinterpret_cast<uint32_t*>(b2 + o_keys_out);
  uint64_t* pay = reinterpret_cast<uint64_t*>(b2 + o_pay);
  uint64_t* pay_out = reinterpret_cast<uint64_t*>(b2 + o_pay_out);
  float* steps = reinterpret_cast<float*>(b2 + o_steps);
  uint8_t* img = reinterpret_cast<uint8_t*>(b2 + o_img);
  DLIOM_HIP_TRY(hipMemcpyAsync(steps, kLogOddsSteps.step, sizeof(kLogOddsSteps.step), hipMemcpyHostToDevice, st));
  PixelMap M{texture ? 1 : 0, r->min_x, r->max_x, r->min_y, r->max_y, static_cast<int>(r->width)};
  hipLaunchKernelGGL(xray_emit_kernel, dim3(static_cast<unsigned>(S)), dim3(kLeafThreads), 0, st, g->d_pool,
                     g->d_slot_coord, g->d_count, ids_out, counts, incl, T, M, pk, pay);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(b2 + o_tmp, sort2_bytes, pk, pk_out, pay, pay_out, static_cast<int>(n), 0,
                                                   end_bit, st));
  PixelArgs a{pk_out, pay_out, static_cast<int>(n), pixels, kValueToProbabilityScale, kValueToProbabilityOffset, steps, img};
  if (texture) {
    hipLaunchKernelGGL(xray_texture_kernel, dim3(blocks_of(pixels, 256)), dim3(256), 0, st, a);
  } else {
    const float gain = 255.f / (kMaxProbability - kMinProbability);
    hipLaunchKernelGGL(xray_image_kernel, dim3(blocks_of(pixels, 256)), dim3(256), 0, st, a, gain);
  }
  DLIOM_HIP_TRY(hipGetLastError());
  if (device_out != nullptr) {
    *device_out = img;
    return DLIOM_OK;
  }
  DLIOM_HIP_TRY(hipMemcpyAsync(out, img, static_cast<size_t>(bpp * pixels), hipMemcpyDeviceToHost, st));
  DLIOM_HIP_TRY(hipStreamSynchronize(st));
  ++ctx->host_syncs;
  return DLIOM_OK;
}

PoseD pose_from7(const double* p) {
  PoseD r;
  for (int i = 0; i < 3; ++i) r.t[i] = p[i];
  for (int i = 0; i < 4; ++i) r.q[i] = p[3 + i];
  return r;
}

// ProjectToCvMat (submap_3d.cc:391-463) behind dliom_grid_project_to_image; device_image != nullptr: see run_xray
int project_to_image(const dliom_grid* grid, const double transform7[7], uint8_t* image, int64_t capacity,
                     const uint8_t** device_image, int32_t* width, int32_t* height, double* ox, double* oy, double* resolution) {
  const PoseD g = pose_from7(transform7);
  // yaw = GetYaw(transform) (transform.h:43-52): atan2 of the rotated unit x, in double
  const double ux[3] = {1.0, 0.0, 0.0};
  double dir[3];
  qrot_d(g.q, ux, dir);
  const double yaw = std::atan2(dir[1], dir[0]);
  // Embed3D(Rigid2d::Rotation(-yaw)) (transform.h:110-115): AngleAxisd(-yaw, UnitZ) -> quaternion, then cast<float>
  const double ha = 0.5 * -yaw, sh = std::sin(ha);
  const QF yaw_q{static_cast<float>(std::cos(ha)), static_cast<float>(sh * 0.0), static_cast<float>(sh * 0.0),
                 static_cast<float>(sh * 1.0)};
  // Rigid3d::Rotation(transform.rotation()).cast<float>(), composed: Rigid3f product (rigid_transform.h:206-212)
  const QF rot_q{static_cast<float>(g.q[0]), static_cast<float>(g.q[1]), static_cast<float>(g.q[2]), static_cast<float>(g.q[3])};
  const QF q = qnormalized(qmul(yaw_q, rot_q));
  const F3 t = add3(qrot(yaw_q, F3{0.f, 0.f, 0.f}), F3{0.f, 0.f, 0.f});
  XrayTransform T;
  T.q = Quat4{q.w, q.x, q.y, q.z};
  T.t[0] = t.x;
  T.t[1] = t.y;
  T.t[2] = t.z;
  const double res = grid->resolution;  // `double& resolution` in ProjectToCvMat
  T.resolution = grid->resolution;
  T.inv_resolution = static_cast<float>(1.f / res);  // double division, stored to float (submap_3d.cc:399)
  T.threshold = obstructed_threshold();
  XrayResult r;
  const int s = run_xray(grid, T, false, image, capacity, &r, device_image);
  *width = static_cast<int32_t>(r.width);
  *height = static_cast<int32_t>(r.height);
  *resolution = res;
  *ox = r.min_x * res;  // int * double (submap_3d.cc:422-423)
  *oy = r.min_y * res;
  return s;
}

// AddToTextureProto (submap_3d.cc:53-177) behind dliom_grid_xray_texture; device_cells != nullptr: see run_xray
int xray_texture(const dliom_grid* grid, const double global_submap_pose7[7], uint8_t* cells, int64_t capacity,
                 const uint8_t** device_cells, int32_t* width, int32_t* height, double* resolution, double slice_pose7[7]) {
  const PoseD g = pose_from7(global_submap_pose7);
  XrayTransform T;
  T.q = Quat4{static_cast<float>(g.q[0]), static_cast<float>(g.q[1]), static_cast<float>(g.q[2]), static_cast<float>(g.q[3])};
  for (int i = 0; i < 3; ++i) T.t[i] = static_cast<float>(g.t[i]);  // global_submap_pose.cast<float>()
  T.resolution = grid->resolution;
  T.inv_resolution = 1.f / grid->resolution;  // submap_3d.cc:85
  T.threshold = obstructed_threshold();
  XrayResult r;
  const int s = run_xray(grid, T, true, cells, capacity, &r, device_cells);
  *width = static_cast<int32_t>(r.width);
  *height = static_cast<int32_t>(r.height);
  *resolution = grid->resolution;
  // global_submap_pose.inverse() * Translation(max_x * res, max_y * res, t.z): float products widened (submap_3d.cc:173-176)
  PoseD slice;
  slice.t[0] = static_cast<double>(static_cast<float>(r.max_x) * grid->resolution);
  slice.t[1] = static_cast<double>(static_cast<float>(r.max_y) * grid->resolution);
  slice.t[2] = g.t[2];
  slice.q[0] = 1.0;
  slice.q[1] = slice.q[2] = slice.q[3] = 0.0;
  const PoseD sp = pose_mul(pose_inverse(g), slice);
  for (int i = 0; i < 3; ++i) slice_pose7[i] = sp.t[i];
  for (int i = 0; i < 4; ++i) slice_pose7[3 + i] = sp.q[i];
  return s;
}

}  // namespace

int xray_texture_on_device(const dliom_grid* grid, const double global_submap_pose7[7], const uint8_t** cells, int32_t* width,
                           int32_t* height, double* resolution, double slice_pose7[7]) {
  *cells = nullptr;  // stays so under an empty projection
  return xray_texture(grid, global_submap_pose7, nullptr, 0, cells, width, height, resolution, slice_pose7);
}

int project_to_image_on_device(const dliom_grid* grid, const double transform7[7], const uint8_t** image, int32_t* width,
                               int32_t* height, double* ox, double* oy, double* resolution) {
  *image = nullptr;  // stays so under an empty projection
  return project_to_image(grid, transform7, nullptr, 0, image, width, height, ox, oy, resolution);
}

}  // namespace dliom

using namespace dliom;

extern "C" {

uint8_t dliom_probability_to_log_odds_integer(float probability) {
  return static_cast<uint8_t>(log_odds_from_steps(kLogOddsSteps.step, probability));
}

int dliom_grid_xray_texture(const dliom_grid* grid, const double global_submap_pose7[7], uint8_t* cells, int64_t capacity,
                            int32_t* width, int32_t* height, double* resolution, double slice_pose7[7]) {
  if (grid == nullptr || global_submap_pose7 == nullptr || width == nullptr || height == nullptr || resolution == nullptr ||
      slice_pose7 == nullptr || capacity < 0)
    return DLIOM_ERR_INVALID_ARGUMENT;
  return xray_texture(grid, global_submap_pose7, cells, capacity, nullptr, width, height, resolution, slice_pose7);
}

int dliom_grid_xray_texture_gzip(const dliom_grid* grid, const double global_submap_pose7[7], uint8_t* cells_gz, int64_t capacity,
                                 int64_t* cells_gz_size, int32_t* width, int32_t* height, double* resolution, double slice_pose7[7],
                                 dliom_gzip_stats* gzip_stats) {
  if (grid == nullptr || global_submap_pose7 == nullptr || cells_gz_size == nullptr || width == nullptr || height == nullptr ||
      resolution == nullptr || slice_pose7 == nullptr || capacity < 0)
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (gzip_stats != nullptr) *gzip_stats = dliom_gzip_stats{0, 0, 0, 0};
  if (cells_gz == nullptr) {
    DLIOM_TRY(xray_texture(grid, global_submap_pose7, nullptr, 0, nullptr, width, height, resolution, slice_pose7));
    *cells_gz_size = dliom_gzip_bound(int64_t{2} * *width * *height);
    return DLIOM_OK;
  }
  const uint8_t* cells = nullptr;
  DLIOM_TRY(xray_texture(grid, global_submap_pose7, nullptr, 0, &cells, width, height, resolution, slice_pose7));
  const int64_t offsets[2] = {0, int64_t{2} * *width * *height};
  int64_t out_offsets[2] = {0, 0};
  DLIOM_HIP_TRY(hipSetDevice(grid->ctx->device));  // (an empty grid's projection returns before it touches the device)
  const int st = gzip_on_device(grid->ctx, cells, offsets, 1, false, cells_gz, capacity, out_offsets, gzip_stats);
  if (st == DLIOM_OK || st == DLIOM_ERR_CAPACITY) *cells_gz_size = out_offsets[1];
  return st;
}

int dliom_grid_project_to_image(const dliom_grid* grid, const double transform7[7], uint8_t* image, int64_t capacity,
                                int32_t* width, int32_t* height, double* ox, double* oy, double* resolution) {
  if (grid == nullptr || transform7 == nullptr || width == nullptr || height == nullptr || ox == nullptr || oy == nullptr ||
      resolution == nullptr || capacity < 0)
    return DLIOM_ERR_INVALID_ARGUMENT;
  return project_to_image(grid, transform7, image, capacity, nullptr, width, height, ox, oy, resolution);
}

}  // extern "C"
