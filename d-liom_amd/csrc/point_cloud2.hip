// PointCloud2 messages decoded on the device (dliom.h "PointCloud2 messages decoded on the device", DESIGN.md section
// 3.20): SensorBridge::HandlePointCloud2Message's four branches with HandleRangefinder's change of frame
// (cartographer_ros/sensor_bridge.cc:176-240, 286-299) and the export's ToPointCloudWithIntensities[RsLiDAR]
// (msg_conversion.cc:185-226), one pass over the message's bytes.
//
// Records are not aligned (Velodyne: 22 bytes, the float `time` at offset 18; Robosense: a double in a 32-byte record), so
// no typed pointer ever points into the message.  A workgroup of 256 points copies its byte span into LDS with aligned
// 16-byte loads -- one span a row it touches, broken at row ends when row_step pads the rows -- and every field is put
// together from two aligned LDS words.  Records too long for that (decode_fits_lds) take the same words from global memory.
// The kept points keep the message's order through compact.hip's keep flags and scan; the call's ONE read-back brings the
// kept count, the bad-time flag and the first and last kept t.
#include <cmath>
#include <cstring>

#include "device_common.h"
#include "point_cloud2_layout.h"
#include "timed_cloud.h"

namespace dliom {
namespace {

constexpr int kBlock = 256;
constexpr unsigned kLdsBytes = 48 * 1024;  // the span of 256 records, its alignment slack and the word behind
enum { kWordBadTime = 0, kWordFront = 1, kWordBack = 2, kWords = 4 };

struct FrameChange {
  int given;
  Quat4 q;
  float t[3];
};

// the 32 bits at byte `at` of a word array: two aligned words, funnel-shifted (the word behind the last one is read and
// shifted out: both sources keep it readable)
template <class Words>
__device__ __forceinline__ uint32_t bits32(const Words* w, uint32_t at) {
  const uint32_t i = at >> 2, shift = (at & 3u) * 8u;
  const uint64_t pair = (static_cast<uint64_t>(w[i + 1]) << 32) | w[i];
  return static_cast<uint32_t>(pair >> shift);
}

// One record at byte `at` of `w`: the point in its output frame, t and the intensity.  Returns the keep flag; *bad_time: a
// kept point whose t the assembler would refuse.
template <class Words>
__device__ __forceinline__ unsigned decode_record(const PointCloud2Plan& p, const FrameChange& fc, const Words* w, uint32_t at,
                                                  float4* out, float* intensity, bool* bad_time) {
  const float x = __uint_as_float(bits32(w, at + p.off_x));
  const float y = __uint_as_float(bits32(w, at + p.off_y));
  const float z = __uint_as_float(bits32(w, at + p.off_z));
  float t = 0.f;
  if (p.time_kind == kPc2TimeUint32Ns) {
    // point.t * 1e-9f - rel_time_last: uint32 -> float to nearest, a float product, then double
    const float seconds = __fmul_rn(__uint2float_rn(bits32(w, at + p.off_time)), 1e-9f);
    t = __double2float_rn(__dsub_rn(static_cast<double>(seconds), p.rel_time_last));
  } else if (p.time_kind == kPc2TimeFloat32) {
    t = __double2float_rn(__dsub_rn(static_cast<double>(__uint_as_float(bits32(w, at + p.off_time))), p.rel_time_last));
  } else if (p.time_kind == kPc2TimeFloat64) {
    const uint64_t bits = (static_cast<uint64_t>(bits32(w, at + p.off_time + 4)) << 32) | bits32(w, at + p.off_time);
    t = __double2float_rn(__dsub_rn(__longlong_as_double(static_cast<long long>(bits)), p.rel_time_last));
  }
  if (p.intensity_kind == kPc2IntensityFloat32) *intensity = __uint_as_float(bits32(w, at + p.off_intensity));
  else if (p.intensity_kind == kPc2IntensityUint8) *intensity = static_cast<float>(bits32(w, at + p.off_intensity) & 0xFFu);
  else *intensity = 1.0f;
  const bool finite = fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;  // (false for NaN)
  const bool keep = p.drop_non_finite == 0 || finite;
  *bad_time = keep && !(fabs(static_cast<double>(t) * 1e7) < 9223372036854775808.0);
  float ox = x, oy = y, oz = z;
  if (fc.given != 0) {  // sensor_to_tracking.cast<float>() * p
    rotate_point(fc.q, x, y, z, ox, oy, oz);
    ox = ox + fc.t[0];
    oy = oy + fc.t[1];
    oz = oz + fc.t[2];
  }
  *out = make_float4(ox, oy, oz, t);
  return keep ? 1u : 0u;
}

__device__ __forceinline__ void store_record(const PointCloud2Plan& p, uint32_t i, unsigned keep, const float4& v, float intensity,
                                             bool bad_time, float4* __restrict__ xyzt, float* __restrict__ intensities,
                                             unsigned* __restrict__ keep_flags, unsigned* __restrict__ words) {
  xyzt[i] = v;
  if (p.intensity_kind != kPc2IntensityNone) intensities[i] = intensity;
  keep_flags[i] = keep;
  if (bad_time) atomicOr(&words[kWordBadTime], 1u);
}

// 256 points a workgroup, through LDS.  data: the message's bytes, 16-byte aligned, readable up to used_bytes rounded up
// to 16.  The workgroup's points lie in one span a row: rows [first / width, last / width].
__global__ __launch_bounds__(kBlock) void decode_lds_kernel(PointCloud2Plan p, FrameChange fc, const uint4* __restrict__ data,
                                                            float4* __restrict__ xyzt, float* __restrict__ intensities,
                                                            unsigned* __restrict__ keep_flags, unsigned* __restrict__ words) {
  extern __shared__ uint4 span[];
  const uint32_t first = blockIdx.x * kBlock;
  const uint32_t count = min(static_cast<uint32_t>(kBlock), p.n - first);
  const uint32_t mine = first + threadIdx.x;
  uint32_t my_at = 0, done = 0, units = 0;  // units: 16-byte units of LDS filled so far
  while (done < count) {
    const uint32_t row = (first + done) / p.width, col = (first + done) % p.width;
    const uint32_t seg = min(p.width - col, count - done);  // this row's points of the workgroup
    const uint64_t g = static_cast<uint64_t>(row) * p.row_step + static_cast<uint64_t>(col) * p.point_step;
    const uint32_t lead = static_cast<uint32_t>(g & 15u);
    const uint32_t seg_units = (lead + seg * p.point_step + 15u) >> 4;
    const uint4* src = data + (g >> 4);
    for (uint32_t u = threadIdx.x; u < seg_units; u += kBlock) span[units + u] = src[u];
    if (threadIdx.x >= done && threadIdx.x < done + seg) my_at = 16u * units + lead + (threadIdx.x - done) * p.point_step;
    units += seg_units;
    done += seg;
  }
  __syncthreads();
  if (mine >= p.n) return;
  float4 v;
  float intensity;
  bool bad_time;
  const unsigned keep = decode_record(p, fc, reinterpret_cast<const uint32_t*>(span), my_at, &v, &intensity, &bad_time);
  store_record(p, mine, keep, v, intensity, bad_time, xyzt, intensities, keep_flags, words);
}

// Records too long for the LDS span: the same two aligned words a field, from global memory
__global__ __launch_bounds__(kBlock) void decode_direct_kernel(PointCloud2Plan p, FrameChange fc, const uint32_t* __restrict__ data,
                                                               float4* __restrict__ xyzt, float* __restrict__ intensities,
                                                               unsigned* __restrict__ keep_flags, unsigned* __restrict__ words) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  const uint64_t g = static_cast<uint64_t>(i / p.width) * p.row_step + static_cast<uint64_t>(i % p.width) * p.point_step;
  float4 v;
  float intensity;
  bool bad_time;
  // (per-record base: the offsets inside stay 32-bit)
  const unsigned keep = decode_record(p, fc, data + (g >> 2), static_cast<uint32_t>(g & 3u), &v, &intensity, &bad_time);
  store_record(p, i, keep, v, intensity, bad_time, xyzt, intensities, keep_flags, words);
}

// The kept points to the front in the message's order (by compact.hip's scan), and the first and last kept t
__global__ __launch_bounds__(kBlock) void place_kept_kernel(const float4* __restrict__ xyzt, const float* __restrict__ intensities,
                                                            uint32_t n, const unsigned* __restrict__ keep_flags,
                                                            const unsigned* __restrict__ inclusive, float4* __restrict__ out_xyzt,
                                                            float* __restrict__ out_intensities, unsigned* __restrict__ words) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || keep_flags[i] == 0u) return;
  const unsigned rank = inclusive[i];
  const float4 v = xyzt[i];
  out_xyzt[rank - 1u] = v;
  if (out_intensities != nullptr) out_intensities[rank - 1u] = intensities[i];
  if (rank == 1u) words[kWordFront] = __float_as_uint(v.w);
  if (rank == inclusive[n - 1u]) words[kWordBack] = __float_as_uint(v.w);
}

// bytes of LDS the span of a workgroup takes at most: 256 records, a row's alignment slack (< 32 bytes with the rounding up)
// for every row the workgroup can touch, and the word behind
unsigned lds_span_bytes(const PointCloud2Plan& p) {
  const uint64_t rows = p.width >= static_cast<uint32_t>(kBlock) ? 2 : kBlock / p.width + 2;
  const uint64_t bytes = static_cast<uint64_t>(kBlock) * p.point_step + 32 * rows + 16;
  return bytes <= kLdsBytes ? static_cast<unsigned>(bytes) : 0u;
}

}  // namespace
}  // namespace dliom

using namespace dliom;

extern "C" {

int dliom_point_cloud2_check(const dliom_point_cloud2* message, int mode, int64_t* time, double* rel_time_last) {
  PointCloud2Plan plan;
  int64_t stamp;
  DLIOM_TRY(point_cloud2_plan(message, mode, &plan, &stamp));
  if (time != nullptr) *time = stamp;
  if (rel_time_last != nullptr) *rel_time_last = plan.rel_time_last;
  return DLIOM_OK;
}

int dliom_point_cloud2_decode(dliom_ctx* ctx, const dliom_point_cloud2* message, int mode, const double sensor_to_tracking[7],
                              dliom_timed_cloud** out, int64_t* time, float origin[3]) {
  if (ctx == nullptr || out == nullptr || time == nullptr || origin == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  PointCloud2Plan plan;
  int64_t stamp;
  DLIOM_TRY(point_cloud2_plan(message, mode, &plan, &stamp));
  FrameChange fc{};
  if (sensor_to_tracking != nullptr) {
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(sensor_to_tracking[k])) return DLIOM_ERR_INVALID_ARGUMENT;
    fc.given = 1;
    for (int k = 0; k < 3; ++k) fc.t[k] = static_cast<float>(sensor_to_tracking[k]);
    fc.q = Quat4{static_cast<float>(sensor_to_tracking[3]), static_cast<float>(sensor_to_tracking[4]),
                 static_cast<float>(sensor_to_tracking[5]), static_cast<float>(sensor_to_tracking[6])};
  }
  const bool with_intensities = plan.intensity_kind != kPc2IntensityNone;
  dliom_timed_cloud* cloud = new dliom_timed_cloud;
  cloud->ctx = ctx;
  cloud->device = ctx->device;
  cloud->has_intensities = with_intensities;
  const int64_t n = plan.n;
  int st = DLIOM_OK;
  unsigned head[kWords] = {0u, 0u, 0u, 0u};
  int64_t kept = 0;
  if (n > 0) {
    st = hipSetDevice(ctx->device) == hipSuccess ? DLIOM_OK : DLIOM_ERR_HIP;
    // the object, with room for every point: what is kept is known only at the read-back, behind the last launch
    const size_t nn = static_cast<size_t>(n);
    if (st == DLIOM_OK) st = device_block_alloc(ctx->device, align256(16 * nn) + (with_intensities ? 4 * nn : 0), &cloud->base, &cloud->base_bytes);
    if (st == DLIOM_OK) {
      cloud->d_xyzt = static_cast<float4*>(cloud->base);
      if (with_intensities) cloud->d_intensities = reinterpret_cast<float*>(static_cast<char*>(cloud->base) + align256(16 * nn));
    }
    // behind the compaction's scratch: words | the message's bytes (+ the word behind) | xyzt of every point | intensities
    const size_t wb = 256, raw = align256(static_cast<size_t>(plan.used_bytes) + 32), all = align256(16 * nn);
    CompactScratch s{};
    if (st == DLIOM_OK) st = carve_compact(ctx, n, &s, wb + raw + all + (with_intensities ? align256(4 * nn) : 0), 4 * kWords);
    if (st == DLIOM_OK) {
      char* base = static_cast<char*>(s.extra);
      unsigned* words = reinterpret_cast<unsigned*>(base);
      float4* xyzt = reinterpret_cast<float4*>(base + wb + raw);
      float* intensities = with_intensities ? reinterpret_cast<float*>(base + wb + raw + all) : nullptr;
      const unsigned blocks = blocks_of(n, kBlock);
      const unsigned lds = lds_span_bytes(plan);
      if (hipMemcpyAsync(base + wb, message->data, static_cast<size_t>(plan.used_bytes), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        st = DLIOM_ERR_HIP;
      if (st == DLIOM_OK) {
        if (lds != 0u)
          hipLaunchKernelGGL(decode_lds_kernel, dim3(blocks), dim3(kBlock), lds, ctx->stream, plan, fc,
                             reinterpret_cast<const uint4*>(base + wb), xyzt, intensities, s.keep, words);
        else
          hipLaunchKernelGGL(decode_direct_kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, plan, fc,
                             reinterpret_cast<const uint32_t*>(base + wb), xyzt, intensities, s.keep, words);
        if (hipGetLastError() != hipSuccess) st = DLIOM_ERR_HIP;
      }
      if (st == DLIOM_OK) st = scan_kept(ctx, n, s);
      if (st == DLIOM_OK) {
        hipLaunchKernelGGL(place_kept_kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, xyzt, intensities, plan.n, s.keep, s.inclusive,
                           cloud->d_xyzt, cloud->d_intensities, words);
        if (hipGetLastError() != hipSuccess) st = DLIOM_ERR_HIP;
      }
      const GatherJob words_job{words, static_cast<unsigned>(kWords)};
      float max_sq;  // (not taken: a timed cloud has no bound; its consumers make their own)
      if (st == DLIOM_OK) st = read_kept(ctx, n, s, &words_job, &kept, &max_sq, head);
    }
    if (st == DLIOM_OK && head[kWordBadTime] != 0u) st = DLIOM_ERR_INVALID_ARGUMENT;
  }
  if (st != DLIOM_OK) {
    dliom_timed_cloud_destroy(cloud);
    return st;
  }
  cloud->n = kept;
  if (kept > 0) {
    std::memcpy(&cloud->front_t, &head[kWordFront], 4);
    std::memcpy(&cloud->back_t, &head[kWordBack], 4);
  }
  *out = cloud;
  *time = stamp;
  for (int k = 0; k < 3; ++k) origin[k] = fc.given != 0 ? fc.t[k] : 0.f;
  return DLIOM_OK;
}

int dliom_timed_cloud_destroy(dliom_timed_cloud* cloud) {
  if (cloud == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  if (cloud->base != nullptr) device_block_free(cloud->device, cloud->base, cloud->base_bytes);
  delete cloud;
  return DLIOM_OK;
}

int dliom_timed_cloud_size(const dliom_timed_cloud* cloud, int64_t* n) {
  if (cloud == nullptr || n == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *n = cloud->n;
  return DLIOM_OK;
}

int dliom_timed_cloud_has_intensities(const dliom_timed_cloud* cloud, int* has) {
  if (cloud == nullptr || has == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *has = cloud->has_intensities ? 1 : 0;
  return DLIOM_OK;
}

int dliom_timed_cloud_has_origin_index(const dliom_timed_cloud* cloud, int* has) {
  if (cloud == nullptr || has == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *has = cloud->has_origin_index ? 1 : 0;
  return DLIOM_OK;
}

int dliom_timed_cloud_download_origin_index(const dliom_timed_cloud* cloud, float* origin_index) {
  if (cloud == nullptr || origin_index == nullptr || !cloud->has_origin_index) return DLIOM_ERR_INVALID_ARGUMENT;
  if (cloud->n == 0) return DLIOM_OK;
  DLIOM_HIP_TRY(hipSetDevice(cloud->device));
  DLIOM_HIP_TRY(hipStreamSynchronize(cloud->ctx->stream));
  DLIOM_HIP_TRY(hipMemcpy(origin_index, cloud->d_origin_index, 4 * static_cast<size_t>(cloud->n), hipMemcpyDeviceToHost));
  return DLIOM_OK;
}

int dliom_timed_cloud_front_back_time(const dliom_timed_cloud* cloud, float* front, float* back) {
  if (cloud == nullptr || front == nullptr || back == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *front = cloud->front_t;
  *back = cloud->back_t;
  return DLIOM_OK;
}

int dliom_timed_cloud_download(const dliom_timed_cloud* cloud, float* xyzt, float* intensities) {
  if (cloud == nullptr || (intensities != nullptr && !cloud->has_intensities)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (cloud->n == 0) return DLIOM_OK;
  DLIOM_HIP_TRY(hipSetDevice(cloud->device));
  DLIOM_HIP_TRY(hipStreamSynchronize(cloud->ctx->stream));
  const size_t n = static_cast<size_t>(cloud->n);
  if (xyzt != nullptr) DLIOM_HIP_TRY(hipMemcpy(xyzt, cloud->d_xyzt, 16 * n, hipMemcpyDeviceToHost));
  if (intensities != nullptr) DLIOM_HIP_TRY(hipMemcpy(intensities, cloud->d_intensities, 4 * n, hipMemcpyDeviceToHost));
  return DLIOM_OK;
}

}  // extern "C"

namespace dliom {
// cvtPointCloud: a timed cloud's xyz as they stand, and the largest squared norm for the cloud's bound
__global__ __launch_bounds__(256) void timed_points_kernel(const float4* __restrict__ xyzt, int n, float* __restrict__ x,
                                                           float* __restrict__ y, float* __restrict__ z, unsigned* max_sq) {
  const int i = static_cast<int>(blockIdx.x) * 256 + threadIdx.x;
  unsigned word = 0u;
  if (i < n) {
    const float4 p = xyzt[i];
    x[i] = p.x;
    y[i] = p.y;
    z[i] = p.z;
    word = norm_word(p.x, p.y, p.z);
  }
  note_kept(word, max_sq);
}
}  // namespace dliom

extern "C" int dliom_timed_cloud_points(dliom_ctx* ctx, const dliom_timed_cloud* in, dliom_cloud** out) {
  if (out != nullptr) *out = nullptr;
  if (ctx == nullptr || in == nullptr || out == nullptr || in->ctx != ctx || in->n < 0 || in->n > (int64_t{1} << 30))
    return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  if (in->n == 0) return empty_cloud(ctx, out);
  const int n = static_cast<int>(in->n);
  DLIOM_TRY(ctx->misc.reserve(256));
  unsigned* const max_sq = ctx->misc.as<unsigned>();
  const FillJob fill{max_sq, 4, 0u};
  DLIOM_TRY(fill_multi(ctx, &fill, 1));
  float *x, *y, *z;
  DLIOM_TRY(alloc_device_cloud(ctx, n, out, &x, &y, &z));
  hipLaunchKernelGGL(timed_points_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, ctx->stream, in->d_xyzt, n, x, y, z, max_sq);
  int st = hipGetLastError() == hipSuccess ? DLIOM_OK : DLIOM_ERR_HIP;
  unsigned* const host = pinned_at<unsigned>(ctx, kPinReadback);
  const GatherJob job{max_sq, 1};
  if (st == DLIOM_OK) st = gather_and_wait(ctx, &job, 1, host);
  float sq = 0.f;
  if (st == DLIOM_OK) {
    std::memcpy(&sq, host, 4);
    st = finish_device_cloud(ctx, *out, std::sqrt(sq));  // sqrt is monotone: the max of the norms
  }
  if (st != DLIOM_OK) {
    dliom_cloud_destroy(*out);
    *out = nullptr;
  }
  return st;
}

// what the consumers (preprocess.hip, assemble.hip) take of an object
namespace dliom {
int timed_cloud_view(const dliom_timed_cloud* cloud, const dliom_ctx* ctx, int64_t* n, const float4** d_xyzt, const float** d_intensities,
                     float* front_t) {
  if (cloud == nullptr || cloud->ctx != ctx) return DLIOM_ERR_INVALID_ARGUMENT;
  *n = cloud->n;
  *d_xyzt = cloud->d_xyzt;
  if (d_intensities != nullptr) *d_intensities = cloud->n > 0 ? cloud->d_intensities : nullptr;
  if (front_t != nullptr) *front_t = cloud->front_t;
  return DLIOM_OK;
}
int timed_cloud_origin_index(const dliom_timed_cloud* cloud, bool* has, const float** d_origin_index) {
  if (cloud == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *has = cloud->has_origin_index;
  if (d_origin_index != nullptr) *d_origin_index = cloud->n > 0 ? cloud->d_origin_index : nullptr;
  return DLIOM_OK;
}
}  // namespace dliom
