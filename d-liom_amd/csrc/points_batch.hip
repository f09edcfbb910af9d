// io::PointsBatch in HBM and the stages of the points-processor pipeline that only move or recolour its points
// (DESIGN.md section 3.14): ColoringPointsProcessor, IntensityToColorPointsProcessor, FixedRatioSamplingPointsProcessor
// over common::FixedRatioSampler, and the per-point loops of PlyWritingPointsProcessor / PcdWritingPointsProcessor as
// packed records.  The compacting stages that decide by geometry (range filter, outlier removal) live in outlier.hip and
// the head of the export in assemble.hip; all of them share compact.hip's scan, scatter and attribute gather.
//
// Everything here equals the reference byte for byte: the colour stages are float arithmetic in the reference's order
// (no contraction, IEEE division), the sampler's decisions are the sequential loop's (proven per call, below), and the
// records are copies of bytes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "voxel_hash.h"

namespace dliom {
namespace {

constexpr int kBlock = 256;
// Pulses a thread replays in the sampler.  64: a 64 x 1024 scan gives 1024 threads of 64 double divisions each, and the
// words a repair pass touches stay few.
constexpr int kChunk = 64;
// Points a workgroup packs.  256 records of any size are a whole number of dwords (and of 256-byte lines), so every
// workgroup's part of the output starts dword-aligned and only the last one has a tail of 1 to 3 bytes.
constexpr int kPackPoints = 256;
constexpr int kMaxRecord = 19;

inline unsigned blocks_of(int64_t n) { return dliom::blocks_of(n, kBlock); }

// common::Clamp (common/math.h:32-40): NaN fails both comparisons and passes through
__device__ __forceinline__ float clamp_ref(float v, float lo, float hi) {
  if (v > hi) return hi;
  if (v < lo) return lo;
  return v;
}

__global__ __launch_bounds__(kBlock) void intensity_to_color_kernel(const float* __restrict__ intensities, unsigned n, float lo,
                                                                    float hi, float* __restrict__ colors) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float gray = clamp_ref((intensities[i] - lo) / (hi - lo), 0.f, 1.f);
  colors[3 * static_cast<size_t>(i)] = gray;
  colors[3 * static_cast<size_t>(i) + 1] = gray;
  colors[3 * static_cast<size_t>(i) + 2] = gray;
}

// ---- the sampler ---------------------------------------------------------------------------------------------------
// Chunk c holds the pulses [c * kChunk, (c + 1) * kChunk) of the batch.  start[c]: the value of num_samples it assumes
// on entry; end[c]: what it leaves.  A thread replays its chunk with the reference's expression.
// First pass (only_bad == 0): chunk 0 starts from the sampler's true state; the others guess -- a sampler that began at
// (0, 0) holds about ceil(ratio * pulses) samples.  Nothing rests on the guess except how many passes the call takes: a
// wrong start is found by the check below.  Repair passes (only_bad) re-run the chunks the check marked, from the start
// it corrected.
__global__ __launch_bounds__(kBlock) void sampler_chunks_kernel(unsigned n, unsigned chunks, long long pulses0, long long samples0,
                                                                double ratio, long long* __restrict__ start,
                                                                long long* __restrict__ end, const unsigned* __restrict__ bad,
                                                                int only_bad, unsigned* __restrict__ keep) {
  const unsigned c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= chunks || (only_bad && bad[c] == 0u)) return;
  const unsigned first = c * kChunk, last = min(n, first + kChunk);
  long long pulses = pulses0 + first;
  long long samples;
  if (only_bad) {
    samples = start[c];
  } else {
    samples = samples0;
    if (c > 0) {
      const double guess = ceil(ratio * static_cast<double>(pulses));
      const long long hi = samples0 + first;  // every pulse of the batch so far kept
      samples = guess < static_cast<double>(samples0) ? samples0 : guess > static_cast<double>(hi) ? hi : static_cast<long long>(guess);
    }
    start[c] = samples;
  }
  for (unsigned i = first; i < last; ++i) {
    ++pulses;  // Pulse(): ++num_pulses_; static_cast<double>(num_samples_) / num_pulses_ < ratio_
    const bool k = static_cast<double>(samples) / static_cast<double>(pulses) < ratio;
    if (k) ++samples;
    keep[i] = k ? 1u : 0u;
  }
  end[c] = samples;
}

// The proof: chunk c's assumed start against chunk c - 1's end.  A wrong one is corrected and marked for the next pass;
// words[0] counts them.  (start[0] is the sampler's true state.)
__global__ __launch_bounds__(kBlock) void sampler_check_kernel(unsigned chunks, long long* __restrict__ start,
                                                               const long long* __restrict__ end, unsigned* __restrict__ bad,
                                                               unsigned* __restrict__ words) {
  const unsigned c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= chunks) return;
  unsigned wrong = 0;
  if (c > 0 && start[c] != end[c - 1]) {
    start[c] = end[c - 1];
    wrong = 1;
  }
  bad[c] = wrong;
  if (wrong) atomicAdd(&words[0], 1u);
}

// ---- the writers' records ------------------------------------------------------------------------------------------
// FloatComponentToUint8 (io/color.h:35-38): uint8(lround(Clamp(c, 0.f, 1.f) * 255))
__device__ __forceinline__ unsigned to_uint8(float c) {
  return static_cast<unsigned>(lroundf(clamp_ref(c, 0.f, 1.f) * 255.f)) & 0xffu;
}

struct PackArgs {
  const float *x, *y, *z, *intensities, *colors;  // intensities / colors null: not in the record (or `rgb` for every point)
  float rgb[3];
  int single_color;
  int with_colors, with_intensities, pcd;
  unsigned n, record;  // bytes a record
};

// A workgroup stages its kPackPoints records in LDS -- records of 15 and 19 bytes are not dword-aligned, and a byte store
// a lane to HBM would be a partial write of a line each -- and writes them out as whole dwords, one a lane, coalesced.
// The last workgroup's 1 to 3 remaining bytes go out as bytes: nothing at or beyond n * record is touched.
__global__ __launch_bounds__(kPackPoints) void pack_records_kernel(PackArgs a, unsigned char* __restrict__ out) {
  __shared__ unsigned stage[kPackPoints * kMaxRecord / 4];
  unsigned char* bytes = reinterpret_cast<unsigned char*>(stage);
  const unsigned first = blockIdx.x * kPackPoints;
  const unsigned i = first + threadIdx.x;
  if (i < a.n) {
    unsigned w[5];
    w[0] = __float_as_uint(a.x[i]);
    w[1] = __float_as_uint(a.y[i]);
    w[2] = __float_as_uint(a.z[i]);
    unsigned char* rec = bytes + threadIdx.x * a.record;
    unsigned r8 = 0, g8 = 0, b8 = 0;
    if (a.with_colors) {
      const float r = a.single_color ? a.rgb[0] : a.colors[3 * static_cast<size_t>(i)];
      const float g = a.single_color ? a.rgb[1] : a.colors[3 * static_cast<size_t>(i) + 1];
      const float b = a.single_color ? a.rgb[2] : a.colors[3 * static_cast<size_t>(i) + 2];
      r8 = to_uint8(r);
      g8 = to_uint8(g);
      b8 = to_uint8(b);
    }
    if ((a.record & 3u) == 0u) {  // 12 or 16 bytes: the record is dword-aligned in LDS
      unsigned* rw = reinterpret_cast<unsigned*>(rec);
      rw[0] = w[0];
      rw[1] = w[1];
      rw[2] = w[2];
      if (a.pcd && a.with_colors) rw[3] = b8 | (g8 << 8) | (r8 << 16);         // b g r 0
      else if (a.with_intensities) rw[3] = __float_as_uint(a.intensities[i]);  // PLY, 16 bytes: x y z intensity
    } else {  // PLY with colours, 15 or 19 bytes
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        rec[4 * k] = static_cast<unsigned char>(w[k]);
        rec[4 * k + 1] = static_cast<unsigned char>(w[k] >> 8);
        rec[4 * k + 2] = static_cast<unsigned char>(w[k] >> 16);
        rec[4 * k + 3] = static_cast<unsigned char>(w[k] >> 24);
      }
      rec[12] = static_cast<unsigned char>(r8);
      rec[13] = static_cast<unsigned char>(g8);
      rec[14] = static_cast<unsigned char>(b8);
      if (a.with_intensities) {
        const unsigned v = __float_as_uint(a.intensities[i]);
        rec[15] = static_cast<unsigned char>(v);
        rec[16] = static_cast<unsigned char>(v >> 8);
        rec[17] = static_cast<unsigned char>(v >> 16);
        rec[18] = static_cast<unsigned char>(v >> 24);
      }
    }
  }
  __syncthreads();
  const unsigned points_here = min(static_cast<unsigned>(kPackPoints), a.n - first);
  const unsigned total = points_here * a.record;  // bytes of this workgroup
  const size_t base = static_cast<size_t>(first) * a.record;  // a multiple of 256
  unsigned* out_words = reinterpret_cast<unsigned*>(out + base);
  for (unsigned w = threadIdx.x; w < total / 4u; w += kPackPoints) out_words[w] = stage[w];
  const unsigned tail = total & 3u;
  if (threadIdx.x < tail) out[base + (total & ~3u) + threadIdx.x] = bytes[(total & ~3u) + threadIdx.x];
}

int copy_text(const std::string& text, char* buffer, int64_t capacity, int64_t* length) {
  *length = static_cast<int64_t>(text.size());
  if (buffer == nullptr || capacity < *length) return DLIOM_ERR_CAPACITY;
  std::memcpy(buffer, text.data(), text.size());
  return DLIOM_OK;
}

// std::setw(15) << std::setfill('0') << num_points
std::string padded_count(int64_t num_points) {
  char text[32];
  std::snprintf(text, sizeof text, "%015lld", static_cast<long long>(num_points));
  return text;
}

}  // namespace
}  // namespace dliom

using namespace dliom;

struct dliom_fixed_ratio_sampler {
  double ratio = 0.0;
  int64_t num_pulses = 0, num_samples = 0;
  int64_t chunks = 0, repaired_chunks = 0, repair_passes = 0;
};

extern "C" {

int dliom_points_batch_create(dliom_ctx* ctx, const float* points_xyz, int64_t n, const float origin[3], const float* intensities,
                              const float* colors_rgb, int64_t num_colors, dliom_points_batch** out) {
  if (ctx == nullptr || out == nullptr || origin == nullptr || n < 0 || n > INT32_MAX || (n > 0 && points_xyz == nullptr) ||
      (num_colors != 0 && num_colors != n) || (num_colors > 0 && colors_rgb == nullptr))
    return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  dliom_points_batch* b = new dliom_points_batch;
  b->ctx = ctx;
  std::memcpy(b->origin, origin, 12);
  int st = dliom_cloud_create(ctx, points_xyz, n, &b->cloud);
  const size_t un = static_cast<size_t>(n);
  if (st == DLIOM_OK && intensities != nullptr) st = b->intensities.alloc(ctx, un);
  if (st == DLIOM_OK && num_colors > 0) st = b->colors.alloc(ctx, 3 * un);
  if (st == DLIOM_OK && b->intensities.p != nullptr &&
      hipMemcpyAsync(b->intensities.p, intensities, 4 * un, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    st = DLIOM_ERR_HIP;
  if (st == DLIOM_OK && b->colors.p != nullptr &&
      hipMemcpyAsync(b->colors.p, colors_rgb, 12 * un, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    st = DLIOM_ERR_HIP;
  if (st == DLIOM_OK && (b->intensities.p != nullptr || b->colors.p != nullptr)) {
    // the host buffers may be reused by the caller as soon as we return
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) st = DLIOM_ERR_HIP;
    ++ctx->host_syncs;
  }
  if (st != DLIOM_OK) {
    if (b->cloud != nullptr) dliom_points_batch_destroy(b);
    else delete b;
    return st;
  }
  *out = b;
  return DLIOM_OK;
}

int dliom_points_batch_destroy(dliom_points_batch* b) {
  if (b == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  b->intensities.release(b->ctx);
  b->colors.release(b->ctx);
  if (b->cloud != nullptr) dliom_cloud_destroy(b->cloud);
  delete b;
  return DLIOM_OK;
}

int dliom_points_batch_size(const dliom_points_batch* b, int64_t* n) {
  if (b == nullptr || n == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *n = b->cloud->n;
  return DLIOM_OK;
}

int dliom_points_batch_has_intensities(const dliom_points_batch* b, int* has) {
  if (b == nullptr || has == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *has = b->has_intensities() ? 1 : 0;
  return DLIOM_OK;
}

int dliom_points_batch_has_colors(const dliom_points_batch* b, int* has) {
  if (b == nullptr || has == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *has = b->has_colors() ? 1 : 0;
  return DLIOM_OK;
}

int dliom_points_batch_cloud(const dliom_points_batch* b, const dliom_cloud** cloud) {
  if (b == nullptr || cloud == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *cloud = b->cloud;
  return DLIOM_OK;
}

int dliom_points_batch_origin(const dliom_points_batch* b, float origin[3]) {
  if (b == nullptr || origin == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  std::memcpy(origin, b->origin, 12);
  return DLIOM_OK;
}

int dliom_points_batch_download(const dliom_points_batch* b, float* points_xyz, float* intensities, float* colors_rgb) {
  if (b == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  const size_t n = static_cast<size_t>(b->cloud->n);
  if (n == 0) return DLIOM_OK;
  if ((intensities != nullptr && !b->has_intensities()) || (colors_rgb != nullptr && !b->has_colors())) return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_ctx* ctx = b->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  if (points_xyz != nullptr) DLIOM_TRY(dliom_cloud_download(b->cloud, points_xyz));
  bool copies = false;
  if (intensities != nullptr) {
    DLIOM_HIP_TRY(hipMemcpyAsync(intensities, b->intensities.p, 4 * n, hipMemcpyDeviceToHost, ctx->stream));
    copies = true;
  }
  if (colors_rgb != nullptr) {
    if (b->single_color) {
      for (size_t i = 0; i < n; ++i) std::memcpy(colors_rgb + 3 * i, b->rgb, 12);
    } else {
      DLIOM_HIP_TRY(hipMemcpyAsync(colors_rgb, b->colors.p, 12 * n, hipMemcpyDeviceToHost, ctx->stream));
      copies = true;
    }
  }
  if (copies) {
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    ++ctx->host_syncs;
  }
  return DLIOM_OK;
}

int dliom_points_batch_color(dliom_points_batch* b, const float rgb[3]) {
  if (b == nullptr || rgb == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  if (b->cloud->n == 0) return DLIOM_OK;  // colors.clear(), and nothing pushed
  b->colors.release(b->ctx);
  b->single_color = true;
  std::memcpy(b->rgb, rgb, 12);
  return DLIOM_OK;
}

int dliom_points_batch_intensity_to_color(dliom_points_batch* b, float min_intensity, float max_intensity) {
  if (b == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  if (!b->has_intensities()) return DLIOM_OK;
  dliom_ctx* ctx = b->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const unsigned n = static_cast<unsigned>(b->cloud->n);
  AttrBlock fresh;  // swapped in only once the launch is enqueued: a failed call leaves the batch as it was
  if (b->colors.p == nullptr) DLIOM_TRY(fresh.alloc(ctx, 3 * static_cast<size_t>(n)));
  float* colors = b->colors.p != nullptr ? b->colors.p : fresh.p;
  hipLaunchKernelGGL(intensity_to_color_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, b->intensities.p, n, min_intensity,
                     max_intensity, colors);
  if (hipGetLastError() != hipSuccess) {
    fresh.release(ctx);
    return DLIOM_ERR_HIP;
  }
  if (fresh.p != nullptr) b->colors = fresh;
  b->single_color = false;
  return DLIOM_OK;
}

int dliom_fixed_ratio_sampler_create(double ratio, dliom_fixed_ratio_sampler** out) {
  if (out == nullptr || !(ratio >= 0.0) || !(ratio <= 1.0)) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = new dliom_fixed_ratio_sampler;
  (*out)->ratio = ratio;
  return DLIOM_OK;
}

int dliom_fixed_ratio_sampler_destroy(dliom_fixed_ratio_sampler* s) {
  if (s == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  delete s;
  return DLIOM_OK;
}

int dliom_fixed_ratio_sampler_reset(dliom_fixed_ratio_sampler* s) {
  if (s == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  s->num_pulses = s->num_samples = 0;
  return DLIOM_OK;
}

int dliom_fixed_ratio_sampler_state(const dliom_fixed_ratio_sampler* s, int64_t* num_pulses, int64_t* num_samples) {
  if (s == nullptr || num_pulses == nullptr || num_samples == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *num_pulses = s->num_pulses;
  *num_samples = s->num_samples;
  return DLIOM_OK;
}

int dliom_fixed_ratio_sampler_stats(const dliom_fixed_ratio_sampler* s, dliom_fixed_ratio_sampler_statistics* out) {
  if (s == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  out->chunks = s->chunks;
  out->repaired_chunks = s->repaired_chunks;
  out->repair_passes = s->repair_passes;
  return DLIOM_OK;
}

int dliom_points_batch_fixed_ratio_sample(dliom_fixed_ratio_sampler* sampler, dliom_points_batch* b) {
  if (sampler == nullptr || b == nullptr || b->cloud->n > INT32_MAX) return DLIOM_ERR_INVALID_ARGUMENT;
  const int64_t n64 = b->cloud->n;
  if (n64 == 0) return DLIOM_OK;
  dliom_ctx* ctx = b->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const unsigned n = static_cast<unsigned>(n64);
  const unsigned chunks = (n + kChunk - 1) / kChunk;
  // behind the compaction's scratch: start | end | bad | words
  const size_t per8 = align256(8 * static_cast<size_t>(chunks)), per4 = align256(4 * static_cast<size_t>(chunks));
  CompactScratch s;
  DLIOM_TRY(carve_compact(ctx, n64, &s, 2 * per8 + per4 + 256));
  char* e = static_cast<char*>(s.extra);
  long long* d_start = reinterpret_cast<long long*>(e);
  long long* d_end = reinterpret_cast<long long*>(e + per8);
  unsigned* d_bad = reinterpret_cast<unsigned*>(e + 2 * per8);
  unsigned* d_words = reinterpret_cast<unsigned*>(e + 2 * per8 + per4);
  int64_t repaired = 0, passes = 0, kept = 0;
  const dliom_cloud* in = b->cloud;
  for (unsigned pass = 0;; ++pass) {
    if (pass > chunks) return DLIOM_ERR_INTERNAL;  // (cannot happen: pass p proves the first p + 1 chunks)
    const FillJob fills[2] = {{d_words, 4, 0u}, {s.max_sq, 4, 0u}};
    DLIOM_TRY(fill_multi(ctx, fills, 2));
    hipLaunchKernelGGL(sampler_chunks_kernel, dim3(blocks_of(chunks)), dim3(kBlock), 0, ctx->stream, n, chunks,
                       static_cast<long long>(sampler->num_pulses), static_cast<long long>(sampler->num_samples), sampler->ratio, d_start,
                       d_end, d_bad, pass > 0 ? 1 : 0, s.keep);
    hipLaunchKernelGGL(sampler_check_kernel, dim3(blocks_of(chunks)), dim3(kBlock), 0, ctx->stream, chunks, d_start, d_end, d_bad,
                       d_words);
    DLIOM_HIP_TRY(hipGetLastError());
    DLIOM_TRY(max_of_kept(ctx, in->d_x, in->d_y, in->d_z, n64, s));
    unsigned wrong = 0;
    // the number of wrong starts rides in the read-back of the kept count; while it is not zero nothing is compacted
    DLIOM_TRY(compact_batch(b, s, d_words, &wrong, &kept));
    if (wrong == 0u) break;
    repaired += wrong;
    ++passes;
  }
  sampler->num_pulses += n64;
  sampler->num_samples += kept;
  sampler->chunks += chunks;
  sampler->repaired_chunks += repaired;
  sampler->repair_passes += passes;
  return DLIOM_OK;
}

int dliom_points_batch_pack(const dliom_points_batch* b, int format, int with_colors, int with_intensities, uint8_t* bytes,
                            int64_t capacity, int64_t* num_bytes) {
  if (b == nullptr || num_bytes == nullptr || capacity < 0 || (format != DLIOM_PACK_PLY && format != DLIOM_PACK_PCD) ||
      (format == DLIOM_PACK_PCD && with_intensities != 0))
    return DLIOM_ERR_INVALID_ARGUMENT;
  *num_bytes = 0;
  const int64_t n = b->cloud->n;
  if (n == 0) return DLIOM_OK;  // the writers pass an empty batch on before they look at it
  const bool colors = with_colors != 0, intensities = with_intensities != 0;
  if ((colors && !b->has_colors()) || (intensities && !b->has_intensities())) return DLIOM_ERR_INVALID_ARGUMENT;  // CHECK_EQ
  if (format == DLIOM_PACK_PCD && !colors && b->has_colors()) return DLIOM_ERR_INVALID_ARGUMENT;
  const unsigned record = format == DLIOM_PACK_PCD ? (colors ? 16u : 12u) : 12u + (colors ? 3u : 0u) + (intensities ? 4u : 0u);
  *num_bytes = n * record;
  if (bytes == nullptr) return DLIOM_OK;
  if (capacity < *num_bytes) return DLIOM_ERR_CAPACITY;
  dliom_ctx* ctx = b->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const unsigned groups = dliom::blocks_of(n, kPackPoints);
  DLIOM_TRY(ctx->outlier.reserve(static_cast<size_t>(groups) * kPackPoints * record));
  PackArgs a{};
  a.x = b->cloud->d_x;
  a.y = b->cloud->d_y;
  a.z = b->cloud->d_z;
  a.intensities = intensities ? b->intensities.p : nullptr;
  a.colors = colors && !b->single_color ? b->colors.p : nullptr;
  std::memcpy(a.rgb, b->rgb, 12);
  a.single_color = b->single_color ? 1 : 0;
  a.with_colors = colors ? 1 : 0;
  a.with_intensities = intensities ? 1 : 0;
  a.pcd = format == DLIOM_PACK_PCD ? 1 : 0;
  a.n = static_cast<unsigned>(n);
  a.record = record;
  hipLaunchKernelGGL(pack_records_kernel, dim3(groups), dim3(kPackPoints), 0, ctx->stream, a, ctx->outlier.as<unsigned char>());
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipMemcpyAsync(bytes, ctx->outlier.p, static_cast<size_t>(*num_bytes), hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  return DLIOM_OK;
}

int dliom_ply_header(int with_colors, int with_intensities, int64_t num_points, char* buffer, int64_t capacity, int64_t* length) {
  if (length == nullptr || capacity < 0 || num_points < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  const std::string text = std::string("ply\nformat binary_little_endian 1.0\ncomment generated by Cartographer\nelement vertex ") +
                           padded_count(num_points) + "\nproperty float x\nproperty float y\nproperty float z\n" +
                           (with_colors ? "property uchar red\nproperty uchar green\nproperty uchar blue\n" : "") +
                           (with_intensities ? "property float intensity\n" : "") + "end_header\n";
  return copy_text(text, buffer, capacity, length);
}

int dliom_pcd_header(int with_colors, int64_t num_points, char* buffer, int64_t capacity, int64_t* length) {
  if (length == nullptr || capacity < 0 || num_points < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  const std::string count = padded_count(num_points);
  const std::string text = std::string("# generated by Cartographer\nVERSION .7\nFIELDS x y z") + (with_colors ? " rgb" : "") +
                           "\nSIZE 4 4 4" + (with_colors ? " 4" : "") + "\nTYPE F F F" + (with_colors ? " U" : "") + "\nCOUNT 1 1 1" +
                           (with_colors ? " 1" : "") + "\nWIDTH " + count + "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " + count +
                           "\nDATA binary\n";
  return copy_text(text, buffer, capacity, length);
}

}  // extern "C"
